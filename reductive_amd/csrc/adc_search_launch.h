// adc_search_launch.h -- what the translation units of the ADC searches share on the host: the dispatch from run-time
// values to instantiated kernels, the launch structs that pqhip_adc.hip fills (it owns the policy of every search:
// checks, queries per pass, list length, grids, scratch, the plan and the merge -- one exhaustive and one list driver,
// which a code format enters with a SearchRoute / ListsRoute) and the row mask with the launchers of the masked
// producers, which pqhip_adc_masked.hip instantiates so that the build compiles them beside pqhip_adc.hip.
#pragma once
#include "pqhip_internal.h"

#include "launch_dispatch.h"   // dispatch_int: here Vs is the list of instantiated values

namespace pqh {

// the list lengths of the searches: 64 L entries per (wave, query)
template <typename F>
int32_t dispatch_list_regs(int L, F&& f) { return dispatch_int<1, 2, 4, 8, 16>(L, f); }
// the queries of one pass over the codes
template <typename F>
int32_t dispatch_queries_per_pass(int nq_pass, F&& f) { return dispatch_int<8, 4, 1>(nq_pass, f); }

struct SearchLaunch {
    int64_t n, c_rs, rows_per_wg;
    unsigned grid;
    int M, K, k;
    const float* scales;     // IP: [n] row scales or null; unused by the distance search
    unsigned* part_k;
    uint64_t* part_i;
    int* err;
    hipStream_t st;
    const uint32_t* allow;   // row mask (ceil(n / 32) words) or null: the masked producers serve a non-null one
};

struct ListsLaunch {
    int64_t n, c_rs;
    unsigned G, nq;          // grid (G, nq)
    int M, K, k, n_probe;
    const float* scales;     // residual distance search: the row terms
    const float* bias;       // residual searches: probe bias rows of the launch's queries, else null
    int64_t b_rs;
    const int64_t *seg_begin, *seg_cum;
    unsigned* part_k;
    uint64_t* part_i;
    int* err;
    hipStream_t st;
    const uint32_t* allow;   // row mask in position order or null
};

// Inputs of the residual searches beside those of the plain ones: bias [nq][b_rs] f32, one value per (query, probe
// slot), and for the distance the row terms [n] f32 (they travel in the place of the scales).
struct ListsResidual {
    const float* bias;
    int64_t b_rs;
};

// A row mask as the search routines take it: the words and the launchers of the masked producers.  The launchers come
// with the mask so that pqhip_adc.hip refers to nothing of pqhip_adc_masked.hip: the dependency runs one way, from the
// masked entry points to the routines, and a program linked without the masked unit lacks those entry points only.
// search: ip = the similarity form; nq_pass in {8, 4, 1}; L and nvb as chosen for the unmasked producers
// (search_list_regs, search_nv_bucket / lists_nv_bucket); lds: the same budget.
using SearchProducer = int32_t (*)(bool ip, int nq_pass, int L, int nvb, const SearchLaunch& a, const void* codes, const float* lut,
                                   size_t lds);
using ListsProducer = int32_t (*)(bool ip, int L, int nvb, const ListsLaunch& a, const void* codes, const float* lut, size_t lds);
struct RowMask {
    const uint32_t* words;
    SearchProducer search;
    ListsProducer lists;
};

// What a code format brings to the two drivers below; everything else of a search is one policy.
struct SearchRoute {         // exhaustive searches
    int64_t row_len;         // least row stride: M codes, ceil(M / 2) bytes of packed rows
    size_t table_bytes;      // the LDS table image of one query
    int nvb;                 // code dwords fetched per row, an instantiated width
    bool multi_query;        // 8 / 4 queries per pass where they fit (the generic kernels take one)
    int64_t forced_wgs;      // producer workgroups when > 0, else one per CU with at least 4,096 rows
    SearchProducer launch;
};
struct ListsRoute {          // list searches
    int64_t row_len;
    size_t table_bytes;
    int nvb;
    ListsProducer launch;
};

// pqhip_adc.hip: the exhaustive and the list search from the point where a caller has made the checks that need its
// format -- EINVAL for null cb and negative counts, ENODEV, and EUNSUPPORTED for what the format does not serve, in this
// order -- and has chosen its route.  They go on with the remaining checks in the order of every search (EUNSUPPORTED,
// nq == 0, null pointers, ESHAPE), then the padding-only path, the grid resp. G, the chunking, the scratch layout and
// the plan -> producer -> merge loop.  res != null: the residual searches; d_scales then holds the row terms of the
// distance search (required).
int32_t adc_search_run(bool ip, pqhip_codebook* cb, int32_t slot, const SearchRoute& r, const float* d_tables, int64_t nq,
                       const void* d_codes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales, int32_t k,
                       float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream);
int32_t adc_search_lists_run(bool ip, pqhip_codebook* cb, int32_t slot, const ListsRoute& r, const float* d_tables, int64_t nq,
                             const void* d_codes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const int64_t* d_list_off,
                             int64_t n_lists, const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales,
                             int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream,
                             const ListsResidual* res);

// pqhip_adc.hip: adc_search / adc_search_lists behind the masked entry points (mask.words != null)
int32_t adc_search_masked(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                          int32_t code_bytes, int64_t n, int64_t c_rs, const float* d_scales, int32_t k, float* d_val, int64_t v_rs,
                          int64_t* d_idx, int64_t i_rs, void* stream, const RowMask& mask);
int32_t adc_search_lists_masked(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_list_off, int64_t n_lists,
                                const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales, int32_t k,
                                float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream, const ListsResidual* res,
                                const RowMask& mask);

// pqhip_adc.hip: what the range searches (pqhip_adc_range.hip) take from the searches' policy, so that a range call and
// the search of the same shape make the same choices: the code dwords fetched per row (0: no instantiation), the
// workgroups that share a query of a list call, the scratch bound of one chunk of queries, and the launch of
// k_adc_lists_plan -- the only reader of the offsets and probes, for both.
int search_nv_bucket(int nv);
int search_list_regs(int k);                                   // L: 64 L >= k entries per (wave, query)
size_t search_lds(size_t table_bytes, int nq, int L);          // a producer's dynamic LDS: max(table image + queues, combine lists)
int lists_nv_bucket(int nv);
int64_t lists_wgs_per_query(int64_t n, int64_t n_lists, int64_t n_probe, int64_t nq, int n_cus);
constexpr size_t kListsScratchBytes = 512u << 20;   // plan + partial lists of one chunk of queries
int32_t launch_lists_plan(const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int n_probe, int64_t p_rs, int64_t n,
                          int64_t* seg_begin, int64_t* seg_cum, unsigned nq, int* err, hipStream_t st);

// pqhip_adc.hip: the door to k_adc_search_merge for a producer of another unit (pqhip_adc_among.hip): merges the G partial
// lists [nq][G][64 L] of nq <= 65535 queries into the outputs; G == 0 writes the padding only, for any nq.
int32_t adc_search_merge(bool ip, int L, int64_t nq, int G, int k, const unsigned* part_k, const uint64_t* part_i, float* d_val,
                         int64_t v_rs, int64_t* d_idx, int64_t i_rs, hipStream_t st);

// pqhip_adc_packed4_lists.hip: the list producers over 4-bit packed codes (kernels_adc_packed4.hip.h), a unit of their
// own so that the build compiles them beside the exhaustive ones.  nvb in {2, 8, 13} packed dwords; a.allow and a.bias
// may be null.
int32_t launch_lists_packed4(bool ip, int L, int nvb, const ListsLaunch& a, const void* packed, const float* lut, size_t lds);

}  // namespace pqh
