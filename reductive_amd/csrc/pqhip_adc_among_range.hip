// pqhip_adc_among_range.hip -- ADC range search among given rows (include/pqhip.h: pqhip_adc_among_range_f32_dev,
// pqhip_adc_ip_among_range_f32_dev): the two entry points, their policy (checks, workgroups per query, chunks, scratch,
// the count / scan / fill sequence) and the instantiations of k_adc_among_range_u8 (kernels_adc_among_range.hip.h).  The
// NV bucket and the scratch bound of a chunk of queries are the list searches' (adc_search_launch.h), the workgroups per
// query are chosen as pqhip_adc_among.hip chooses them, the scan is the range searches' k_adc_range_scan.  A unit of its
// own so that the build compiles its 32 kernels beside the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_adc_among_range.hip.h"

using namespace pqhip;

namespace pqh {

constexpr int64_t kAmongRangeScanMax = 1 << 20;   // partial counts of one chunk of queries: what one scan launch sums
constexpr int64_t kAmongRangeSpanMax = 1ll << 31;   // places a query's bitmap covers at most: 256 MB, half the scratch bound
constexpr size_t kAmongRangeStaticLds = 2 * kRangeWaves * sizeof(int) + kRangeWaves * sizeof(long long);

struct AmongRangeLaunch {
    int64_t n, c_rs;
    unsigned G, nq;          // grid (G, nq)
    int M, K;
    const float* extra;      // scales (IP) or row terms (residual distance) or null
    const float* thr;
    const int64_t *lims, *ids;
    int64_t n_ids;
    const int64_t* row_list; // residual: [n] list of every row, else null
    int64_t n_lists;
    const float* bias;       // residual: bias rows of the launch's queries, else null
    int64_t b_rs;
    int64_t* part;           // [nq][G]
    unsigned long long* hits;   // [nq][bm_words]
    int64_t bm_words;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
    int* err;
    hipStream_t st;
};

template <bool IP, bool RESIDUAL, int NV, bool FILL>
static int32_t launch_among_range_t(const AmongRangeLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    static const char* const names[2][2][2] = {
        {{"k_adc_among_range_u8<count>", "k_adc_among_range_u8<fill>"},
         {"k_adc_among_range_residual_u8<count>", "k_adc_among_range_residual_u8<fill>"}},
        {{"k_adc_ip_among_range_u8<count>", "k_adc_ip_among_range_u8<fill>"},
         {"k_adc_ip_among_range_residual_u8<count>", "k_adc_ip_among_range_residual_u8<fill>"}}};
    auto kern = k_adc_among_range_u8<IP, RESIDUAL, NV, FILL>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)kAmongRangeStaticLds));
    hipLaunchKernelGGL(kern, dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n, a.c_rs, lut, a.extra, a.M, a.K, a.thr, a.lims, a.ids,
                       a.n_ids, a.row_list, a.n_lists, a.bias, a.b_rs, a.part, a.hits, a.bm_words, a.capacity, a.out_v, a.out_i,
                       a.err);
    note_kernel(names[IP][RESIDUAL][FILL]);
    return PQHIP_OK;
}

// a.bias != null: the residual producer
static int32_t launch_among_range_u8(bool ip, int nvb, bool fill, const AmongRangeLaunch& a, const void* codes, const float* lut,
                                     size_t lds)
{
    const int32_t status = dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_int<0, 1>(a.bias != nullptr, [&](auto res_c) {
            return dispatch_int<0, 1>(fill, [&](auto fill_c) {
                return dispatch_int<4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
                    return launch_among_range_t<decltype(ip_c)::value != 0, decltype(res_c)::value != 0, decltype(nv_c)::value,
                                                decltype(fill_c)::value != 0>(a, (const uint8_t*)codes, lut, lds);
                });
            });
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    return PQHIP_OK;
}

// Workgroups per query: the rule of pqhip_adc_among_f32_dev -- from the mean number of ids per query, at least 4,096
// places per workgroup and no more than the CUs the queries of a launch leave each other.  The estimate only sets the
// grid: slices are cut from the clamped range on the device and no result depends on G.
static int64_t among_range_wgs_per_query(int64_t mean_ids, int64_t nq, int n_cus)
{
    const int64_t by_rows = (mean_ids + 4095) / 4096;
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min(by_rows, by_cus));
}

// Both calls.  Checks in the order of adc_among (pqhip_adc_among.hip): EINVAL for what no shape excuses, ENODEV,
// EUNSUPPORTED, nq == 0, null pointers and the pairing of the residual inputs, ESHAPE; then the empty path, G, the
// chunking and count -> scan -> fill per chunk of queries.  A chunk keeps its partial counts and hit bitmaps within the
// scratch bound of the list searches and its counts within kAmongRangeScanMax.  The bitmap of a query has the words of
// `span` places: n_ids for a shared list (every trip has its words), else min(n_ids, 4 x the mean range + 1,024) -- the
// host cannot see the ranges, a longer range is legal, and its trips beyond the bitmap are looked at twice --, either
// cut to kAmongRangeSpanMax, so that one query's bitmap stays inside the scratch bound whatever n_ids.  The G
// workgroups of a query with at most `span` places use at most span / 64 + 32 G words between them (each rounds its slice
// up to whole trips of 16 words: below 2 trips of excess per workgroup).  d_extra: the scales (ip) or the row terms.
static int32_t adc_among_range(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                               int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids,
                               int64_t n_ids, const int64_t* d_row_list, int64_t n_lists, const float* d_bias, int64_t b_rs,
                               const float* d_extra, const float* d_thr, int64_t* d_out_lims, float* d_val, int64_t* d_idx,
                               int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n < 0 || n_ids < 0 || n_lists < 0 || capacity < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1) return PQHIP_EUNSUPPORTED;
    const size_t table = (size_t)cb->M * cb->K * sizeof(float);
    const int nvb = lists_nv_bucket(((int)cb->M + 3) / 4);
    if (nvb == 0 || table + kAmongRangeStaticLds > 160 * 1024) return PQHIP_EUNSUPPORTED;   // the table must fit LDS
    if (n > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;                                // the scope of the top-k call
    if (nq == 0) return PQHIP_OK;
    const bool residual = d_row_list != nullptr;
    if (!d_out_lims || !d_thr || (capacity > 0 && (!d_val || !d_idx)) || (n_ids > 0 && !d_ids) ||
        (n > 0 && n_ids > 0 && (!d_tables || !d_codes)))
        return PQHIP_EINVAL;
    if ((d_row_list != nullptr) != (d_bias != nullptr) || (residual && !ip && !d_extra)) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < cb->M) || (residual && b_rs < n_lists)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_ids == 0) {                                     // nothing can be named: no row, or no id to flag
        HIPCHK(hipMemsetAsync(d_out_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_out_lims, 0, sizeof(int64_t), st));     // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const int64_t mean = d_lims ? n_ids / nq : n_ids;
    const int64_t forced = cb->ctx->opt.adc_among_range_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : among_range_wgs_per_query(mean, std::min<int64_t>(nq, 65535), cb->ctx->devs[slot]->n_cus);
    const size_t part_q = (size_t)G * sizeof(int64_t);
    const int64_t span = std::min<int64_t>(d_lims ? std::min<int64_t>(n_ids, 4 * mean + 1024) : n_ids, kAmongRangeSpanMax);
    const int64_t bm_words = span / 64 + 32 * G + kRangeWaves;
    const size_t bm_q = (size_t)bm_words * sizeof(unsigned long long);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (part_q + bm_q)),
                                                                  kAmongRangeScanMax / G}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (part_q + bm_q)));
    int64_t* part = (int64_t*)lease.ptr();                          // [chunk][G], then the bitmaps: 8-byte items all
    unsigned long long* hits = (unsigned long long*)(part + (size_t)chunk * G);
    const int M = (int)cb->M, K = (int)cb->K;
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        const AmongRangeLaunch a{n, c_rs, (unsigned)G, nqc, M, K, (ip || residual) ? d_extra : nullptr, d_thr + q,
                                 d_lims ? d_lims + q : nullptr, d_ids, n_ids, d_row_list, n_lists,
                                 residual ? d_bias + q * b_rs : nullptr, residual ? b_rs : 0, part, hits, bm_words, capacity, d_val,
                                 d_idx, ef.flag, st};
        const float* lut = d_tables + q * (int64_t)M * K;
        PQCHK(launch_among_range_u8(ip, nvb, false, a, d_codes, lut, table));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, G, (int64_t)nqc, d_out_lims + q);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) PQCHK(launch_among_range_u8(ip, nvb, true, a, d_codes, lut, table));   // capacity == 0: a pure count call
    }
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_adc_among_range_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                      int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids,
                                      int64_t n_ids, const int64_t* d_row_list, int64_t n_lists, const float* d_list_bias,
                                      int64_t b_rs, const float* d_row_terms, const float* d_thr, int64_t* d_out_lims, float* d_val,
                                      int64_t* d_idx, int64_t capacity, void* stream)
{
    return adc_among_range(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_lims, d_ids, n_ids, d_row_list, n_lists,
                           d_list_bias, b_rs, d_row_terms, d_thr, d_out_lims, d_val, d_idx, capacity, stream);
}

int32_t pqhip_adc_ip_among_range_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                         int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids,
                                         int64_t n_ids, const int64_t* d_row_list, int64_t n_lists, const float* d_list_bias,
                                         int64_t b_rs, const float* d_scales, const float* d_thr, int64_t* d_out_lims, float* d_val,
                                         int64_t* d_idx, int64_t capacity, void* stream)
{
    return adc_among_range(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_lims, d_ids, n_ids, d_row_list, n_lists,
                           d_list_bias, b_rs, d_scales, d_thr, d_out_lims, d_val, d_idx, capacity, stream);
}

}  // extern "C"
