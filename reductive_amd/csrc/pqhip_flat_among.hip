// pqhip_flat_among.hip -- exact search among given rows (include/pqhip.h: pqhip_flat_among_f32_dev,
// pqhip_flat_range_among_f32_dev): the two entry points, their policy (checks, workgroups per query, chunks, scratch, the
// producer -> merge resp. count / scan / fill sequence) and the instantiations of kernels_flat_among.hip.h.  The list
// length, the LDS budget, the scratch bound of a chunk of queries and the merge are the list searches'
// (adc_search_launch.h); the scan is the ADC range searches' k_adc_range_scan.  There is no plan kernel: a workgroup
// clamps its query's two lims words itself.  A unit of its own so that the build compiles its producers beside the other
// searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_among.hip.h"

using namespace pqhip;

namespace pqh {

constexpr int64_t kFlatAmongScanMax = 1 << 20;   // partial counts of one chunk of queries: what one scan launch sums

struct FlatAmongLaunch {
    const float* q;
    int64_t q_rs;
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const int64_t *lims, *ids;
    int64_t n_ids;
    unsigned G, nq;          // grid (G, nq)
    int* err;
    hipStream_t st;
};

// Workgroups per query, from what the host knows without a synchronisation: the mean number of ids per query (n_ids with
// a shared list) and the row bytes, by the rule of flat_lists_wgs_per_query with the mean in the place of the expected
// probed rows --
//   one workgroup per 256 KB of named rows, no more than one per 256 places (16 waves x one tile: fewer leave waves idle)
//   and no more than the CUs the queries of a launch leave each other (one 1,024-thread workgroup per CU).
// The 256 KB are the list search's constant, taken over BEFORE anything was measured here; tools/flat_among_time.py
// records what it gives.  The estimate only sets the grid: slices are cut from the clamped range on the device and the
// result does not depend on G.
static int64_t flat_among_wgs_per_query(int64_t mean_ids, int64_t nq, int64_t row_bytes, int n_cus)
{
    const int64_t by_bytes = (int64_t)(((double)mean_ids * (double)row_bytes + 262143.0) / 262144.0);
    const int64_t by_tiles = (mean_ids + kSearchWaves * kFlatTile - 1) / (kSearchWaves * kFlatTile);
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min({by_bytes, by_tiles, by_cus}));
}

template <typename T, bool IP, int L>
static int32_t launch_flat_among_t(const FlatAmongLaunch& a, int k, unsigned* part_k, uint64_t* part_i, size_t lds)
{
    auto kern = k_flat_among<T, IP, L>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.G, a.nq), dim3(1024), lds, a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d, a.x_rs, k, a.lims, a.ids,
                       a.n_ids, part_k, part_i, a.err);
    return PQHIP_OK;
}

static int32_t launch_flat_among(bool f16, bool ip, int L, const FlatAmongLaunch& a, int k, unsigned* part_k, uint64_t* part_i,
                                 size_t lds)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            constexpr bool IP = decltype(ip_c)::value != 0;
            return dispatch_list_regs(L, [&](auto l_c) {
                return launch_flat_among_t<T, IP, decltype(l_c)::value>(a, k, part_k, part_i, lds);
            });
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(ip ? "k_flat_ip_among" : "k_flat_among");
    return PQHIP_OK;
}

struct FlatRangeAmongOut {
    const float* thr;
    int64_t* part;
    uint16_t* hits;
    int64_t bm_tiles;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
};

template <typename T, bool IP>
static int32_t launch_flat_range_among_t(const FlatAmongLaunch& a, const FlatRangeAmongOut& o, int fill)
{
    auto kern = k_flat_range_among<T, IP>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.G, a.nq), dim3(1024), (size_t)a.d * sizeof(float), a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d,
                       a.x_rs, o.thr, a.lims, a.ids, a.n_ids, fill, o.part, o.hits, o.bm_tiles, o.capacity, o.out_v, o.out_i, a.err);
    return PQHIP_OK;
}

static int32_t launch_flat_range_among(bool f16, bool ip, const FlatAmongLaunch& a, const FlatRangeAmongOut& o, int fill)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            return launch_flat_range_among_t<T, decltype(ip_c)::value != 0>(a, o, fill);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(ip ? "k_flat_ip_range_among" : "k_flat_range_among");
    return PQHIP_OK;
}

// the checks both calls make, in the precedence EINVAL, ENODEV, EUNSUPPORTED, then -- for n_queries > 0 -- the null
// pointers; `extra_einval` / `extra_unsupported` / `null_out` are what the call adds
#define FLAT_AMONG_HEAD_CHECKS(extra_einval, extra_unsupported, null_out)                                                \
    if (!cb || nq < 0 || n_rows < 0 || n_ids < 0 || d < 1 || (metric != 0 && metric != 1) || (extra_einval))             \
        return PQHIP_EINVAL;                                                                                             \
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;                                                    \
    if ((vec_bytes != 2 && vec_bytes != 4) || d > kFlatMaxD || n_rows > (int64_t)0xfffffffell || (extra_unsupported))    \
        return PQHIP_EUNSUPPORTED;                                                                                       \
    if (nq == 0) return PQHIP_OK;                                                                                        \
    if ((null_out) || !d_q || (n_ids > 0 && !d_ids) || (n_rows > 0 && !d_x)) return PQHIP_EINVAL

}  // namespace pqh

using namespace pqh;

extern "C" {

// Checks, then the padding-only path (no id: nothing can be named or flagged), G, the chunking and the producer -> merge
// loop of the ADC among call.  n_rows == 0 with ids takes the ordinary path: every id other than -1 fails the range
// check, raises the flag and forms no address, and the merge writes the padding.
int32_t pqhip_flat_among_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                 int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const int64_t* d_lims,
                                 const int64_t* d_ids, int64_t n_ids, int32_t metric, int32_t k, float* d_val, int64_t v_rs,
                                 int64_t* d_idx, int64_t i_rs, void* stream)
{
    FLAT_AMONG_HEAD_CHECKS(k < 1, k > kSearchMaxK, !d_val || !d_idx);
    if (q_rs < d || (n_rows > 0 && x_rs < d) || v_rs < k || i_rs < k) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const bool ip = metric != 0;
    const int L = search_list_regs(k);
    if (n_ids == 0) return adc_search_merge(ip, L, nq, 0, k, nullptr, nullptr, d_val, v_rs, d_idx, i_rs, st);
    ErrFlag ef(cb, slot, st);
    const int64_t forced = cb->ctx->opt.flat_among_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : flat_among_wgs_per_query(d_lims ? n_ids / nq : n_ids, std::min<int64_t>(nq, 65535), d * vec_bytes,
                                                            cb->ctx->devs[slot]->n_cus);
    // the partial lists of one chunk of queries within 512 MB of scratch, as for the list searches
    const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / lists_q)}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * lists_q));
    uint64_t* part_i = (uint64_t*)lease.ptr();                                         // [chunk][G][64 L], then the keys
    unsigned* part_k = (unsigned*)(part_i + (size_t)chunk * G * 64 * L);
    const size_t lds = search_lds((size_t)d * sizeof(float), 1, L);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        const FlatAmongLaunch a{d_q + q * q_rs, q_rs, d_x, n_rows, (int)d, x_rs, d_lims ? d_lims + q : nullptr, d_ids, n_ids,
                                (unsigned)G, nqc, ef.flag, st};
        PQCHK(launch_flat_among(vec_bytes == 2, ip, L, a, k, part_k, part_i, lds));
        PQCHK(adc_search_merge(ip, L, nqc, (int)G, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
    }
    return PQHIP_OK;
}

// Checks, then count / scan / fill over a (G, queries) grid per chunk of queries, as pqhip_flat_range_lists_f32_dev
// without its plan.  A chunk keeps the partial counts and the hit bitmaps within the scratch bound of the list searches and
// the counts within kFlatAmongScanMax.  The bitmap of a query has a slot for every tile of `span` places: n_ids for a
// shared list (every tile has its slot), else min(n_ids, 4 x the mean range + 1,024) -- the host cannot see the ranges, a
// longer range is legal, and its tiles beyond the bitmap are looked at twice.  The 16 G units of a query with at most
// `span` places hold at most span / 16 + 65 G tiles between them.
int32_t pqhip_flat_range_among_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                       int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const int64_t* d_lims,
                                       const int64_t* d_ids, int64_t n_ids, int32_t metric, const float* d_thr, int64_t* d_out_lims,
                                       float* d_val, int64_t* d_idx, int64_t capacity, void* stream)
{
    FLAT_AMONG_HEAD_CHECKS(capacity < 0, false, !d_out_lims || !d_thr || (capacity > 0 && (!d_val || !d_idx)));
    if (q_rs < d || (n_rows > 0 && x_rs < d)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n_ids == 0) {
        HIPCHK(hipMemsetAsync(d_out_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_out_lims, 0, sizeof(int64_t), st));     // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const int64_t mean = d_lims ? n_ids / nq : n_ids;
    const int64_t forced = cb->ctx->opt.flat_range_among_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : flat_among_wgs_per_query(mean, std::min<int64_t>(nq, 65535), d * vec_bytes,
                                                            cb->ctx->devs[slot]->n_cus);
    const int64_t units = G * kRangeWaves;
    const size_t part_q = (size_t)units * sizeof(int64_t);
    const int64_t span = d_lims ? std::min<int64_t>(n_ids, 4 * mean + 1024) : n_ids;
    const int64_t bm_tiles = round_up(span / kFlatTile + 65 * G + 1, 4);
    const size_t bm_q = (size_t)bm_tiles * sizeof(uint16_t);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (part_q + bm_q)),
                                                                  kFlatAmongScanMax / units}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (part_q + bm_q)));
    int64_t* part = (int64_t*)lease.ptr();                          // [chunk][16 G], then the bitmaps
    uint16_t* hits = (uint16_t*)(part + (size_t)chunk * units);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        const FlatAmongLaunch a{d_q + q * q_rs, q_rs, d_x, n_rows, (int)d, x_rs, d_lims ? d_lims + q : nullptr, d_ids, n_ids,
                                (unsigned)G, nqc, ef.flag, st};
        const FlatRangeAmongOut o{d_thr + q, part, hits, bm_tiles, capacity, d_val, d_idx};
        PQCHK(launch_flat_range_among(vec_bytes == 2, metric != 0, a, o, 0));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, (int64_t)nqc, d_out_lims + q);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) PQCHK(launch_flat_range_among(vec_bytes == 2, metric != 0, a, o, 1));   // capacity == 0: a pure count call
    }
    return PQHIP_OK;
}

}  // extern "C"
