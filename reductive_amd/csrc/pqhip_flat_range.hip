// pqhip_flat_range.hip -- exact range search over resident vectors (include/pqhip.h: pqhip_flat_range_f32_dev,
// pqhip_flat_range_lists_f32_dev): the two entry points, their policy (checks, queries per pass, row ranges resp.
// workgroups per query, chunks, scratch, the count / scan / fill sequence) and the instantiations of
// kernels_flat_range.hip.h.  The plan kernel and the scratch bound of a chunk of queries are the list searches'
// (adc_search_launch.h); the scan is the ADC range searches' k_adc_range_scan.  A unit of its own so that the build compiles
// its producers beside the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_range.hip.h"

using namespace pqhip;

namespace pqh {

constexpr int64_t kFlatRangeScanMax = 1 << 20;   // partial counts of one pass / chunk of queries: what one scan launch sums
constexpr int kFlatRangeQueries = 4;             // queries of a pass while their images fit the LDS

// the prefix over part [nq][units] and lims[q0 .. q0 + nq] (lims points at lims[q0], which holds the total so far)
static int32_t launch_flat_range_scan(int64_t* part, int64_t units, int64_t nq, int64_t* lims, hipStream_t st)
{
    hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, nq, lims);
    HIPCHK(hipGetLastError());
    note_kernel("k_adc_range_scan");
    return PQHIP_OK;
}

// what both passes of a call share: ONE decomposition (grid, row ranges) serves count and fill
struct FlatRangeLaunch {
    const float* q;
    int64_t q_rs;
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    const float* thr;
    int64_t rows_per_wg;
    unsigned grid;
    int64_t* part;
    uint16_t* hits;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
    hipStream_t st;
};

// Queries per pass: there are no queues and no k, so the LDS holds the query images alone -- the flat search's rule, 4
// queries while d <= 9,216 (147 KB of the 160), else one; the last nq mod 4 queries one per pass.  64 partials and 16 row
// elements per lane stay within the 128 VGPRs of a 1,024-thread workgroup.
static int flat_range_queries_per_pass(int64_t nq_left, int d)
{
    return nq_left >= kFlatRangeQueries && d <= 9216 ? kFlatRangeQueries : 1;
}

template <typename T, bool IP, int NQ>
static int32_t launch_flat_range_t(const FlatRangeLaunch& a, int fill)
{
    auto kern = k_flat_range<T, IP, NQ>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), (size_t)NQ * a.d * sizeof(float), a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d,
                       a.x_rs, a.allow, a.thr, a.rows_per_wg, fill, a.part, a.hits, a.capacity, a.out_v, a.out_i);
    return PQHIP_OK;
}

static int32_t launch_flat_range(bool f16, bool ip, int nqp, const FlatRangeLaunch& a, int fill)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            return dispatch_int<kFlatRangeQueries, 1>(nqp, [&](auto nq_c) {
                using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
                return launch_flat_range_t<T, decltype(ip_c)::value != 0, decltype(nq_c)::value>(a, fill);
            });
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    if (nqp == kFlatRangeQueries) note_kernel(ip ? "k_flat_ip_range<4 queries>" : "k_flat_range<4 queries>");
    else note_kernel(ip ? "k_flat_ip_range" : "k_flat_range");
    return PQHIP_OK;
}

struct FlatRangeListsLaunch {
    const float* q;
    int64_t q_rs;
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    const float* thr;
    const int64_t *seg_begin, *seg_cum;
    int n_probe;
    unsigned G, nq;          // grid (G, nq)
    int64_t* part;
    uint16_t* hits;
    int64_t bm_tiles;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
    hipStream_t st;
};

template <typename T, bool IP>
static int32_t launch_flat_range_lists_t(const FlatRangeListsLaunch& a, int fill)
{
    auto kern = k_flat_range_lists<T, IP>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.G, a.nq), dim3(1024), (size_t)a.d * sizeof(float), a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d,
                       a.x_rs, a.allow, a.thr, a.seg_begin, a.seg_cum, a.n_probe, fill, a.part, a.hits, a.bm_tiles, a.capacity,
                       a.out_v, a.out_i);
    return PQHIP_OK;
}

static int32_t launch_flat_range_lists(bool f16, bool ip, const FlatRangeListsLaunch& a, int fill)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            return launch_flat_range_lists_t<T, decltype(ip_c)::value != 0>(a, fill);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(ip ? "k_flat_ip_range_lists" : "k_flat_range_lists");
    return PQHIP_OK;
}

// Workgroups per query of the list call, from the expected probed bytes: the rule of pqhip_flat_search_lists_f32_dev (one
// workgroup per 256 KB of probed rows, no more than one per 256 rows -- 16 waves x one tile -- and no more than the CUs
// the queries of a launch leave each other).  It only sets the grid: slices are cut from the actual T_q on the device.
static int64_t flat_range_wgs_per_query(int64_t n, int64_t n_lists, int64_t n_probe, int64_t nq, int64_t row_bytes, int n_cus)
{
    const double frac = (double)std::min<int64_t>(n_probe, n_lists) / (double)n_lists;
    const int64_t expected = (int64_t)((double)n * frac) + 1;
    const int64_t by_bytes = (int64_t)(((double)expected * (double)row_bytes + 262143.0) / 262144.0);
    const int64_t by_tiles = (expected + kRangeWaves * kFlatTile - 1) / (kRangeWaves * kFlatTile);
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min({by_bytes, by_tiles, by_cus}));
}

// the checks both calls make, in the precedence EINVAL, ENODEV, EUNSUPPORTED, then -- for n_queries > 0 -- the null
// pointers; `extra_einval` / `extra_unsupported` are the list call's own
#define FLAT_RANGE_HEAD_CHECKS(extra_einval, extra_unsupported)                                                          \
    if (!cb || nq < 0 || n_rows < 0 || capacity < 0 || d < 1 || (metric != 0 && metric != 1) || (extra_einval))          \
        return PQHIP_EINVAL;                                                                                             \
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;                                                    \
    if ((vec_bytes != 2 && vec_bytes != 4) || d > kFlatMaxD || (extra_unsupported)) return PQHIP_EUNSUPPORTED;           \
    if (nq == 0) return PQHIP_OK;                                                                                        \
    if (!d_lims || !d_thr || (capacity > 0 && (!d_val || !d_idx)) || !d_q || (n_rows > 0 && !d_x)) return PQHIP_EINVAL

}  // namespace pqh

using namespace pqh;

extern "C" {

// One 1,024-thread workgroup per CU by default (option "flat_range_wgs" forces the number, up to the 16,384 at which a
// pass of 4 queries has kFlatRangeScanMax counts), a contiguous row range each (a multiple of 1,024), cut into 16 wave
// sub-ranges by the kernel.  Scratch of a pass: the partial counts [queries][units] and the hit bitmap, 2 bytes per
// (query, tile of 16 rows).
int32_t pqhip_flat_range_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                 int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const uint32_t* d_allow, int32_t metric,
                                 const float* d_thr, int64_t* d_lims, float* d_val, int64_t* d_idx, int64_t capacity, void* stream)
{
    FLAT_RANGE_HEAD_CHECKS(false, false);
    if (q_rs < d || (n_rows > 0 && x_rs < d)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first pass starts from it
    const int64_t forced = cb->ctx->opt.flat_range_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, kFlatRangeScanMax / (kFlatRangeQueries * kRangeWaves))
                                   : cb->ctx->devs[slot]->n_cus;
    const int64_t rows_per_wg = round_up((n_rows + wgs - 1) / wgs, 1024);
    const int64_t grid = (n_rows + rows_per_wg - 1) / rows_per_wg;
    const int64_t units = grid * kRangeWaves;
    const int64_t tiles = (n_rows + kFlatTile - 1) / kFlatTile;
    const int nqp_first = flat_range_queries_per_pass(nq, (int)d);
    const size_t part_bytes = (size_t)nqp_first * units * sizeof(int64_t);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire(part_bytes + (size_t)nqp_first * tiles * sizeof(uint16_t)));
    int64_t* part = (int64_t*)lease.ptr();
    uint16_t* hits = (uint16_t*)((char*)lease.ptr() + part_bytes);
    FlatRangeLaunch a{nullptr, q_rs, d_x, n_rows, (int)d, x_rs, d_allow, nullptr, rows_per_wg, (unsigned)grid, part, hits, capacity,
                      d_val, d_idx, st};
    for (int64_t q = 0; q < nq;) {
        const int nqp = flat_range_queries_per_pass(nq - q, (int)d);
        a.q = d_q + q * q_rs;
        a.thr = d_thr + q;
        PQCHK(launch_flat_range(vec_bytes == 2, metric != 0, nqp, a, 0));
        PQCHK(launch_flat_range_scan(part, units, nqp, d_lims + q, st));
        if (capacity > 0) PQCHK(launch_flat_range(vec_bytes == 2, metric != 0, nqp, a, 1));   // capacity == 0: a pure count call
        q += nqp;
    }
    return PQHIP_OK;
}

// The checks of pqhip_flat_search_lists_f32_dev and of the ADC range calls, the plan kernel of the list searches
// (unchanged: the only reader of the offsets and probes), then count / scan / fill over a (G, queries) grid per chunk of
// queries.  A chunk keeps the plan, the partial counts and the hit bitmap within the scratch bound of the list searches
// and the counts within kFlatRangeScanMax.  The bitmap of a query has a slot for every tile of T_q <= n_rows places: the
// 16 G units of a query hold at most n_rows / 16 + 65 G tiles between them.
int32_t pqhip_flat_range_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                       int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const uint32_t* d_allow,
                                       const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                       int64_t p_rs, int32_t metric, const float* d_thr, int64_t* d_lims, float* d_val,
                                       int64_t* d_idx, int64_t capacity, void* stream)
{
    const size_t plan_q = ((size_t)std::max(n_probe, 1) * 2 + 1) * sizeof(int64_t);
    FLAT_RANGE_HEAD_CHECKS(n_lists < 0 || n_probe < 1, n_rows > (int64_t)0xfffffffell || plan_q > kListsScratchBytes / 2);
    if (!d_list_off || !d_probes) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d) || p_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0 || n_lists == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const int64_t forced = cb->ctx->opt.flat_range_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : flat_range_wgs_per_query(n_rows, n_lists, n_probe, std::min<int64_t>(nq, 65535), d * vec_bytes,
                                                            cb->ctx->devs[slot]->n_cus);
    const int64_t units = G * kRangeWaves;
    const size_t part_q = (size_t)units * sizeof(int64_t);
    const int64_t bm_tiles = round_up(n_rows / kFlatTile + 65 * G + 1, 4);
    const size_t bm_q = (size_t)bm_tiles * sizeof(uint16_t);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (plan_q + part_q + bm_q)),
                                                                  kFlatRangeScanMax / units}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (plan_q + part_q + bm_q)));
    // 8-byte items first: part [chunk][16 G], seg_begin [chunk][n_probe], seg_cum [chunk][n_probe + 1]; then the bitmap
    int64_t* part = (int64_t*)lease.ptr();
    int64_t* seg_begin = part + (size_t)chunk * units;
    int64_t* seg_cum = seg_begin + (size_t)chunk * n_probe;
    uint16_t* hits = (uint16_t*)(seg_cum + (size_t)chunk * ((size_t)n_probe + 1));
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        PQCHK(launch_lists_plan(d_list_off, n_lists, d_probes + q * p_rs, (int)n_probe, p_rs, n_rows, seg_begin, seg_cum, nqc, ef.flag, st));
        const FlatRangeListsLaunch a{d_q + q * q_rs, q_rs, d_x, n_rows, (int)d, x_rs, d_allow, d_thr + q, seg_begin, seg_cum,
                                     (int)n_probe, (unsigned)G, nqc, part, hits, bm_tiles, capacity, d_val, d_idx, st};
        PQCHK(launch_flat_range_lists(vec_bytes == 2, metric != 0, a, 0));
        PQCHK(launch_flat_range_scan(part, units, nqc, d_lims + q, st));
        if (capacity > 0) PQCHK(launch_flat_range_lists(vec_bytes == 2, metric != 0, a, 1));   // capacity == 0: a pure count call
    }
    return PQHIP_OK;
}

}  // extern "C"
