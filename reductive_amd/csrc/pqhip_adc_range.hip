// pqhip_adc_range.hip -- ADC range search (include/pqhip.h: pqhip_adc_*range*_f32_dev): every row within a radius resp.
// at or above a similarity, exhaustive and over probed lists, as CSR with a capacity protocol.  This unit holds the six
// entry points, their policy (checks, queries per pass, row ranges, scratch, the count / scan / fill sequence) and the
// instantiations of kernels_adc_range.hip.h.  From pqhip_adc.hip it takes the plan of the list searches and the
// choices a range call shares with them (adc_search_launch.h); nothing in pqhip_adc.hip refers to this unit.
#include "adc_search_launch.h"

#define PQHIP_ADC_TEMPLATES_ONLY   // kernels_adc.hip.h: its non-template kernels belong to pqhip_adc.hip
#include "kernels_adc_range.hip.h"

using namespace pqhip;

namespace pqh {

// what both passes of a call share: ONE decomposition (grid, row ranges) serves count and fill
struct RangeLaunch {
    int64_t n, c_rs, rows_per_wg;
    unsigned grid;
    int M, K;
    const uint32_t* allow;
    const float* scales;
    const float* thr;
    int64_t* part;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
    int* err;
    hipStream_t st;
};

template <bool IP, int NV, int NQ>
int32_t launch_range(const RangeLaunch& a, const uint8_t* codes, const float* lut, size_t lds, int fill)
{
    HIPCHK(hipFuncSetAttribute((const void*)k_adc_range_u8<IP, NV, NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((k_adc_range_u8<IP, NV, NQ>), dim3(a.grid), dim3(1024), lds, a.st, codes, a.n, a.c_rs, a.allow, lut,
                       a.scales, a.thr, a.M, a.K, a.rows_per_wg, fill, a.part, a.capacity, a.out_v, a.out_i, a.err);
    if (IP) note_kernel(NQ == 8 ? "k_adc_ip_range_u8_mq<8 queries>" : NQ == 4 ? "k_adc_ip_range_u8_mq<4 queries>" : "k_adc_ip_range_u8");
    else note_kernel(NQ == 8 ? "k_adc_range_u8_mq<8 queries>" : NQ == 4 ? "k_adc_range_u8_mq<4 queries>" : "k_adc_range_u8");
    return PQHIP_OK;
}

int32_t launch_range_u8(bool ip, int nq_pass, int nvb, const RangeLaunch& a, const uint8_t* codes, const float* lut, size_t lds, int fill)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_queries_per_pass(nq_pass, [&](auto nq_c) {
            return dispatch_int<1, 2, 4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
                return launch_range<decltype(ip_c)::value != 0, decltype(nv_c)::value, decltype(nq_c)::value>(a, codes, lut, lds, fill);
            });
        });
    });
}

constexpr int64_t kRangeScanMax = 1 << 20;   // partial counts of one pass / chunk of queries: what one scan launch sums

// the prefix over part [nq][units] and lims[q0 .. q0 + nq] (lims points at lims[q0], which holds the total so far)
int32_t launch_range_scan(int64_t* part, int64_t units, int64_t nq, int64_t* lims, hipStream_t st)
{
    hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, nq, lims);
    HIPCHK(hipGetLastError());
    note_kernel("k_adc_range_scan");
    return PQHIP_OK;
}

// The checks every range call makes on its outputs, in the precedence of adc_search (EINVAL, ENODEV, EUNSUPPORTED, then
// -- for n_queries > 0 -- the null pointers and ESHAPE); `unsupported` is the call's own scope test.
#define RANGE_HEAD_CHECKS(extra_einval, unsupported)                                              \
    if (!cb || nq < 0 || n < 0 || capacity < 0 || (extra_einval)) return PQHIP_EINVAL;            \
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;                             \
    if (unsupported) return PQHIP_EUNSUPPORTED;                                                   \
    if (nq == 0) return PQHIP_OK;                                                                 \
    if (!d_lims || !d_thr || (capacity > 0 && (!d_val || !d_idx))) return PQHIP_EINVAL

// Exhaustive range search.  Queries per pass: 8, 4 or 1 table images in the 160 KB of LDS (option "adc_single_query"
// keeps one), a host choice on which no result depends.  One 1,024-thread workgroup per CU by default (option
// "adc_range_wgs" forces the number, up to the 8,192 at which a pass of 8 queries has kRangeScanMax counts), a contiguous
// row range each, cut into 16 wave sub-ranges by the kernel.
template <bool IP>
int32_t adc_range(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes, int32_t code_bytes,
                  int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales, const float* d_thr, int64_t* d_lims,
                  float* d_val, int64_t* d_idx, int64_t capacity, void* stream)
{
    RANGE_HEAD_CHECKS(false, code_bytes != 1 || search_nv_bucket(((int)cb->M + 3) / 4) == 0 ||
                                 (size_t)cb->M * cb->K * sizeof(float) > 160 * 1024);
    if (n > 0 && (!d_tables || !d_codes)) return PQHIP_EINVAL;
    if (n > 0 && c_rs < cb->M) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first pass starts from it
    ErrFlag ef(cb, slot, st);
    const int M = (int)cb->M, K = (int)cb->K;
    const size_t table = (size_t)M * K * sizeof(float);
    const int nvb = search_nv_bucket((M + 3) / 4);
    const bool mq_on = cb->ctx->opt.adc_single_query.load(std::memory_order_relaxed) == 0;
    int nqp_first = 1;
    if (mq_on) {
        for (int c : {8, 4}) {
            if (table * c <= 160 * 1024 && nq >= c) { nqp_first = c; break; }
        }
    }
    const int64_t forced = cb->ctx->opt.adc_range_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, kRangeScanMax / (8 * kRangeWaves)) : cb->ctx->devs[slot]->n_cus;
    int64_t rows_per_wg = round_up((n + wgs - 1) / wgs, 1024);
    if (forced <= 0) rows_per_wg = std::max<int64_t>(rows_per_wg, 4096);
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    if (grid > 0x7fffffff) return PQHIP_EUNSUPPORTED;
    const int64_t units = grid * kRangeWaves;
    ScratchLease part(cb, slot, st);
    PQCHK(part.acquire((size_t)nqp_first * units * sizeof(int64_t)));
    RangeLaunch a{n, c_rs, rows_per_wg, (unsigned)grid, M, K, d_allow, d_scales, d_thr, (int64_t*)part.ptr(), capacity, d_val, d_idx,
                  ef.flag, st};
    int64_t q = 0;
    for (int nqp : {8, 4, 1}) {
        if (nqp > nqp_first) continue;
        if (nqp == 4 && !(mq_on && table * 4 <= 160 * 1024)) continue;
        for (; q + nqp <= nq; q += nqp) {
            const float* lut = d_tables + q * (int64_t)M * K;
            a.thr = d_thr + q;
            PQCHK((launch_range_u8(IP, nqp, nvb, a, (const uint8_t*)d_codes, lut, table * nqp, 0)));
            HIPCHK(hipGetLastError());
            PQCHK(launch_range_scan(a.part, units, nqp, d_lims + q, st));
            if (capacity > 0) {     // capacity == 0: a pure count call
                PQCHK((launch_range_u8(IP, nqp, nvb, a, (const uint8_t*)d_codes, lut, table * nqp, 1)));
                HIPCHK(hipGetLastError());
            }
        }
    }
    return PQHIP_OK;
}

struct RangeListsLaunch {
    int64_t n, c_rs;
    unsigned G, nq;
    int M, K, n_probe;
    const uint32_t* allow;
    const float* bias;
    int64_t b_rs;
    const float* extra;
    const float* thr;
    const int64_t *seg_begin, *seg_cum;
    int64_t* part;
    int64_t capacity;
    float* out_v;
    int64_t* out_i;
    int* err;
    hipStream_t st;
};

template <int POL, int NV>
int32_t launch_range_lists(const RangeListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds, int fill)
{
    HIPCHK(hipFuncSetAttribute((const void*)k_adc_range_lists_u8<POL, NV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((k_adc_range_lists_u8<POL, NV>), dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n, a.c_rs, a.allow, lut,
                       a.bias, a.b_rs, a.extra, a.thr, a.M, a.K, a.seg_begin, a.seg_cum, a.n_probe, fill, a.part, a.capacity,
                       a.out_v, a.out_i, a.err);
    note_kernel(POL == kRangeL2 ? "k_adc_range_lists_u8" : POL == kRangeIP ? "k_adc_ip_range_lists_u8"
                : POL == kRangeResL2 ? "k_adc_range_lists_residual_u8" : "k_adc_ip_range_lists_residual_u8");
    return PQHIP_OK;
}

int32_t launch_range_lists_p(int pol, int nvb, const RangeListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds, int fill)
{
    return dispatch_int<kRangeL2, kRangeIP, kRangeResL2, kRangeResIP>(pol, [&](auto pol_c) {
        return dispatch_int<4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
            return launch_range_lists<decltype(pol_c)::value, decltype(nv_c)::value>(a, codes, lut, lds, fill);
        });
    });
}

// All four list range calls: the checks of adc_search_lists, its plan kernel (unchanged: the only reader of the offsets
// and probes), then count / scan / fill over a (G, queries) grid per chunk of queries.  A chunk keeps the plan and the
// partial counts within the scratch bound of the list searches and within kRangeScanMax counts.
int32_t adc_range_lists(int pol, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                        int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const int64_t* d_list_off,
                        int64_t n_lists, const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_bias, int64_t b_rs,
                        const float* d_extra, const float* d_thr, int64_t* d_lims, float* d_val, int64_t* d_idx, int64_t capacity,
                        void* stream)
{
    const bool res = pol == kRangeResL2 || pol == kRangeResIP;
    const size_t plan_q = ((size_t)std::max(n_probe, 1) * 2 + 1) * sizeof(int64_t);
    RANGE_HEAD_CHECKS(n_lists < 0 || n_probe < 1,
                      code_bytes != 1 || lists_nv_bucket(((int)cb->M + 3) / 4) == 0 ||
                          (size_t)cb->M * cb->K * sizeof(float) > 160 * 1024 || n > (int64_t)0xfffffffell ||
                          plan_q > kListsScratchBytes / 2);
    if (!d_list_off || !d_probes || (n > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if (res && (!d_bias || (pol == kRangeResL2 && !d_extra))) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < cb->M) || p_rs < n_probe) return PQHIP_ESHAPE;
    if (res && b_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_lists == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const int M = (int)cb->M, K = (int)cb->K;
    const size_t table = (size_t)M * K * sizeof(float);
    const int nvb = lists_nv_bucket((M + 3) / 4);
    const int64_t forced = cb->ctx->opt.adc_range_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : lists_wgs_per_query(n, n_lists, n_probe, std::min<int64_t>(nq, 65535), cb->ctx->devs[slot]->n_cus);
    const int64_t units = G * kRangeWaves;
    const size_t part_q = (size_t)units * sizeof(int64_t);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (plan_q + part_q)),
                                                                  kRangeScanMax / units}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (plan_q + part_q)));
    // part [chunk][16 G], seg_begin [chunk][n_probe], seg_cum [chunk][n_probe + 1]: 8-byte items all
    int64_t* part = (int64_t*)lease.ptr();
    int64_t* seg_begin = part + (size_t)chunk * units;
    int64_t* seg_cum = seg_begin + (size_t)chunk * n_probe;
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        PQCHK(launch_lists_plan(d_list_off, n_lists, d_probes + q * p_rs, (int)n_probe, p_rs, n, seg_begin, seg_cum, nqc, ef.flag, st));
        RangeListsLaunch a{n, c_rs, (unsigned)G, nqc, M, K, (int)n_probe, d_allow, res ? d_bias + q * b_rs : nullptr, res ? b_rs : 0,
                           d_extra, d_thr + q, seg_begin, seg_cum, part, capacity, d_val, d_idx, ef.flag, st};
        const float* lut = d_tables + q * (int64_t)M * K;
        PQCHK(launch_range_lists_p(pol, nvb, a, (const uint8_t*)d_codes, lut, table, 0));
        HIPCHK(hipGetLastError());
        PQCHK(launch_range_scan(part, units, nqc, d_lims + q, st));
        if (capacity > 0) {         // capacity == 0: a pure count call
            PQCHK(launch_range_lists_p(pol, nvb, a, (const uint8_t*)d_codes, lut, table, 1));
            HIPCHK(hipGetLastError());
        }
    }
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_adc_range_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_thr,
                                int64_t* d_lims, float* d_val, int64_t* d_idx, int64_t capacity, void* stream)
{
    return adc_range<false>(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, nullptr, d_thr, d_lims, d_val, d_idx,
                            capacity, stream);
}

int32_t pqhip_adc_ip_range_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                   int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales,
                                   const float* d_thr, int64_t* d_lims, float* d_val, int64_t* d_idx, int64_t capacity,
                                   void* stream)
{
    return adc_range<true>(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, d_scales, d_thr, d_lims, d_val, d_idx,
                           capacity, stream);
}

int32_t pqhip_adc_range_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                      int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                      const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                      int64_t p_rs, const float* d_thr, int64_t* d_lims, float* d_val, int64_t* d_idx,
                                      int64_t capacity, void* stream)
{
    return adc_range_lists(kRangeL2, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, d_list_off, n_lists, d_probes,
                           n_probe, p_rs, nullptr, 0, nullptr, d_thr, d_lims, d_val, d_idx, capacity, stream);
}

int32_t pqhip_adc_ip_range_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                         int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                         const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                         int64_t p_rs, const float* d_scales, const float* d_thr, int64_t* d_lims, float* d_val,
                                         int64_t* d_idx, int64_t capacity, void* stream)
{
    return adc_range_lists(kRangeIP, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, d_list_off, n_lists, d_probes,
                           n_probe, p_rs, nullptr, 0, d_scales, d_thr, d_lims, d_val, d_idx, capacity, stream);
}

int32_t pqhip_adc_range_lists_residual_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                               const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                               const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                               const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_probe_bias,
                                               int64_t b_rs, const float* d_row_terms, const float* d_thr, int64_t* d_lims,
                                               float* d_val, int64_t* d_idx, int64_t capacity, void* stream)
{
    return adc_range_lists(kRangeResL2, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, d_list_off, n_lists, d_probes,
                           n_probe, p_rs, d_probe_bias, b_rs, d_row_terms, d_thr, d_lims, d_val, d_idx, capacity, stream);
}

int32_t pqhip_adc_ip_range_lists_residual_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                  const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                  const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                                  const int64_t* d_probes, int32_t n_probe, int64_t p_rs,
                                                  const float* d_probe_bias, int64_t b_rs, const float* d_scales,
                                                  const float* d_thr, int64_t* d_lims, float* d_val, int64_t* d_idx,
                                                  int64_t capacity, void* stream)
{
    return adc_range_lists(kRangeResIP, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, d_list_off, n_lists, d_probes,
                           n_probe, p_rs, d_probe_bias, b_rs, d_scales, d_thr, d_lims, d_val, d_idx, capacity, stream);
}

}  // extern "C"
