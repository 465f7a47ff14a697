// pqhip_adc_screen_lists_residual.hip -- conservative range screen over resident RESIDUAL u8 codes in probed lists
// (include/pqhip.h: pqhip_adc_screen_lists_residual_f32_dev): the entry point, its policy (checks, slots per group, chunks
// of queries, scratch, the reduce / prep / pairs / units / scatter / scan / count / scan / fill sequence) and the
// instantiations of kernels_adc_screen_lists_residual.hip.h.  Planning kernels, scans, options and the code dwords per row
// are those of pqhip_adc_screen_lists.hip.  A unit of its own so that the build compiles its kernels beside the other
// searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_adc_screen_lists_residual.hip.h"

using namespace pqhip;

namespace pqh {

constexpr size_t kAdcScreenResLds = 160 * 1024;
constexpr int64_t kAdcScreenResUnitRows = 16384;     // the list screen's unit
constexpr int64_t kAdcScreenResWgsMax = 65535;

struct AdcScreenResLaunch {
    const uint8_t* codes;
    int64_t n, c_rs;
    const uint32_t* allow;
    const float* xrow;         // the row terms (ip 0), the scales or null (ip 1)
    const float* bias;
    int64_t b_rs;
    const int* ext;            // [0] the largest scale (bits), [1] the least term (key)
    const int64_t* list_off;
    int64_t n_lists;
    const int64_t* probes;
    int n_probe;
    int64_t p_rs, nq;
    const unsigned *lcnt, *pair_off;
    const int64_t* unit_off;
    const unsigned* pairs;
    const uint8_t* imgq;
    int64_t pitch;
    const AdcScreenPrm* prm;
    int M, K;
    int64_t unit_rows;
    const int64_t* hoff;
    int64_t budget;
    uint32_t* hits;
    int64_t* cnt;
    int64_t capacity;
    int64_t* out_i;
    unsigned grid;
    int* err;
    hipStream_t st;
};

template <int NV, int NQ, bool IP>
static int32_t launch_adc_screen_res_t(const AdcScreenResLaunch& a)
{
    auto kern = k_adc_screen_lists_residual<NV, NQ, IP>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAdcScreenResLds));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), adc_screen_lists_residual_lds_bytes(a.M, a.K, NQ), a.st, a.codes, a.n, a.c_rs,
                       a.allow, a.xrow, a.bias, a.b_rs, a.ext, a.list_off, a.n_lists, a.lcnt, a.pair_off, a.unit_off, a.pairs, a.n_probe,
                       a.imgq, a.pitch, a.prm, a.M, a.K, a.unit_rows, a.hoff, a.budget, a.hits, (unsigned long long*)a.cnt, a.err);
    return PQHIP_OK;
}

static int32_t launch_adc_screen_res(int nvb, int slots, bool ip, const AdcScreenResLaunch& a)
{
    const int32_t status = dispatch_int<1, 2, 4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
        return dispatch_int<32, 16, 8, 4>(slots, [&](auto nq_c) {
            return ip ? launch_adc_screen_res_t<decltype(nv_c)::value, decltype(nq_c)::value, true>(a)
                      : launch_adc_screen_res_t<decltype(nv_c)::value, decltype(nq_c)::value, false>(a);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(slots == 32 ? "k_adc_screen_lists_residual<32 pairs>" : slots == 16 ? "k_adc_screen_lists_residual<16 pairs>"
                : slots == 8 ? "k_adc_screen_lists_residual<8 pairs>" : "k_adc_screen_lists_residual<4 pairs>");
    return PQHIP_OK;
}

// the most slots of a group whose image, parameters, biases, limits and pair records fit the LDS; 0 when 4 do not
static int adc_screen_res_slots(int M, int K)
{
    for (int c : {32, 16, 8, 4})
        if (adc_screen_lists_residual_lds_bytes(M, K, c) <= kAdcScreenResLds) return c;
    return 0;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

// Chunks, scratch and grid are those of pqhip_adc_screen_lists_f32_dev, under the same three options.  The head of the
// scratch holds the call-wide largest scale and least term: one reduction each in front of the passes.
int32_t pqhip_adc_screen_lists_residual_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                                int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                                int64_t p_rs, const float* d_probe_bias, int64_t b_rs, const float* d_row_terms,
                                                int32_t ip, const float* d_scales, const float* d_thr, int64_t* d_lims, int64_t* d_idx,
                                                int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n < 0 || capacity < 0 || n_lists < 0 || n_probe < 1 || (ip != 0 && ip != 1) || (!ip && d_scales) ||
        (ip && d_row_terms))
        return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || cb->M > kAdcScreenMaxM || n > (int64_t)0xfffffffell || n_probe > kFslMaxEntries) return PQHIP_EUNSUPPORTED;
    const int nvb = search_nv_bucket(((int)cb->M + 3) / 4);
    const int slots = adc_screen_res_slots((int)cb->M, (int)cb->K);
    if (nvb == 0 || slots == 0) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || (n > 0 && (!d_tables || !d_codes)) || !d_list_off || !d_probes || !d_probe_bias ||
        (!ip && !d_row_terms))
        return PQHIP_EINVAL;
    if ((n > 0 && c_rs < cb->M) || p_rs < n_probe || b_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_lists == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const Options& opt = cb->ctx->opt;
    const int M = (int)cb->M, K = (int)cb->K;
    const int64_t pitch = adc_screen_lists_pitch(M, K);
    const int64_t forced_rows = opt.adc_screen_lists_unit_rows.load(std::memory_order_relaxed);
    const int64_t unit_rows = forced_rows > 0 ? round_up(forced_rows, 64) : kAdcScreenResUnitRows;
    const int64_t forced_wgs = opt.adc_screen_lists_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = std::min<int64_t>(forced_wgs > 0 ? forced_wgs : (int64_t)cb->ctx->devs[slot]->n_cus, kAdcScreenResWgsMax);
    const size_t head_bytes = 256;                                  // the largest scale, the least term
    const size_t lists_bytes = (size_t)round_up((n_lists + 1) * 20, 256);
    const int64_t words_q = fsl_words_per_query(n, n_lists, n_probe);
    const size_t per_q = (size_t)pitch + sizeof(AdcScreenPrm) + 8 + (size_t)n_probe * 20 + (size_t)words_q * 4;
    const size_t room = kListsScratchBytes > lists_bytes + head_bytes + 4096 ? kListsScratchBytes - lists_bytes - head_bytes - 4096 : 0;
    const int64_t forced_chunk = opt.adc_screen_lists_chunk_queries.load(std::memory_order_relaxed);
    int64_t chunk = std::min<int64_t>(nq, kFslMaxEntries / n_probe);
    chunk = forced_chunk > 0 ? std::min<int64_t>(chunk, forced_chunk) : std::min<int64_t>(chunk, (int64_t)(room / per_q));
    chunk = std::max<int64_t>(chunk, 1);
    const int64_t entries_max = chunk * n_probe;
    const size_t img_bytes = (size_t)round_up(chunk * pitch, 256);
    const size_t prm_bytes = (size_t)round_up(chunk * (int64_t)sizeof(AdcScreenPrm), 256);
    const size_t ent8_bytes = (size_t)round_up(entries_max * 8, 256);
    const size_t scan0_bytes = (size_t)round_up((chunk + 1) * 8, 256);
    const size_t pairs_bytes = (size_t)round_up(entries_max * 4, 256);
    const size_t fixed = head_bytes + img_bytes + prm_bytes + 2 * ent8_bytes + scan0_bytes + pairs_bytes + lists_bytes;
    // a single query whose words exceed the bound keeps what fits; the fill pass forms the rest again
    const int64_t budget = std::max<int64_t>(0, std::min<int64_t>(chunk * words_q, fixed < kListsScratchBytes ? (int64_t)((kListsScratchBytes - fixed) / 4) : 0));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire(fixed + (size_t)budget * 4 + 256));
    char* p = (char*)lease.ptr();
    int* ext = (int*)p;                                p += head_bytes;
    uint8_t* imgq = (uint8_t*)p;                       p += img_bytes;
    AdcScreenPrm* prm = (AdcScreenPrm*)p;              p += prm_bytes;
    int64_t* cnt = (int64_t*)p;                        p += ent8_bytes;
    int64_t* hoff = (int64_t*)p;                       p += ent8_bytes;
    int64_t* scan0 = (int64_t*)p;                      p += scan0_bytes;
    unsigned* pairs = (unsigned*)p;                    p += pairs_bytes;
    int64_t* unit_off = (int64_t*)p;                   // [n_lists + 1], then the three 4-byte arrays
    unsigned* lcnt = (unsigned*)(unit_off + n_lists + 1);
    unsigned* cursor = lcnt + n_lists;
    unsigned* pair_off = cursor + n_lists;             // [n_lists + 1]
    p += lists_bytes;
    uint32_t* hits = (uint32_t*)p;
    {                                                               // one reduction per call: scale 0, term +Inf to start from
        HIPCHK(hipMemsetAsync(ext, 0, sizeof(int), st));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(ext + 1), 0x7f800000, 1, st));
        const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
        if (d_scales) {
            hipLaunchKernelGGL(k_adc_screen_scale_max, dim3(g), dim3(256), 0, st, d_scales, n, (unsigned*)ext);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_scale_max");
        } else if (!ip) {
            hipLaunchKernelGGL(k_adc_screen_term_min, dim3(g), dim3(256), 0, st, d_row_terms, n, ext + 1);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_term_min");
        }
    }
    const float* xrow = ip ? d_scales : d_row_terms;
    AdcScreenResLaunch a{(const uint8_t*)d_codes, n, c_rs, d_allow, xrow, nullptr, b_rs, ext, d_list_off, n_lists, nullptr, (int)n_probe, p_rs,
                         0, lcnt, pair_off, unit_off, pairs, imgq, pitch, prm, M, K, unit_rows, hoff, budget, hits, cnt, capacity, d_idx,
                         (unsigned)wgs, ef.flag, st};
    for (int64_t q = 0; q < nq; q += chunk) {
        const int64_t nqc = std::min<int64_t>(chunk, nq - q);
        const int64_t entries = nqc * n_probe;
        const unsigned plan_grid = (unsigned)((entries + kFslPlanThreads - 1) / kFslPlanThreads);
        a.probes = d_probes + q * p_rs;
        a.bias = d_probe_bias + q * b_rs;
        a.nq = nqc;
        hipLaunchKernelGGL(k_adc_screen_lists_residual_prep, dim3((unsigned)nqc), dim3(kAsPrepThreads), 0, st,
                           d_tables + q * (int64_t)M * K, M, K, d_thr + q, (int)ip, d_scales ? 1 : 0, (const int*)ext, d_list_off, n_lists, n,
                           a.probes, (int)n_probe, p_rs, a.bias, b_rs, imgq, pitch, prm);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_screen_lists_residual_prep");
        HIPCHK(hipMemsetAsync(lcnt, 0, (size_t)n_lists * 2 * sizeof(unsigned), st));   // pairs per list and the cursors
        hipLaunchKernelGGL(k_fsl_pairs, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, d_list_off, n_lists, a.probes, (int)n_probe, p_rs,
                           n, nqc, lcnt, hoff, cnt, scan0, ef.flag);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_pairs");
        hipLaunchKernelGGL(k_fsl_units, dim3(1), dim3(1024), 0, st, d_list_off, n_lists, n, lcnt, slots, unit_rows, pair_off, unit_off);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_units");
        hipLaunchKernelGGL(k_fsl_scatter, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, a.probes, (int)n_probe, p_rs, nqc, hoff, pair_off,
                           cursor, pairs);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_scatter");
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, hoff, (int64_t)n_probe, nqc, scan0);   // tiles -> first hit word
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        PQCHK(launch_adc_screen_res(nvb, slots, ip != 0, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, cnt, (int64_t)n_probe, nqc, d_lims + q);   // counts -> first slot
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) {                                         // capacity == 0: a pure count call
            const unsigned grid = (unsigned)std::min<int64_t>((entries + kRangeWaves - 1) / kRangeWaves, kAdcScreenResWgsMax);
            auto fill = ip ? k_adc_screen_lists_residual_fill<true> : k_adc_screen_lists_residual_fill<false>;
            hipLaunchKernelGGL(fill, dim3(grid), dim3(64 * kRangeWaves), 0, st, a.codes, n, c_rs, d_allow, xrow, a.bias, b_rs, d_list_off,
                               n_lists, a.probes, (int)n_probe, p_rs, nqc, imgq, pitch, prm, M, K, hoff, budget, hits, cnt, capacity, d_idx);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_lists_residual_fill");
        }
    }
    return PQHIP_OK;
}

}  // extern "C"
