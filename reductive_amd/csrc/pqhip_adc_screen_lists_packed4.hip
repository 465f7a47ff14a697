// pqhip_adc_screen_lists_packed4.hip -- the one-hot i8 screen over 4-bit packed rows in probed lists (include/pqhip.h:
// pqhip_adc_screen_lists_packed4_f32_dev): the entry point, its policy (checks, slots per group, chunks of queries,
// scratch, the scale / prep / pairs / units / scatter / scan / count / scan / fill sequence -- that of
// pqhip_adc_screen_lists.hip) and the instantiations of kernels_adc_screen_lists_packed4.hip.h.  The planning kernels
// are the flat list screen's, both scans are the ADC range searches' k_adc_range_scan, the packed dwords per row are the
// wider buckets of the packed searches.  A unit of its own; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_adc_screen_lists_packed4.hip.h"

using namespace pqhip;

namespace pqh {

constexpr size_t kAdcScreenListsP4Lds = 160 * 1024;
constexpr int64_t kAdcScreenListsP4UnitRows = 16384;   // 16 waves x 32 tiles; the u8 list screen's
constexpr int64_t kAdcScreenListsP4WgsMax = 65535;

struct AdcScreenListsP4Launch {
    const uint8_t* codes;
    int64_t n, c_rs;
    const uint32_t* allow;
    const float* scales;
    const int64_t* list_off;
    int64_t n_lists;
    const unsigned *lcnt, *pair_off;
    const int64_t* unit_off;
    const unsigned* pairs;
    int n_probe;
    const uint8_t* imgq;
    int64_t pitch;
    const AdcScreenPrm* prm;
    int M, K;
    int64_t unit_rows;
    const int64_t* hoff;
    int64_t budget;
    uint32_t* hits;
    int64_t* cnt;
    unsigned grid;
    int* err;
    hipStream_t st;
};

template <int NV, int QB>
static int32_t launch_adc_screen_lists_p4_t(const AdcScreenListsP4Launch& a)
{
    auto kern = k_adc_screen_lists_p4<NV, QB>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAdcScreenListsP4Lds));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), adc_screen_lists_p4_lds_bytes(a.M, QB), a.st, a.codes, a.n, a.c_rs, a.allow,
                       a.scales, a.list_off, a.n_lists, a.lcnt, a.pair_off, a.unit_off, a.pairs, a.n_probe, a.imgq, a.pitch, a.prm, a.M,
                       a.K, a.unit_rows, a.hoff, a.budget, a.hits, (unsigned long long*)a.cnt, a.err);
    return PQHIP_OK;
}

// blocks of 32 slots per group: two, and one for rows of more than 32 packed bytes (M > 64), where the 14 row dwords
// beside 32 accumulators spill vector registers (kP4ScreenMaxBlocks)
constexpr int adc_screen_lists_p4_blocks(int nvb) { return nvb < 13 ? kP4ScreenMaxBlocks : 1; }

// the three instantiations: <4, 2>, <8, 2>, <13, 1>
static int32_t launch_adc_screen_lists_p4(int nvb, const AdcScreenListsP4Launch& a)
{
    const int32_t status = dispatch_int<4, 8, 13>(nvb, [&](auto nv_c) {
        constexpr int NV = decltype(nv_c)::value;
        return launch_adc_screen_lists_p4_t<NV, adc_screen_lists_p4_blocks(NV)>(a);
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(adc_screen_lists_p4_blocks(nvb) == 2 ? "k_adc_screen_lists_p4<64 pairs>" : "k_adc_screen_lists_p4<32 pairs>");
    return PQHIP_OK;
}

// packed dwords per row: the wider buckets of the packed searches (a wider window is always correct).  The buckets 1 and
// 2 are not instantiated: around their short k loops the compiler keeps enough per-lane values over the tile loop to
// spill vector registers beside the 32 accumulators, and the unit is built without private memory.
static int adc_screen_lists_p4_nv_bucket(int nv)
{
    for (int b : {4, 8, 13})
        if (nv <= b) return b;
    return 0;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

// Chunks of queries, scratch, grid and units as in pqhip_adc_screen_lists_f32_dev, under the same three options; the
// image of a query takes 32 ceil(M / 2) bytes of the scratch.
int32_t pqhip_adc_screen_lists_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                               int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                               const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                               int64_t p_rs, int32_t ip, const float* d_scales, const float* d_thr, int64_t* d_lims,
                                               int64_t* d_idx, int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n < 0 || capacity < 0 || n_lists < 0 || n_probe < 1 || (ip != 0 && ip != 1) || (!ip && d_scales))
        return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || cb->M > kAdcScreenMaxM || cb->K > 16 || n > (int64_t)0xfffffffell || n_probe > kFslMaxEntries)
        return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, K = (int)cb->K, PB = (M + 1) / 2;
    const int nvb = adc_screen_lists_p4_nv_bucket((PB + 3) / 4);
    if (nvb == 0) return PQHIP_EUNSUPPORTED;
    const int blocks = adc_screen_lists_p4_blocks(nvb);
    if (adc_screen_lists_p4_lds_bytes(M, blocks) > kAdcScreenListsP4Lds) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || (n > 0 && (!d_tables || !d_codes)) || !d_list_off || !d_probes) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < PB) || p_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_lists == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const Options& opt = cb->ctx->opt;
    const int64_t pitch = adc_screen_lists_p4_pitch(M);
    const int64_t forced_rows = opt.adc_screen_lists_unit_rows.load(std::memory_order_relaxed);
    const int64_t unit_rows = forced_rows > 0 ? round_up(forced_rows, 64) : kAdcScreenListsP4UnitRows;
    const int64_t forced_wgs = opt.adc_screen_lists_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = std::min<int64_t>(forced_wgs > 0 ? forced_wgs : (int64_t)cb->ctx->devs[slot]->n_cus, kAdcScreenListsP4WgsMax);
    // per list: lcnt, cursor, pair_off (+1), unit_off (+1); per query: image, parameters, the dummy lims of the tile
    // scan, per entry cnt, hoff and the pair; the hit words
    const size_t head_bytes = 256;                                  // the largest scale
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
    unsigned* cmax = (unsigned*)p;                     p += head_bytes;
    uint8_t* imgq = (uint8_t*)p;                       p += img_bytes;    // 256-byte aligned: the count pass copies 16 bytes at a time
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
    if (d_scales) {                                                 // one reduction per call
        HIPCHK(hipMemsetAsync(cmax, 0, sizeof(unsigned), st));
        const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
        hipLaunchKernelGGL(k_adc_screen_scale_max, dim3(g), dim3(256), 0, st, d_scales, n, cmax);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_screen_scale_max");
    }
    const AdcScreenListsP4Launch a{(const uint8_t*)d_codes, n, c_rs, d_allow, d_scales, d_list_off, n_lists, lcnt, pair_off, unit_off, pairs,
                                   (int)n_probe, imgq, pitch, prm, M, K, unit_rows, hoff, budget, hits, cnt, (unsigned)wgs, ef.flag, st};
    for (int64_t q = 0; q < nq; q += chunk) {
        const int64_t nqc = std::min<int64_t>(chunk, nq - q);
        const int64_t entries = nqc * n_probe;
        const unsigned plan_grid = (unsigned)((entries + kFslPlanThreads - 1) / kFslPlanThreads);
        const int64_t* probes = d_probes + q * p_rs;
        hipLaunchKernelGGL(k_adc_screen_lists_p4_prep, dim3((unsigned)nqc), dim3(kAsPrepThreads), 0, st, d_tables + q * (int64_t)M * K, M, K,
                           d_thr + q, (int)ip, d_scales ? 1 : 0, cmax, (int8_t*)imgq, pitch, prm);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_screen_lists_p4_prep");
        HIPCHK(hipMemsetAsync(lcnt, 0, (size_t)n_lists * 2 * sizeof(unsigned), st));   // pairs per list and the cursors
        hipLaunchKernelGGL(k_fsl_pairs, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, d_list_off, n_lists, probes, (int)n_probe, p_rs, n,
                           nqc, lcnt, hoff, cnt, scan0, ef.flag);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_pairs");
        hipLaunchKernelGGL(k_fsl_units, dim3(1), dim3(1024), 0, st, d_list_off, n_lists, n, lcnt, 32 * blocks, unit_rows, pair_off, unit_off);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_units");
        hipLaunchKernelGGL(k_fsl_scatter, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, probes, (int)n_probe, p_rs, nqc, hoff, pair_off,
                           cursor, pairs);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_scatter");
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, hoff, (int64_t)n_probe, nqc, scan0);   // tiles -> first hit word
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        PQCHK(launch_adc_screen_lists_p4(nvb, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, cnt, (int64_t)n_probe, nqc, d_lims + q);   // counts -> first slot
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) {                                         // capacity == 0: a pure count call
            const unsigned grid = (unsigned)std::min<int64_t>((entries + kRangeWaves - 1) / kRangeWaves, kAdcScreenListsP4WgsMax);
            hipLaunchKernelGGL(k_adc_screen_lists_p4_fill, dim3(grid), dim3(64 * kRangeWaves), 0, st, a.codes, n, c_rs, d_allow, d_scales,
                               d_list_off, n_lists, probes, (int)n_probe, p_rs, nqc, (const int8_t*)imgq, pitch, prm, M, hoff, budget, hits,
                               cnt, capacity, d_idx);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_lists_p4_fill");
        }
    }
    return PQHIP_OK;
}

}  // extern "C"
