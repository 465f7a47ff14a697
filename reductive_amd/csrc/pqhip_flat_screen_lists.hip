// pqhip_flat_screen_lists.hip -- conservative range screen in probed lists on the matrix cores (include/pqhip.h:
// pqhip_flat_screen_lists_f32_dev): the entry point, its policy (checks, chunks of queries, scratch, the prep / pairs /
// units / scatter / scan / count / scan / fill sequence) and the instantiations of kernels_flat_screen_lists.hip.h.  The
// image kernel is the screen's k_flat_screen_prep, both scans are the ADC range searches' k_adc_range_scan.  A unit of its
// own so that the build compiles its kernels beside the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_screen_lists.hip.h"

using namespace pqhip;

namespace pqh {

constexpr int kFlatScreenListsWideD = 1024;      // groups of 64 pairs while their image fits the LDS, else of 32
constexpr int64_t kFlatScreenListsUnitRows = 1024;   // 8 waves x 4 tiles: the gather of a group is a few percent of a unit
constexpr int64_t kFlatScreenListsWgsMax = 65535;

struct FlatScreenListsLaunch {
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    const int64_t* list_off;
    int64_t n_lists;
    const int64_t* probes;
    int n_probe;
    int64_t p_rs, nq;
    const unsigned *lcnt, *pair_off;
    const int64_t* unit_off;
    const unsigned* pairs;
    const unsigned short* img;
    const float2* prm;
    int ldq;
    float cx, cxx;
    int al;
    int64_t unit_rows;
    const int64_t* hoff;
    int64_t budget;
    uint32_t* hits;
    int64_t* cnt;
    int64_t capacity;
    int64_t* out_i;
    unsigned grid;
    hipStream_t st;
};

template <typename T, int NB>
static int32_t launch_flat_screen_lists_t(const FlatScreenListsLaunch& a)
{
    auto kern = k_flat_screen_lists<T, NB>;
    const size_t lds = flat_screen_lists_lds(32 * NB, a.d);         // at most 133 KB; the kernel has 16 static bytes beside it
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(64 * kFsWaves), lds, a.st, (const T*)a.x, a.n, a.d,
                       a.x_rs, a.allow, a.list_off, a.n_lists, a.lcnt, a.pair_off, a.unit_off, a.pairs, a.n_probe, a.img, a.prm,
                       a.ldq, a.cx, a.cxx, a.al, a.unit_rows, a.hoff, a.budget, a.hits, (unsigned long long*)a.cnt);
    return PQHIP_OK;
}

static int32_t launch_flat_screen_lists(bool f16, int nb, const FlatScreenListsLaunch& a)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<2, 1>(nb, [&](auto nb_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            return launch_flat_screen_lists_t<T, decltype(nb_c)::value>(a);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(nb == 2 ? "k_flat_screen_lists<64 pairs>" : "k_flat_screen_lists<32 pairs>");
    return PQHIP_OK;
}

template <typename T>
static int32_t launch_flat_screen_lists_fill_t(const FlatScreenListsLaunch& a)
{
    const int64_t entries = a.nq * a.n_probe;
    const unsigned grid = (unsigned)std::min<int64_t>((entries + kFsWaves - 1) / kFsWaves, kFlatScreenListsWgsMax);
    hipLaunchKernelGGL(k_flat_screen_lists_fill<T>, dim3(grid), dim3(64 * kFsWaves), 0, a.st, (const T*)a.x, a.n, a.d, a.x_rs, a.allow,
                       a.list_off, a.n_lists, a.probes, a.n_probe, a.p_rs, a.nq, a.img, a.prm, a.ldq, a.cx, a.cxx, a.al, a.hoff,
                       a.budget, a.hits, a.cnt, a.capacity, a.out_i);
    HIPCHK(hipGetLastError());
    note_kernel("k_flat_screen_lists_fill");
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

// Chunks of queries: at most kFslMaxEntries (query, slot) entries -- one scan launch -- and a scratch of at most
// kListsScratchBytes (option "flat_screen_lists_chunk_queries" forces the number).  Scratch of a chunk: the f16 image
// and the (s, tau) pairs of its queries; per entry the count, the first hit word and the pair's place; per list its
// pairs, cursor and the two prefixes; the hit words.  A fixed grid of four workgroups per CU (option
// "flat_screen_lists_wgs") strides over the units; a unit has 1,024 rows (option "flat_screen_lists_unit_rows").
int32_t pqhip_flat_screen_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                        int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const uint32_t* d_allow,
                                        const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                        int64_t p_rs, int32_t metric, int32_t x_exp, const float* d_thr, int64_t* d_lims,
                                        int64_t* d_idx, int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n_rows < 0 || capacity < 0 || d < 1 || (metric != 0 && metric != 1) || n_lists < 0 || n_probe < 1)
        return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if ((vec_bytes != 2 && vec_bytes != 4) || d > kFlatScreenMaxD || n_rows > (int64_t)0xfffffffell || n_probe > kFslMaxEntries)
        return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || !d_q || (n_rows > 0 && !d_x) || !d_list_off || !d_probes) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d) || p_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0 || n_lists == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first chunk starts from it
    ErrFlag ef(cb, slot, st);
    const Options& opt = cb->ctx->opt;
    const int nb = d <= kFlatScreenListsWideD ? 2 : 1;
    const int ldq = flat_screen_dp((int)d) + kFsRowPad;
    const int64_t forced_rows = opt.flat_screen_lists_unit_rows.load(std::memory_order_relaxed);
    const int64_t unit_rows = forced_rows > 0 ? round_up(forced_rows, kFsTile) : kFlatScreenListsUnitRows;
    const int64_t forced_wgs = opt.flat_screen_lists_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = std::min<int64_t>(forced_wgs > 0 ? forced_wgs : 4 * (int64_t)cb->ctx->devs[slot]->n_cus, kFlatScreenListsWgsMax);
    // per list: lcnt, cursor, pair_off (+1), unit_off (+1); per query: image row, (s, tau), the dummy lims of the tile
    // scan, per entry cnt, hoff and the pair; the hit words
    const size_t lists_bytes = (size_t)round_up((n_lists + 1) * 20, 256);
    const int64_t words_q = fsl_words_per_query(n_rows, n_lists, n_probe);
    const size_t per_q = (size_t)ldq * 2 + 8 + 8 + (size_t)n_probe * 20 + (size_t)words_q * 4;
    const size_t room = kListsScratchBytes > lists_bytes + 4096 ? kListsScratchBytes - lists_bytes - 4096 : 0;
    const int64_t forced_chunk = opt.flat_screen_lists_chunk_queries.load(std::memory_order_relaxed);
    int64_t chunk = std::min<int64_t>(nq, kFslMaxEntries / n_probe);
    chunk = forced_chunk > 0 ? std::min<int64_t>(chunk, forced_chunk) : std::min<int64_t>(chunk, (int64_t)(room / per_q));
    chunk = std::max<int64_t>(chunk, 1);
    const int64_t entries_max = chunk * n_probe;
    const size_t img_bytes = (size_t)round_up(chunk * ldq * 2, 256);
    const size_t prm_bytes = (size_t)round_up(chunk * 8, 256);
    const size_t ent8_bytes = (size_t)round_up(entries_max * 8, 256);
    const size_t scan0_bytes = (size_t)round_up((chunk + 1) * 8, 256);
    const size_t pairs_bytes = (size_t)round_up(entries_max * 4, 256);
    const size_t fixed = img_bytes + prm_bytes + 2 * ent8_bytes + scan0_bytes + pairs_bytes + lists_bytes;
    // a single query whose words exceed the bound keeps what fits; the fill pass forms the rest again
    const int64_t budget = std::max<int64_t>(0, std::min<int64_t>(chunk * words_q, fixed < kListsScratchBytes ? (int64_t)((kListsScratchBytes - fixed) / 4) : 0));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire(fixed + (size_t)budget * 4 + 256));
    char* p = (char*)lease.ptr();
    unsigned short* img = (unsigned short*)p;          p += img_bytes;
    float2* prm = (float2*)p;                          p += prm_bytes;
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
    const int xe = (int)std::max<int32_t>(-126, std::min<int32_t>(126, x_exp));   // beyond +-40 every query returns every allowed row
    const bool ip = metric != 0;
    const uint64_t low = (uint64_t)(uintptr_t)d_x | ((uint64_t)x_rs * (uint64_t)vec_bytes);   // what base and row stride are both multiples of
    const int al = low % 16 == 0 ? 16 : low % 8 == 0 ? 8 : low % 4 == 0 ? 4 : 2;
    FlatScreenListsLaunch a{d_x, n_rows, (int)d, x_rs, d_allow, d_list_off, n_lists, nullptr, (int)n_probe, p_rs, 0, lcnt, pair_off,
                            unit_off, pairs, img, prm, ldq, std::ldexp(1.0f, xe), ip ? -0.5f * kFlatScreenRel : 1.0f - kFlatScreenRel,
                            al, unit_rows, hoff, budget, hits, cnt, capacity, d_idx, (unsigned)wgs, st};
    for (int64_t q = 0; q < nq; q += chunk) {
        const int64_t nqc = std::min<int64_t>(chunk, nq - q);
        const int64_t entries = nqc * n_probe;
        const unsigned plan_grid = (unsigned)((entries + kFslPlanThreads - 1) / kFslPlanThreads);
        a.probes = d_probes + q * p_rs;
        a.nq = nqc;
        hipLaunchKernelGGL(k_flat_screen_prep, dim3((unsigned)nqc), dim3(kFsPrepThreads), 0, st, d_q + q * q_rs, q_rs, (int)nqc, (int)d,
                           ldq, d_thr + q, ip ? 1 : 0, (int)x_exp, img, (float*)prm);
        HIPCHK(hipGetLastError());
        note_kernel("k_flat_screen_prep");
        HIPCHK(hipMemsetAsync(lcnt, 0, (size_t)n_lists * 2 * sizeof(unsigned), st));   // pairs per list and the cursors
        hipLaunchKernelGGL(k_fsl_pairs, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, d_list_off, n_lists, a.probes, (int)n_probe, p_rs,
                           n_rows, nqc, lcnt, hoff, cnt, scan0, ef.flag);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_pairs");
        hipLaunchKernelGGL(k_fsl_units, dim3(1), dim3(1024), 0, st, d_list_off, n_lists, n_rows, lcnt, 32 * nb, unit_rows, pair_off,
                           unit_off);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_units");
        hipLaunchKernelGGL(k_fsl_scatter, dim3(plan_grid), dim3(kFslPlanThreads), 0, st, a.probes, (int)n_probe, p_rs, nqc, hoff, pair_off,
                           cursor, pairs);
        HIPCHK(hipGetLastError());
        note_kernel("k_fsl_scatter");
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, hoff, (int64_t)n_probe, nqc, scan0);   // tiles -> first hit word
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        PQCHK(launch_flat_screen_lists(vec_bytes == 2, nb, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, cnt, (int64_t)n_probe, nqc, d_lims + q);   // counts -> first slot
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0)                                           // capacity == 0: a pure count call
            PQCHK(vec_bytes == 2 ? launch_flat_screen_lists_fill_t<_Float16>(a) : launch_flat_screen_lists_fill_t<float>(a));
    }
    return PQHIP_OK;
}

}  // extern "C"
