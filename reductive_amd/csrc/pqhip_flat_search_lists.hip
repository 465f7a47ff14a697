// pqhip_flat_search_lists.hip -- exact search in probed lists (include/pqhip.h: pqhip_flat_search_lists_f32_dev): the
// entry point, the host policy and the instantiations of k_flat_search_lists (kernels_flat_search_lists.hip.h).  The plan
// kernel, the list length, the LDS budget, the scratch bound of a chunk of queries and the merge are the list searches'
// (adc_search_launch.h); this unit owns the checks, the workgroups per query and the scratch layout.  A unit of its own so
// that the build compiles its producers beside the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_search_lists.hip.h"

using namespace pqhip;

namespace pqh {

struct FlatListsLaunch {
    const float* q;
    int64_t q_rs;
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    int k;
    const int64_t *seg_begin, *seg_cum;
    int n_probe;
    unsigned G, nq;          // grid (G, nq)
    unsigned* part_k;
    uint64_t* part_i;
    hipStream_t st;
};

// Workgroups per query, from what the host knows: the expected probed bytes (lists of average size).  lists_wgs_per_query
// counts rows of M code bytes; a row here is d elements, hundreds of times as many bytes, so a workgroup earns its fixed
// cost (the query image, the merge of its 16 waves' lists, one partial list) after far fewer rows.
//   one workgroup per 256 KB of probed rows, no more than one per 256 rows (16 waves x one tile: fewer leave waves idle)
//   and no more than the CUs the queries of a launch leave each other (one 1,024-thread workgroup per CU).
// The 256 KB are a starting rule that has NOT been measured (some 8 us of a CU's share of the HBM bandwidth, against a
// fixed cost of that order); tools/flat_lists_time.py sweeps the forced count beside it.  The estimate only sets the
// grid: slices are cut from the actual T_q on the device and the result does not depend on G.
static int64_t flat_lists_wgs_per_query(int64_t n, int64_t n_lists, int64_t n_probe, int64_t nq, int64_t row_bytes, int n_cus)
{
    const double frac = (double)std::min<int64_t>(n_probe, n_lists) / (double)n_lists;
    const int64_t expected = (int64_t)((double)n * frac) + 1;
    const int64_t by_bytes = (int64_t)(((double)expected * (double)row_bytes + 262143.0) / 262144.0);
    const int64_t by_tiles = (expected + kSearchWaves * kFlatTile - 1) / (kSearchWaves * kFlatTile);
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min({by_bytes, by_tiles, by_cus}));
}

template <typename T, bool IP, int L>
static int32_t launch_flat_lists_t(const FlatListsLaunch& a, size_t lds)
{
    auto kern = k_flat_search_lists<T, IP, L>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.G, a.nq), dim3(1024), lds, a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d, a.x_rs, a.allow, a.k,
                       a.seg_begin, a.seg_cum, a.n_probe, a.part_k, a.part_i);
    return PQHIP_OK;
}

static int32_t launch_flat_lists(bool f16, bool ip, int L, const FlatListsLaunch& a, size_t lds)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            constexpr bool IP = decltype(ip_c)::value != 0;
            return dispatch_list_regs(L, [&](auto l_c) { return launch_flat_lists_t<T, IP, decltype(l_c)::value>(a, lds); });
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(ip ? "k_flat_ip_search_lists" : "k_flat_search_lists");
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_flat_search_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                        int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const int64_t* d_list_off,
                                        int64_t n_lists, const int64_t* d_probes, int32_t n_probe, int64_t p_rs,
                                        const uint32_t* d_allow, int32_t metric, int32_t k, float* d_val, int64_t v_rs,
                                        int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!cb || nq < 0 || n_rows < 0 || k < 1 || d < 1 || (metric != 0 && metric != 1) || n_lists < 0 || n_probe < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (vec_bytes != 2 && vec_bytes != 4) return PQHIP_EUNSUPPORTED;
    if (k > kSearchMaxK || d > kFlatMaxD) return PQHIP_EUNSUPPORTED;
    if (n_rows > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;                     // positions are offered as 32-bit values
    const size_t plan_q = ((size_t)n_probe * 2 + 1) * sizeof(int64_t);
    if (plan_q > kListsScratchBytes / 2) return PQHIP_EUNSUPPORTED;                    // n_probe >= 2^24
    if (nq == 0) return PQHIP_OK;
    if (!d_q || !d_val || !d_idx || !d_list_off || !d_probes || (n_rows > 0 && !d_x)) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d) || v_rs < k || i_rs < k || p_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const bool ip = metric != 0;
    const int L = search_list_regs(k);
    if (n_rows == 0 || n_lists == 0) return adc_search_merge(ip, L, nq, 0, k, nullptr, nullptr, d_val, v_rs, d_idx, i_rs, st);
    ErrFlag ef(cb, slot, st);
    const int64_t forced = cb->ctx->opt.flat_lists_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : flat_lists_wgs_per_query(n_rows, n_lists, n_probe, std::min<int64_t>(nq, 65535), d * vec_bytes,
                                                            cb->ctx->devs[slot]->n_cus);
    // plan and partial lists of one chunk of queries within 512 MB of scratch, as for the list searches over codes
    const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (plan_q + lists_q))}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (plan_q + lists_q)));
    // 8-byte items first: part_i [chunk][G][64 L], seg_begin [chunk][n_probe], seg_cum [chunk][n_probe + 1]; then the keys
    uint64_t* part_i = (uint64_t*)lease.ptr();
    int64_t* seg_begin = (int64_t*)(part_i + (size_t)chunk * G * 64 * L);
    int64_t* seg_cum = seg_begin + (size_t)chunk * n_probe;
    unsigned* part_k = (unsigned*)(seg_cum + (size_t)chunk * ((size_t)n_probe + 1));
    const size_t lds = search_lds((size_t)d * sizeof(float), 1, L);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        PQCHK(launch_lists_plan(d_list_off, n_lists, d_probes + q * p_rs, (int)n_probe, p_rs, n_rows, seg_begin, seg_cum, nqc, ef.flag, st));
        const FlatListsLaunch a{d_q + q * q_rs, q_rs, d_x, n_rows, (int)d, x_rs, d_allow, k, seg_begin, seg_cum, (int)n_probe,
                                (unsigned)G, nqc, part_k, part_i, st};
        PQCHK(launch_flat_lists(vec_bytes == 2, ip, L, a, lds));
        PQCHK(adc_search_merge(ip, L, nqc, (int)G, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
    }
    return PQHIP_OK;
}

}  // extern "C"
