// pqhip_flat_search.hip -- exact search over resident vectors (include/pqhip.h: pqhip_flat_search_f32_dev): the entry
// point, the host policy and the instantiations of k_flat_search (kernels_flat_search.hip.h).  List length, LDS budget and
// the merge of the partial lists are the ADC searches' (adc_search_launch.h); this unit owns the queries per pass, the
// producer grid and the scratch of its partial lists.  A unit of its own so that the build compiles its producers beside
// the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_search.hip.h"

using namespace pqhip;

namespace pqh {

struct FlatLaunch {
    const float* q;
    int64_t q_rs;
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    int k;
    int64_t rows_per_wg;
    unsigned grid;
    unsigned* part_k;
    uint64_t* part_i;
    hipStream_t st;
};

// Queries per pass.  Every query of a pass keeps kFlatTile partials per lane beside its list (2 L VGPRs), and a
// 1,024-thread workgroup leaves 128 VGPRs per lane: 4 queries while L <= 2 (k <= 128) -- 64 partials, 16 row elements,
// 16 list registers -- and while 4 query images and the queues fit the 160 KB of LDS (d <= 9,216); else one.
//      k <= 128 and d <= 9,216:  4 queries per pass (the last nq mod 4 queries one per pass)
//      otherwise:                1
static int flat_queries_per_pass(int64_t nq_left, int d, int L)
{
    return nq_left >= 4 && L <= 2 && search_lds((size_t)4 * d * sizeof(float), 4, L) <= 160 * 1024 ? 4 : 1;
}

template <typename T, bool IP, int NQ, int L>
static int32_t launch_flat_t(const FlatLaunch& a, size_t lds)
{
    auto kern = k_flat_search<T, IP, NQ, L>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), lds, a.st, a.q, a.q_rs, (const T*)a.x, a.n, a.d, a.x_rs, a.allow, a.k,
                       a.rows_per_wg, a.part_k, a.part_i);
    return PQHIP_OK;
}

static int32_t launch_flat(bool f16, bool ip, int nqp, int L, const FlatLaunch& a, size_t lds)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<0, 1>(ip, [&](auto ip_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            constexpr bool IP = decltype(ip_c)::value != 0;
            if (nqp == 4) {
                return dispatch_int<1, 2>(L, [&](auto l_c) { return launch_flat_t<T, IP, 4, decltype(l_c)::value>(a, lds); });
            }
            return dispatch_list_regs(L, [&](auto l_c) { return launch_flat_t<T, IP, 1, decltype(l_c)::value>(a, lds); });
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    if (nqp == 4) note_kernel(ip ? "k_flat_ip_search<4 queries>" : "k_flat_search<4 queries>");
    else note_kernel(ip ? "k_flat_ip_search" : "k_flat_search");
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_flat_search_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                  int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const uint32_t* d_allow,
                                  int32_t metric, int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!cb || nq < 0 || n_rows < 0 || k < 1 || d < 1 || (metric != 0 && metric != 1)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (vec_bytes != 2 && vec_bytes != 4) return PQHIP_EUNSUPPORTED;
    if (k > kSearchMaxK || d > kFlatMaxD) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_q || !d_val || !d_idx || (n_rows > 0 && !d_x)) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d) || v_rs < k || i_rs < k) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const bool ip = metric != 0;
    const int L = search_list_regs(k);
    if (n_rows == 0) return adc_search_merge(ip, L, nq, 0, k, nullptr, nullptr, d_val, v_rs, d_idx, i_rs, st);
    // one 1,024-thread workgroup per CU, a contiguous row range each: a multiple of 1,024 rows (a tile's mask bits then
    // lie in one word; offsets within a range are 32-bit)
    const int64_t forced = cb->ctx->opt.flat_search_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, 65536) : cb->ctx->devs[slot]->n_cus;
    int64_t rows_per_wg = round_up((n_rows + wgs - 1) / wgs, 1024);
    rows_per_wg = std::min<int64_t>(rows_per_wg, (int64_t)1 << 30);
    const int64_t grid = (n_rows + rows_per_wg - 1) / rows_per_wg;
    const int nqp_first = flat_queries_per_pass(nq, (int)d, L);
    const size_t list_entries = (size_t)nqp_first * grid * 64 * L;
    ScratchLease part(cb, slot, st);
    PQCHK(part.acquire(list_entries * (sizeof(unsigned) + sizeof(uint64_t))));
    uint64_t* part_i = (uint64_t*)part.ptr();
    unsigned* part_k = (unsigned*)(part_i + list_entries);
    const FlatLaunch a{nullptr, q_rs, d_x, n_rows, (int)d, x_rs, d_allow, k, rows_per_wg, (unsigned)grid, part_k, part_i, st};
    for (int64_t q = 0; q < nq;) {
        const int nqp = flat_queries_per_pass(nq - q, (int)d, L);
        FlatLaunch aq = a;
        aq.q = d_q + q * q_rs;
        PQCHK(launch_flat(vec_bytes == 2, ip, nqp, L, aq, search_lds((size_t)nqp * d * sizeof(float), nqp, L)));
        PQCHK(adc_search_merge(ip, L, nqp, (int)grid, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
        q += nqp;
    }
    return PQHIP_OK;
}

}  // extern "C"
