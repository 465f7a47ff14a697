// pqhip_adc_packed4.hip -- 4-bit packed codes (include/pqhip.h: pqhip_pack_codes4_dev, pqhip_unpack_codes4_dev and the
// six pqhip_adc_*search*_packed4_f32_dev).  The unit holds the entry points, the route on which the packed searches
// enter the drivers of pqhip_adc.hip (adc_search_launch.h: the policy of a search is theirs), and the instantiations of
// the exhaustive producers and of the pack / unpack kernels (kernels_adc_packed4.hip.h).  The list producers are
// instantiated in pqhip_adc_packed4_lists.hip.  Nothing in pqhip_adc.hip refers to this unit.
#include "adc_search_launch.h"

#define PQHIP_ADC_TEMPLATES_ONLY   // kernels_adc.hip.h: its non-template kernels belong to pqhip_adc.hip
#include "kernels_adc_packed4.hip.h"

using namespace pqhip;

namespace pqh {

// Packed dwords fetched per row: ceil(PB / 4) rounded up to an instantiated width (a wider window only reads past the
// row inside the matrix; adc_fetch_row takes byte loads at its ends).  M <= 100: at most 13.
static int packed4_nv_bucket(int nv)
{
    for (int b : {1, 2, 4, 8, kPacked4MaxValueWords})
        if (nv <= b) return b;
    return 0;
}

static int packed4_lists_nv_bucket(int nv)
{
    for (int b : {2, 8, kPacked4MaxValueWords})
        if (nv <= b) return b;
    return 0;
}

template <bool IP, int NV, int NQ, int L>
int32_t launch_search_p4(const SearchLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    if constexpr (NQ * L > 16) {
        return PQHIP_EUNSUPPORTED;
    } else {
        HIPCHK(hipFuncSetAttribute((const void*)k_adc_search_p4<IP, NV, NQ, L>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((k_adc_search_p4<IP, NV, NQ, L>), dim3(a.grid), dim3(1024), lds, a.st, packed, a.n, a.c_rs, a.allow, lut,
                           a.scales, a.M, a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
        if (IP) note_kernel(NQ == 8 ? "k_adc_ip_search_p4_mq<8 queries>" : NQ == 4 ? "k_adc_ip_search_p4_mq<4 queries>" : "k_adc_ip_search_p4");
        else note_kernel(NQ == 8 ? "k_adc_search_p4_mq<8 queries>" : NQ == 4 ? "k_adc_search_p4_mq<4 queries>" : "k_adc_search_p4");
        return PQHIP_OK;
    }
}

int32_t launch_search_packed4(bool ip, int nq_pass, int L, int nvb, const SearchLaunch& a, const void* packed, const float* lut,
                              size_t lds)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_queries_per_pass(nq_pass, [&](auto nq_c) {
            return dispatch_list_regs(L, [&](auto l_c) {
                return dispatch_int<1, 2, 4, 8, kPacked4MaxValueWords>(nvb, [&](auto nv_c) {
                    return launch_search_p4<decltype(ip_c)::value != 0, decltype(nv_c)::value, decltype(nq_c)::value,
                                            decltype(l_c)::value>(a, (const uint8_t*)packed, lut, lds);
                });
            });
        });
    });
}

// The packed searches enter the drivers of pqhip_adc.hip with their own routes: rows of PB = ceil(M / 2) bytes, a table
// image of M x 16 entries per query whatever K is (kernels_adc_packed4.hip.h) -- which is what the queries per pass are
// chosen from -- packed dwords per row, and the packed producers.  First the checks that need the format, in the order
// of every search: EINVAL (the caller's `bad_args`: negative counts), ENODEV, EUNSUPPORTED.
static int32_t packed4_checks(const pqhip_codebook* cb, int32_t slot, bool bad_args, int32_t k)
{
    if (!cb || bad_args) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16 || cb->M > 100 || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    return PQHIP_OK;
}

// Option "adc_packed4_wgs" forces the number of producer workgroups.
static int32_t adc_search_packed4(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const uint8_t* d_packed,
                                  int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales, int32_t k, float* d_val,
                                  int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    PQCHK(packed4_checks(cb, slot, nq < 0 || n < 0 || k < 1, k));
    const int PB = ((int)cb->M + 1) / 2;
    const SearchRoute r{PB, (size_t)cb->M * 16 * sizeof(float), packed4_nv_bucket((PB + 3) / 4), true,
                        cb->ctx->opt.adc_packed4_wgs.load(std::memory_order_relaxed), launch_search_packed4};
    return adc_search_run(ip, cb, slot, r, d_tables, nq, d_packed, n, c_rs, d_allow, d_scales, k, d_val, v_rs, d_idx, i_rs, stream);
}

// res != null: the residual searches; d_scales then holds the row terms of the distance search (required).
static int32_t adc_search_lists_packed4(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                        const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                        const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                        int64_t p_rs, const float* d_scales, int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx,
                                        int64_t i_rs, void* stream, const ListsResidual* res)
{
    PQCHK(packed4_checks(cb, slot, nq < 0 || n < 0 || k < 1 || n_lists < 0 || n_probe < 1, k));
    const int PB = ((int)cb->M + 1) / 2;
    const ListsRoute r{PB, (size_t)cb->M * 16 * sizeof(float), packed4_lists_nv_bucket((PB + 3) / 4), launch_lists_packed4};
    return adc_search_lists_run(ip, cb, slot, r, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe, p_rs,
                                d_scales, k, d_val, v_rs, d_idx, i_rs, stream, res);
}

// one lane per aligned dword of the span [p, p + bytes)
static int64_t span_blocks(const void* p, int64_t bytes)
{
    const int64_t dwords = (bytes + (int64_t)((uintptr_t)p & 3) + 3) / 4;
    return (dwords + 255) / 256;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_pack_codes4_dev(pqhip_codebook* cb, int32_t slot, const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                              uint8_t* d_packed, int64_t p_rs, void* stream)
{
    if (!cb || n < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16 || (code_bytes != 1 && code_bytes != 4)) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, PB = (M + 1) / 2;
    if (n > 0 && p_rs >= PB && (n - 1) > (((int64_t)1 << 39) - PB) / p_rs) return PQHIP_EUNSUPPORTED;
    if (n == 0) return PQHIP_OK;
    if (!d_codes || !d_packed) return PQHIP_EINVAL;
    if (c_rs < M || p_rs < PB) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const unsigned blocks = (unsigned)span_blocks(d_packed, (n - 1) * p_rs + PB);
    if (code_bytes == 1)
        hipLaunchKernelGGL(k_pack_codes4<uint8_t>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)d_codes, n, c_rs, M, (int)cb->K,
                           d_packed, p_rs, ef.flag);
    else
        hipLaunchKernelGGL(k_pack_codes4<uint32_t>, dim3(blocks), dim3(256), 0, st, (const uint32_t*)d_codes, n, c_rs, M, (int)cb->K,
                           d_packed, p_rs, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_pack_codes4");
    return PQHIP_OK;
}

int32_t pqhip_unpack_codes4_dev(pqhip_codebook* cb, int32_t slot, const uint8_t* d_packed, int64_t n, int64_t p_rs,
                                const int64_t* d_rows, int64_t n_rows, uint8_t* d_out, int64_t o_rs, void* stream)
{
    if (!cb || n < 0 || (d_rows && n_rows < 0)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, PB = (M + 1) / 2;
    const int64_t n_out = d_rows ? n_rows : n;
    if (n_out > 0 && o_rs >= M && (n_out - 1) > (((int64_t)1 << 39) - M) / o_rs) return PQHIP_EUNSUPPORTED;
    if (n_out == 0) return PQHIP_OK;
    if (!d_out || (n > 0 && !d_packed)) return PQHIP_EINVAL;
    if (o_rs < M || (n > 0 && p_rs < PB)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const unsigned blocks = (unsigned)span_blocks(d_out, (n_out - 1) * o_rs + M);
    hipLaunchKernelGGL(k_unpack_codes4, dim3(blocks), dim3(256), 0, st, d_packed, n, p_rs, d_rows, n_out, M, d_out, o_rs, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_unpack_codes4");
    return PQHIP_OK;
}

int32_t pqhip_adc_search_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const uint8_t* d_packed,
                                         int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t k, float* d_dist, int64_t d_rs,
                                         int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_ip_search_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                            const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                            const float* d_scales, int32_t k, float* d_score, int64_t s_rs, int64_t* d_idx,
                                            int64_t i_rs, void* stream)
{
    return adc_search_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_search_lists_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                               const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                               const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                               int64_t p_rs, int32_t k, float* d_dist, int64_t d_rs, int64_t* d_idx, int64_t i_rs,
                                               void* stream)
{
    return adc_search_lists_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream, nullptr);
}

int32_t pqhip_adc_ip_search_lists_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                  const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                  const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                  int32_t n_probe, int64_t p_rs, const float* d_scales, int32_t k, float* d_score,
                                                  int64_t s_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_lists_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, nullptr);
}

int32_t pqhip_adc_search_lists_residual_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                        const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                        const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                        int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                        const float* d_row_terms, int32_t k, float* d_dist, int64_t d_rs,
                                                        int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_row_terms, k, d_dist, d_rs, d_idx, i_rs, stream, &res);
}

int32_t pqhip_adc_ip_search_lists_residual_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                           const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                           const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                           int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                           const float* d_scales, int32_t k, float* d_score, int64_t s_rs,
                                                           int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, &res);
}

}  // extern "C"
