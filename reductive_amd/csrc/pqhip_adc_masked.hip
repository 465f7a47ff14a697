// pqhip_adc_masked.hip -- the ADC searches restricted to an allowed set of rows (include/pqhip.h:
// pqhip_adc_*search*_masked_f32_dev, pqhip_pack_row_mask_dev).  The policy of a search is pqhip_adc.hip's, the same
// routines with the mask as one more field (adc_search_launch.h); this unit holds the entry points, the instantiations
// of the masked producers (kernels_adc_search_masked.hip.h) with their launchers, and packs a mask.  A unit of its own
// so that the build compiles it beside pqhip_adc.hip; nothing in pqhip_adc.hip refers to it.
#include "adc_search_launch.h"

#define PQHIP_ADC_TEMPLATES_ONLY   // kernels_adc.hip.h: its non-template kernels belong to pqhip_adc.hip
#include "kernels_adc_search_masked.hip.h"

using namespace pqhip;

namespace pqh {

template <bool IP, int NV, int NQ, int L>
int32_t launch_search_masked(const SearchLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    if constexpr (NQ * L > 16) {
        return PQHIP_EUNSUPPORTED;
    } else {
        const void* kern = IP ? (const void*)k_adc_ip_search_masked_u8<NV, NQ, L> : (const void*)k_adc_search_masked_u8<NV, NQ, L>;
        HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if constexpr (IP) {
            hipLaunchKernelGGL((k_adc_ip_search_masked_u8<NV, NQ, L>), dim3(a.grid), dim3(1024), lds, a.st, codes, a.n, a.c_rs,
                               a.allow, lut, a.scales, a.M, a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
            note_kernel(NQ == 8 ? "k_adc_ip_search_masked_u8_mq<8 queries>"
                                : NQ == 4 ? "k_adc_ip_search_masked_u8_mq<4 queries>" : "k_adc_ip_search_masked_u8");
        } else {
            hipLaunchKernelGGL((k_adc_search_masked_u8<NV, NQ, L>), dim3(a.grid), dim3(1024), lds, a.st, codes, a.n, a.c_rs,
                               a.allow, lut, a.M, a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
            note_kernel(NQ == 8 ? "k_adc_search_masked_u8_mq<8 queries>"
                                : NQ == 4 ? "k_adc_search_masked_u8_mq<4 queries>" : "k_adc_search_masked_u8");
        }
        return PQHIP_OK;
    }
}

template <bool IP, int NQ, int L>
int32_t launch_search_masked_nv(int nvb, const SearchLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    switch (nvb) {
    case 1: return launch_search_masked<IP, 1, NQ, L>(a, codes, lut, lds);
    case 2: return launch_search_masked<IP, 2, NQ, L>(a, codes, lut, lds);
    case 4: return launch_search_masked<IP, 4, NQ, L>(a, codes, lut, lds);
    case 8: return launch_search_masked<IP, 8, NQ, L>(a, codes, lut, lds);
    case 13: return launch_search_masked<IP, 13, NQ, L>(a, codes, lut, lds);
    case kAdcMaxValueWords: return launch_search_masked<IP, kAdcMaxValueWords, NQ, L>(a, codes, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

template <bool IP, int NQ>
int32_t launch_search_masked_l(int L, int nvb, const SearchLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    switch (L) {
    case 1: return launch_search_masked_nv<IP, NQ, 1>(nvb, a, codes, lut, lds);
    case 2: return launch_search_masked_nv<IP, NQ, 2>(nvb, a, codes, lut, lds);
    case 4: return launch_search_masked_nv<IP, NQ, 4>(nvb, a, codes, lut, lds);
    case 8: return launch_search_masked_nv<IP, NQ, 8>(nvb, a, codes, lut, lds);
    case 16: return launch_search_masked_nv<IP, NQ, 16>(nvb, a, codes, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

template <bool IP>
int32_t launch_search_masked_q(int nq_pass, int L, int nvb, const SearchLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    switch (nq_pass) {
    case 8: return launch_search_masked_l<IP, 8>(L, nvb, a, codes, lut, lds);
    case 4: return launch_search_masked_l<IP, 4>(L, nvb, a, codes, lut, lds);
    case 1: return launch_search_masked_l<IP, 1>(L, nvb, a, codes, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

int32_t launch_search_masked_u8(bool ip, int nq_pass, int L, int nvb, const SearchLaunch& a, const uint8_t* codes,
                                const float* lut, size_t lds)
{
    return ip ? launch_search_masked_q<true>(nq_pass, L, nvb, a, codes, lut, lds)
              : launch_search_masked_q<false>(nq_pass, L, nvb, a, codes, lut, lds);
}

template <bool IP, int NV, int L>
int32_t launch_lists_masked(const ListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    if (a.bias) {   // the residual producer
        HIPCHK(hipFuncSetAttribute((const void*)k_adc_search_lists_residual_masked_u8<IP, NV, L>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((k_adc_search_lists_residual_masked_u8<IP, NV, L>), dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n,
                           a.c_rs, a.allow, lut, a.bias, a.b_rs, a.scales, a.M, a.K, a.k, a.seg_begin, a.seg_cum, a.n_probe,
                           a.part_k, a.part_i, a.err);
        note_kernel(IP ? "k_adc_ip_search_lists_residual_masked_u8" : "k_adc_search_lists_residual_masked_u8");
        return PQHIP_OK;
    }
    HIPCHK(hipFuncSetAttribute((const void*)k_adc_search_lists_masked_u8<IP, NV, L>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((k_adc_search_lists_masked_u8<IP, NV, L>), dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n, a.c_rs,
                       a.allow, lut, a.scales, a.M, a.K, a.k, a.seg_begin, a.seg_cum, a.n_probe, a.part_k, a.part_i, a.err);
    note_kernel(IP ? "k_adc_ip_search_lists_masked_u8" : "k_adc_search_lists_masked_u8");
    return PQHIP_OK;
}

template <bool IP, int L>
int32_t launch_lists_masked_nv(int nvb, const ListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    switch (nvb) {
    case 4: return launch_lists_masked<IP, 4, L>(a, codes, lut, lds);
    case 8: return launch_lists_masked<IP, 8, L>(a, codes, lut, lds);
    case 13: return launch_lists_masked<IP, 13, L>(a, codes, lut, lds);
    case kAdcMaxValueWords: return launch_lists_masked<IP, kAdcMaxValueWords, L>(a, codes, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

template <bool IP>
int32_t launch_lists_masked_l(int L, int nvb, const ListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    switch (L) {
    case 1: return launch_lists_masked_nv<IP, 1>(nvb, a, codes, lut, lds);
    case 2: return launch_lists_masked_nv<IP, 2>(nvb, a, codes, lut, lds);
    case 4: return launch_lists_masked_nv<IP, 4>(nvb, a, codes, lut, lds);
    case 8: return launch_lists_masked_nv<IP, 8>(nvb, a, codes, lut, lds);
    case 16: return launch_lists_masked_nv<IP, 16>(nvb, a, codes, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

int32_t launch_lists_masked_u8(bool ip, int L, int nvb, const ListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    return ip ? launch_lists_masked_l<true>(L, nvb, a, codes, lut, lds) : launch_lists_masked_l<false>(L, nvb, a, codes, lut, lds);
}

}  // namespace pqh

using namespace pqh;

extern "C" {

// In all six: d_allow == NULL is the unmasked call itself.
static RowMask row_mask(const uint32_t* d_allow) { return RowMask{d_allow, launch_search_masked_u8, launch_lists_masked_u8}; }

int32_t pqhip_adc_search_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                        int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t k,
                                        float* d_dist, int64_t d_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!d_allow) return pqhip_adc_search_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, k, d_dist, d_rs, d_idx, i_rs, stream);
    return adc_search_masked(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream,
                             row_mask(d_allow));
}

int32_t pqhip_adc_ip_search_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                           const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                           const uint32_t* d_allow, const float* d_scales, int32_t k, float* d_score,
                                           int64_t s_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!d_allow)
        return pqhip_adc_ip_search_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
    return adc_search_masked(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream,
                             row_mask(d_allow));
}

int32_t pqhip_adc_search_lists_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                              const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                              const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                              const int64_t* d_probes, int32_t n_probe, int64_t p_rs, int32_t k, float* d_dist,
                                              int64_t d_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!d_allow)
        return pqhip_adc_search_lists_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes,
                                              n_probe, p_rs, k, d_dist, d_rs, d_idx, i_rs, stream);
    return adc_search_lists_masked(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream, nullptr, row_mask(d_allow));
}

int32_t pqhip_adc_ip_search_lists_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                 const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                 const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                                 const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales,
                                                 int32_t k, float* d_score, int64_t s_rs, int64_t* d_idx, int64_t i_rs,
                                                 void* stream)
{
    if (!d_allow)
        return pqhip_adc_ip_search_lists_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes,
                                                 n_probe, p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
    return adc_search_lists_masked(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, nullptr, row_mask(d_allow));
}

int32_t pqhip_adc_search_lists_residual_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                       const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                       const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                                       const int64_t* d_probes, int32_t n_probe, int64_t p_rs,
                                                       const float* d_probe_bias, int64_t b_rs, const float* d_row_terms,
                                                       int32_t k, float* d_dist, int64_t d_rs, int64_t* d_idx, int64_t i_rs,
                                                       void* stream)
{
    if (!d_allow)
        return pqhip_adc_search_lists_residual_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists,
                                                       d_probes, n_probe, p_rs, d_probe_bias, b_rs, d_row_terms, k, d_dist, d_rs,
                                                       d_idx, i_rs, stream);
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_masked(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, d_row_terms, k, d_dist, d_rs, d_idx, i_rs, stream, &res, row_mask(d_allow));
}

int32_t pqhip_adc_ip_search_lists_residual_masked_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                          const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                          const uint32_t* d_allow, const int64_t* d_list_off, int64_t n_lists,
                                                          const int64_t* d_probes, int32_t n_probe, int64_t p_rs,
                                                          const float* d_probe_bias, int64_t b_rs, const float* d_scales,
                                                          int32_t k, float* d_score, int64_t s_rs, int64_t* d_idx,
                                                          int64_t i_rs, void* stream)
{
    if (!d_allow)
        return pqhip_adc_ip_search_lists_residual_f32_dev(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists,
                                                          d_probes, n_probe, p_rs, d_probe_bias, b_rs, d_scales, k, d_score, s_rs,
                                                          d_idx, i_rs, stream);
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_masked(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, &res, row_mask(d_allow));
}

int32_t pqhip_pack_row_mask_dev(pqhip_codebook* cb, int32_t slot, const uint8_t* d_allow_bytes, int64_t n_src,
                                const int64_t* d_perm, int64_t n, uint32_t* d_words, void* stream)
{
    if (!cb || n < 0 || n_src < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (n > ((int64_t)0x7fffffff << 8)) return PQHIP_EUNSUPPORTED;      // one launch: 256 positions per workgroup
    if (n == 0) return PQHIP_OK;
    if (!d_words || !d_allow_bytes) return PQHIP_EINVAL;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    hipLaunchKernelGGL(k_pack_row_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_allow_bytes, n_src, d_perm, n,
                       d_words, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_pack_row_mask");
    return PQHIP_OK;
}

}  // extern "C"
