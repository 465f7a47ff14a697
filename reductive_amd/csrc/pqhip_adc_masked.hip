// pqhip_adc_masked.hip -- the ADC searches restricted to an allowed set of rows (include/pqhip.h:
// pqhip_adc_*search*_masked_f32_dev, pqhip_pack_row_mask_dev).  The policy of a search is pqhip_adc.hip's, the same
// routines with the mask as one more field (adc_search_launch.h); this unit holds the entry points, the instantiations
// of the u8 producers with their MASKED flag (through the launchers of adc_search_u8_launch.hip.h), and packs a mask.
// A unit of its own so that the build compiles it beside pqhip_adc.hip; nothing in pqhip_adc.hip refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_u8_launch.hip.h"
#include "kernels_adc_search_masked.hip.h"

using namespace pqhip;

using namespace pqh;

extern "C" {

// In all six: d_allow == NULL is the unmasked call itself.
static RowMask row_mask(const uint32_t* d_allow) { return RowMask{d_allow, launch_search_u8<true>, launch_lists_u8<true>}; }

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
