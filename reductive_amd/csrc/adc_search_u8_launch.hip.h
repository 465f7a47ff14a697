// adc_search_u8_launch.hip.h -- the launchers of the u8 search producers (kernels_adc_search.hip.h,
// kernels_adc_search_lists.hip.h), shared by the two units that instantiate them: pqhip_adc.hip the producers without a
// row mask (MASKED = false), pqhip_adc_masked.hip those with one.  Each has the signature the drivers take
// (adc_search_launch.h: SearchProducer, ListsProducer).
#pragma once
#include "adc_search_launch.h"
#include "kernels_adc_search_lists.hip.h"

namespace pqh {

template <bool IP, bool MASKED, int NV, int NQ, int L>
int32_t launch_search_u8_t(const SearchLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    if constexpr (NQ * L > 16) {   // a list of 64 L entries per query and wave: not instantiated beyond 32 list VGPRs
        return PQHIP_EUNSUPPORTED;
    } else {
        static const char* const names[2][2][3] = {
            {{"k_adc_search_u8", "k_adc_search_u8_mq<4 queries>", "k_adc_search_u8_mq<8 queries>"},
             {"k_adc_search_masked_u8", "k_adc_search_masked_u8_mq<4 queries>", "k_adc_search_masked_u8_mq<8 queries>"}},
            {{"k_adc_ip_search_u8", "k_adc_ip_search_u8_mq<4 queries>", "k_adc_ip_search_u8_mq<8 queries>"},
             {"k_adc_ip_search_masked_u8", "k_adc_ip_search_masked_u8_mq<4 queries>", "k_adc_ip_search_masked_u8_mq<8 queries>"}}};
        HIPCHK(hipFuncSetAttribute((const void*)pqhip::k_adc_search_u8<IP, MASKED, NV, NQ, L>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((pqhip::k_adc_search_u8<IP, MASKED, NV, NQ, L>), dim3(a.grid), dim3(1024), lds, a.st, codes, a.n, a.c_rs,
                           a.allow, lut, a.scales, a.M, a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
        note_kernel(names[IP][MASKED][NQ / 4]);
        return PQHIP_OK;
    }
}

template <bool MASKED>
int32_t launch_search_u8(bool ip, int nq_pass, int L, int nvb, const SearchLaunch& a, const void* codes, const float* lut, size_t lds)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_queries_per_pass(nq_pass, [&](auto nq_c) {
            return dispatch_list_regs(L, [&](auto l_c) {
                return dispatch_int<1, 2, 4, 8, 13, pqhip::kAdcMaxValueWords>(nvb, [&](auto nv_c) {
                    return launch_search_u8_t<decltype(ip_c)::value != 0, MASKED, decltype(nv_c)::value, decltype(nq_c)::value,
                                              decltype(l_c)::value>(a, (const uint8_t*)codes, lut, lds);
                });
            });
        });
    });
}

// a.bias != null: the residual producer
template <bool IP, bool RESIDUAL, bool MASKED, int NV, int L>
int32_t launch_lists_u8_t(const ListsLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    static const char* const names[2][2][2] = {
        {{"k_adc_search_lists_u8", "k_adc_search_lists_masked_u8"},
         {"k_adc_search_lists_residual_u8", "k_adc_search_lists_residual_masked_u8"}},
        {{"k_adc_ip_search_lists_u8", "k_adc_ip_search_lists_masked_u8"},
         {"k_adc_ip_search_lists_residual_u8", "k_adc_ip_search_lists_residual_masked_u8"}}};
    HIPCHK(hipFuncSetAttribute((const void*)pqhip::k_adc_search_lists_u8<IP, RESIDUAL, MASKED, NV, L>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((pqhip::k_adc_search_lists_u8<IP, RESIDUAL, MASKED, NV, L>), dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n,
                       a.c_rs, lut, a.scales, a.M, a.K, a.k, a.seg_begin, a.seg_cum, a.n_probe, a.part_k, a.part_i, a.err, a.bias,
                       a.b_rs, a.allow);
    note_kernel(names[IP][RESIDUAL][MASKED]);
    return PQHIP_OK;
}

template <bool MASKED>
int32_t launch_lists_u8(bool ip, int L, int nvb, const ListsLaunch& a, const void* codes, const float* lut, size_t lds)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_int<0, 1>(a.bias != nullptr, [&](auto res_c) {
            return dispatch_list_regs(L, [&](auto l_c) {
                return dispatch_int<4, 8, 13, pqhip::kAdcMaxValueWords>(nvb, [&](auto nv_c) {
                    return launch_lists_u8_t<decltype(ip_c)::value != 0, decltype(res_c)::value != 0, MASKED, decltype(nv_c)::value,
                                             decltype(l_c)::value>(a, (const uint8_t*)codes, lut, lds);
                });
            });
        });
    });
}

}  // namespace pqh
