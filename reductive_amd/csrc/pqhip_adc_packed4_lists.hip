// pqhip_adc_packed4_lists.hip -- the list producers over 4-bit packed codes (kernels_adc_packed4.hip.h:
// k_adc_search_lists_p4) and their launcher.  The policy and the entry points are pqhip_adc_packed4.hip's; a unit of its
// own so that the build compiles these instantiations beside the exhaustive ones.
#include "adc_search_launch.h"

#define PQHIP_ADC_TEMPLATES_ONLY       // kernels_adc.hip.h: its non-template kernels belong to pqhip_adc.hip
#define PQHIP_PACKED4_PRODUCERS_ONLY   // kernels_adc_packed4.hip.h: k_unpack_codes4 belongs to pqhip_adc_packed4.hip
#include "kernels_adc_packed4.hip.h"

using namespace pqhip;

namespace pqh {

template <bool IP, int NV, int L>
int32_t launch_lists_p4(const ListsLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    HIPCHK(hipFuncSetAttribute((const void*)k_adc_search_lists_p4<IP, NV, L>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((k_adc_search_lists_p4<IP, NV, L>), dim3(a.G, a.nq), dim3(1024), lds, a.st, packed, a.n, a.c_rs, a.allow, lut,
                       a.bias, a.b_rs, a.scales, a.M, a.K, a.k, a.seg_begin, a.seg_cum, a.n_probe, a.part_k, a.part_i, a.err);
    if (a.bias) note_kernel(IP ? "k_adc_ip_search_lists_residual_p4" : "k_adc_search_lists_residual_p4");
    else note_kernel(IP ? "k_adc_ip_search_lists_p4" : "k_adc_search_lists_p4");
    return PQHIP_OK;
}

int32_t launch_lists_packed4(bool ip, int L, int nvb, const ListsLaunch& a, const void* packed, const float* lut, size_t lds)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_list_regs(L, [&](auto l_c) {
            return dispatch_int<2, 8, kPacked4MaxValueWords>(nvb, [&](auto nv_c) {
                return launch_lists_p4<decltype(ip_c)::value != 0, decltype(nv_c)::value, decltype(l_c)::value>(
                    a, (const uint8_t*)packed, lut, lds);
            });
        });
    });
}

}  // namespace pqh
