// pqhip_adc_screen16.hip -- conservative range screen over resident u8 codes with 16-bit table images (include/pqhip.h:
// pqhip_adc_screen16_f32_dev): the entry point, the 16-bit image's side of the policy of adc_screen_launch.h (the one the
// u8 screen runs: checks, query slots per pass, grid, scratch, the prep / count / scan / fill sequence) and the
// instantiations of kernels_adc_screen16.hip.h.  A unit of its own so that the build compiles its kernels beside the other
// searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of kernels_adc.hip.h belong to pqhip_adc.hip
#include "adc_screen_launch.h"
#include "kernels_adc_screen16.hip.h"

namespace pqh {

struct AdcScreenU16 {
    static constexpr int kSlots[] = {16, 8, 4};
    static size_t image_bytes(int M, int K, int slots) { return adc_screen16_image_bytes(M, K, slots); }
    static size_t lds_bytes(int M, int K, int slots) { return adc_screen16_lds_bytes(M, K, slots); }
    static void prep(int slots, hipStream_t st, const float* tables, int nqp, int M, int K, const float* thr, int ip, int scaled,
                     const unsigned* cmax, uint8_t* img, AdcScreenPrm* prm)
    {
        hipLaunchKernelGGL(k_adc_screen_prep16, dim3(slots), dim3(kAsPrepThreads), 0, st, tables, nqp, M, K, slots, thr, ip, scaled, cmax,
                           (uint16_t*)img, prm);
        note_kernel("k_adc_screen_prep16");
    }
    static int32_t count(int nvb, int slots, const AdcScreenLaunch& a)
    {
        const int32_t status = dispatch_int<1, 2, 4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
            return dispatch_int<16, 8, 4>(slots, [&](auto nq_c) {
                constexpr int NV = decltype(nv_c)::value, NQ = decltype(nq_c)::value;
                return launch_adc_screen_kernel(k_adc_screen_u16<NV, NQ>, adc_screen16_lds_bytes(a.M, a.K, NQ), a);
            });
        });
        if (status != PQHIP_OK) return status;
        HIPCHK(hipGetLastError());
        note_kernel(slots == 16 ? "k_adc_screen_u16<16 queries>" : slots == 8 ? "k_adc_screen_u16<8 queries>" : "k_adc_screen_u16<4 queries>");
        return PQHIP_OK;
    }
};

}  // namespace pqh

extern "C" {

// the policy, grid (option "adc_screen_wgs") and scratch are adc_screen_run's (adc_screen_launch.h)
int32_t pqhip_adc_screen16_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                   int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t ip,
                                   const float* d_scales, const float* d_thr, int64_t* d_lims, int64_t* d_idx, int64_t capacity,
                                   void* stream)
{
    return pqh::adc_screen_run<pqh::AdcScreenU16>(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, ip, d_scales, d_thr,
                                                  d_lims, d_idx, capacity, stream);
}

}  // extern "C"
