// encode_launch.hip -- compiled once per (PQ_KIND, PQ_T, PQ_DPSET) by the Makefile: the kernels of one unit are the
// (DP, vec, code width) of its DPSET for which mfma_has() (encode_launch.h) holds.
#include "encode_launch.h"
#include "kernels_mfma_lds.hip.h"
#include "kernels_mfma16.hip.h"

#if !defined(PQ_KIND) || !defined(PQ_T) || !defined(PQ_DPSET)
#error "PQ_KIND, PQ_T and PQ_DPSET must be defined"
#endif

namespace pqhip {

template <int KIND, int T, int DP, bool VEC, int CB>
static int32_t launch_one(const EncodeArgs& a, dim3 grid, hipStream_t st, unsigned pad)
{
    if constexpr (!mfma_has(KIND, T, DP, VEC, CB)) {
        return PQHIP_EUNSUPPORTED;
    } else {
        using IdxT = std::conditional_t<CB == 1, uint8_t, std::conditional_t<CB == 4, uint32_t, unsigned long long>>;
        if constexpr (KIND == 3) {
            if (a.rows_per_item > 32 * kMfma16MaxTiles) return PQHIP_EUNSUPPORTED;
            hipLaunchKernelGGL((k_encode_mfma16<T, DP, IdxT>), grid, dim3(256), pad, st, a);
        } else if constexpr (KIND == 2) {
            hipLaunchKernelGGL((k_encode_mfma_lds3<T, DP, VEC, IdxT>), grid, dim3(256), pad, st, a);
        } else {
            hipLaunchKernelGGL((k_encode_mfma<T, DP, VEC, IdxT>), grid, dim3(256), pad, st, a);
        }
        return PQHIP_OK;
    }
}

template <int KIND, int T, int DPSET>
int32_t launch_encode_mfma_t(int DP, bool vec, int code_bytes, const EncodeArgs& a, dim3 grid, hipStream_t st, unsigned pad)
{
    // candidates: every even DP up to 32, every multiple of 8 up to 128; the u8 / u32 / key code widths
    return pqh::dispatch_int<2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120,
                             128>(DP, [&](auto dp_c) -> int32_t {
        constexpr int DPC = decltype(dp_c)::value;
        if constexpr (mfma_dpset(DPC) != DPSET) return PQHIP_EUNSUPPORTED;   // (another unit's)
        else
            return pqh::dispatch_int<0, 1>(vec, [&](auto vec_c) {
                return pqh::dispatch_int<1, 4, 8>(code_bytes, [&](auto cb_c) {
                    return launch_one<KIND, T, DPC, decltype(vec_c)::value != 0, decltype(cb_c)::value>(a, grid, st, pad);
                });
            });
    });
}

template int32_t launch_encode_mfma_t<PQ_KIND, PQ_T, PQ_DPSET>(int, bool, int, const EncodeArgs&, dim3, hipStream_t, unsigned);

}  // namespace pqhip
