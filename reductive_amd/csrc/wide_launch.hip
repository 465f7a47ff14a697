// wide_launch.hip -- instantiations of k_encode_mfma_wide / k_encode_mfma_wide2 (kernels_mfma_wide.hip.h): the (T, DP) for
// which wide_has() (wide_launch.h) holds.
#include "wide_launch.h"
#include <algorithm>
#include "kernels_mfma_wide.hip.h"
#include "launch_dispatch.h"

namespace pqhip {

template <int T, int DP>
static int32_t launch_one(const EncodeArgs& a, const float* xx, dim3 grid, hipStream_t st)
{
    if constexpr (!wide_has(T, DP)) {
        return PQHIP_EUNSUPPORTED;
    } else {
        const size_t lds = ((size_t)T * (DP / 2) * 64 + (size_t)T * 32) * sizeof(float);
        // beyond 256 floats: several rule-2 blocks per dot product (wide_geometry)
        if constexpr (DP > 256) {
            if (hipFuncSetAttribute((const void*)k_encode_mfma_wide2<T, DP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return PQHIP_EHIP;
            hipLaunchKernelGGL((k_encode_mfma_wide2<T, DP>), grid, dim3(256), lds, st, a, xx);
        } else {
            if (hipFuncSetAttribute((const void*)k_encode_mfma_wide<T, DP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return PQHIP_EHIP;
            hipLaunchKernelGGL((k_encode_mfma_wide<T, DP>), grid, dim3(256), lds, st, a, xx);
        }
        return PQHIP_OK;
    }
}

int32_t launch_encode_wide(int T, int DP, const EncodeArgs& a, const float* xx, dim3 grid, hipStream_t st)
{
    // candidates: every multiple of 16 from 144 to 256, every multiple of 64 from 320 to 1,024
    return pqh::dispatch_int<1, 2, 4>(T, [&](auto t_c) {
        return pqh::dispatch_int<144, 160, 176, 192, 208, 224, 240, 256, 320, 384, 448, 512, 576, 640, 704, 768, 832, 896, 960, 1024>(
            DP, [&](auto dp_c) { return launch_one<decltype(t_c)::value, decltype(dp_c)::value>(a, xx, grid, st); });
    });
}

void launch_row_norms(const float* x, int64_t n, int64_t x_rs, int M, int dsub, float* xx, hipStream_t st)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n * M * 8 + 255) / 256, 256 * 64);   // eight lanes per (row, m)
    hipLaunchKernelGGL(k_row_norms, dim3(grid), dim3(256), 0, st, x, n, x_rs, M, dsub, xx);
}

}  // namespace pqhip
