// small16_launch.hip -- instantiations of k_encode_small16 (kernels_small16.hip.h): the (KP, dsub) for which small16_has()
// (small16_launch.h) holds.
#include "small16_launch.h"
#include "kernels_small16.hip.h"
#include "launch_dispatch.h"

namespace pqhip {

// WHOLE: M is a multiple of the subquantizers of a row block
template <int KP, int D, bool WHOLE>
static int32_t launch_one(const SmallKArgs& a, dim3 grid, size_t lds, hipStream_t st)
{
    if constexpr (!small16_has(KP, D)) {
        return PQHIP_EUNSUPPORTED;
    } else {
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void*)k_encode_small16<KP / 16, D, WHOLE>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) != hipSuccess)
            return PQHIP_EHIP;
        hipLaunchKernelGGL((k_encode_small16<KP / 16, D, WHOLE>), grid, dim3(256), lds, st, a);
        return PQHIP_OK;
    }
}

int32_t launch_small16(int KP, int dsub, const SmallKArgs& a, dim3 grid, size_t lds, hipStream_t st)
{
    // candidates: 16 / 32 centroids, every multiple of 4 floats up to 32
    return pqh::dispatch_int<16, 32>(KP, [&](auto kp_c) {
        return pqh::dispatch_int<4, 8, 12, 16, 20, 24, 28, 32>(dsub, [&](auto d_c) {
            constexpr int D = decltype(d_c)::value;
            return pqh::dispatch_int<0, 1>(a.M % (16 * small16_pieces_per_lane(D) / D) == 0, [&](auto whole_c) {
                return launch_one<decltype(kp_c)::value, D, decltype(whole_c)::value != 0>(a, grid, lds, st);
            });
        });
    });
}

}  // namespace pqhip
