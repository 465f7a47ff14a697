// smallk_launch.hip -- compiled once per PQ_KP by the Makefile: k_encode_smallk<PQ_KP, dsub> for the dsub of smallk_has().
#include "smallk_launch.h"

#ifndef PQ_KP
#error "PQ_KP must be defined"
#endif

namespace pqhip {

template <int KP>
int32_t launch_smallk_t(int dsub, const SmallKArgs& a, dim3 grid, hipStream_t st)
{
    // candidates: every even sub-vector length up to 32 floats
    return pqh::dispatch_int<2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32>(dsub, [&](auto d_c) -> int32_t {
        constexpr int D = decltype(d_c)::value;
        if constexpr (smallk_has(D)) {
            hipLaunchKernelGGL((k_encode_smallk<KP, D>), grid, dim3(256), 0, st, a);
            return PQHIP_OK;
        } else {
            return PQHIP_EUNSUPPORTED;
        }
    });
}

template int32_t launch_smallk_t<PQ_KP>(int, const SmallKArgs&, dim3, hipStream_t);

}  // namespace pqhip
