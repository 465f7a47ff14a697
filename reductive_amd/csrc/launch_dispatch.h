// launch_dispatch.h -- from run-time values to an instantiated kernel, for every launcher of the library.  A launcher
// returns PQHIP_OK once its kernel is launched and PQHIP_EUNSUPPORTED when no instantiation serves the values.
#pragma once
#include "../../include/pqhip.h"

#include <type_traits>

namespace pqh {

// f(std::integral_constant<int, V>{}) for the V among Vs that equals v; PQHIP_EUNSUPPORTED when v is none of them.
// Vs is the list of candidate values.  Either every one of them is instantiated and the kernels that exist are the ones
// named at the call, or the leaf asks the family's constexpr predicate (`if constexpr (family_has(..))`, the one
// plan_encode() asks) and returns PQHIP_EUNSUPPORTED where it says no.
template <int... Vs, typename F>
int32_t dispatch_int(int v, F&& f)
{
    int32_t status = PQHIP_EUNSUPPORTED;
    (void)((v == Vs && (status = f(std::integral_constant<int, Vs>{}), true)) || ...);
    return status;
}

}  // namespace pqh
