// adc_key.hip.h -- the order of every search of the library as an unsigned key, and the values a key stands for.
// Shared by the ADC searches (kernels_adc_search.hip.h) and the exact re-ranking (kernels_rerank.hip.h), which live in
// different translation units; inline device functions only.
#pragma once
#include "common.hip.h"

namespace pqhip {

// the first-minimum order as an unsigned key: -0 -> +0, NaN above +Inf (all NaNs one key)
__device__ __forceinline__ unsigned adc_order_key(float f)
{
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the distance a key stands for (a sum from +0 is never -0; a NaN comes back as the canonical quiet NaN)
__device__ __forceinline__ float adc_key_value(unsigned key)
{
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// the score a similarity key stands for (the key is that of -score): a zero comes back as +0 (0 - (+0)), a NaN as the
// canonical quiet NaN, every other score bit for bit (0 - v = -v exactly)
__device__ __forceinline__ float adc_ip_key_score(unsigned key)
{
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return fsub(0.f, adc_key_value(key));
}

}  // namespace pqhip
