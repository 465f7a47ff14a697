// kernels_adc_search_masked.hip.h -- the kernel that packs a row mask.  (Launched from exactly one translation unit,
// pqhip_adc_masked.hip.)
//
// A mask is ceil(n / 32) words in the row order of the code matrix; bit i & 31 of word i >> 5 set means that row i may
// be returned.  The result of a masked search is the unmasked search's on the matrix with every row whose bit is clear
// removed, indices mapped back: the order (key, row) is strict, so leaving rows out of the selection is all a filter has
// to do.  The producers test the bit themselves (adc_mask_bit in kernels_adc.hip.h; the MASKED flag of k_adc_search_u8
// and k_adc_search_lists_u8, `allow` of the packed and range kernels); everything from offer on runs unchanged.
#pragma once
#include "common.hip.h"

namespace pqhip {

// Packs a mask: bit p = allow_bytes[perm ? perm[p] : p] != 0 for p < n, 0 for the tail of the last word.  A source index
// outside [0, n_src) gives bit 0 and raises *err.  One thread per position, 256 per workgroup; one ballot per wave, and
// lanes 0 and 32 store its two words (the second only where it exists).
__global__ __launch_bounds__(256) void k_pack_row_mask(const uint8_t* __restrict__ allow_bytes, int64_t n_src,
                                                       const int64_t* __restrict__ perm, int64_t n,
                                                       uint32_t* __restrict__ words, int* __restrict__ err)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool bit = false, bad = false;
    if (p < n) {
        const int64_t src = perm ? perm[p] : p;
        if (src >= 0 && src < n_src) bit = allow_bytes[src] != 0;
        else bad = true;
    }
    const unsigned long long b = __ballot(bit);
    const int64_t n_words = (n + 31) >> 5;
    const int64_t w = (p >> 5);                                     // lane 0: the wave's first word, lane 32: its second
    if ((lane & 31) == 0 && w < n_words) words[w] = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
    if (bad) atomicOr(err, 1);
}

}  // namespace pqhip
