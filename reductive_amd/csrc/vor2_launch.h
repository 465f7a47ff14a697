// vor2_launch.h -- host-side launcher of k_encode_vor2 (2-float sub-vectors, K <= 256, u8 codes); the kernel lives in its own
// translation unit, vor2_launch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pqhip {
struct Vor2Launch {
    const float* x; int64_t n, x_rs; uint8_t* out; int64_t o_rs;
    const float* cb; const float* cc; const uint32_t* tab; const uint32_t* off;
    int M, K, k_pad, dsub;
    uint32_t max_region_words;
    int n_cus;
};
// The kernel stages the tables, centroids and norms of whole subquantizers in LDS: one subquantizer's must fit 150 KB.  This
// depends on the handle only (codebook_create_impl settles it).
inline size_t vor2_lds_per_m(uint32_t max_region_words, int K) { return ((size_t)max_region_words + 4 + (size_t)K * 4) * 4; }
inline bool vor2_has_lds(uint32_t max_region_words, int K) { return vor2_lds_per_m(max_region_words, K) <= 150 * 1024; }
// ... and the launch's workgroups must fit a one-dimensional grid (2^31 - 1), which depends on the row count
bool vor2_has_grid(int M, int K, int dsub, uint32_t max_region_words, int64_t n, int n_cus);
// PQHIP_EUNSUPPORTED: no launch for the handle or the row count (vor2_has_lds / vor2_has_grid)
int32_t launch_vor2(const Vor2Launch& l, hipStream_t st);
}  // namespace pqhip
