// encode_launch.h -- host-side launchers of the MFMA encode kernels.  Each (KIND, T, DPSET) triple is instantiated in its
// own translation unit (encode_launch.hip, compiled once per triple by the Makefile) so that the kernel instantiations
// build in parallel.  mfma_has() below is the one statement of which instantiations exist.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_mfma.hip.h"
#include "launch_dispatch.h"

namespace pqhip {
// KIND 0: k_encode_mfma (VALU argmin epilogue); KIND 2: k_encode_mfma_lds3 (LDS-atomic argmin, A fragments in LDS,
// 3 waves/SIMD); KIND 3: k_encode_mfma16 (same epilogue on the 16x16x4 matrix instruction, 4 waves/SIMD).
// true when launch_encode_mfma has an instantiation for (kind, T, DP, vec, code_bytes); code_bytes 4: u32 codes (k-means
// assignment step / wide index types), 8: the 64-bit keys of grouped codebooks (KIND 2, T = 8).  KIND 3 also needs
// rows_per_item <= 32 * kMfma16MaxTiles.
constexpr bool mfma_has(int kind, int T, int DP, bool vec, int code_bytes)
{
    if (T != 1 && T != 2 && T != 4 && T != 8) return false;
    const bool codes = code_bytes == 1 || code_bytes == 4 || (code_bytes == 8 && kind == 2 && T == 8);
    if (DP > 32)
        return kind == 2 && codes && (DP == 40 || DP == 48 || DP == 56 || DP == 64 || DP == 80 || DP == 96 || DP == 112 || DP == 128);
    if (DP < 2 || DP % 2 != 0) return false;
    if (kind == 0) return code_bytes == 1;
    if (kind == 2) return codes;
    return kind == 3 && T >= 2 && DP % 4 == 0 && vec && (code_bytes == 1 || code_bytes == 4);
}
// The translation unit of a padded sub-dimension: DPSET 0: DP = 0 (mod 4), 1: DP = 2 (mod 4), 2: wide sub-vectors, DP > 32.
// A unit exists where mfma_has() holds for the first DP of its set.
constexpr int mfma_dpset(int DP) { return DP > 32 ? 2 : DP % 4 == 0 ? 0 : 1; }
constexpr bool mfma_has_unit(int kind, int T, int dpset) { return mfma_has(kind, T, dpset == 0 ? 4 : dpset == 1 ? 2 : 40, true, 1); }

// PQHIP_EUNSUPPORTED: no instantiation for (DP, vec, code_bytes)
template <int KIND, int T, int DPSET>
int32_t launch_encode_mfma_t(int DP, bool vec, int code_bytes, const EncodeArgs& a, dim3 grid, hipStream_t st, unsigned lds_pad);

#define PQHIP_DECL_LAUNCH(KIND, T)                                                                              \
    extern template int32_t launch_encode_mfma_t<KIND, T, 0>(int, bool, int, const EncodeArgs&, dim3, hipStream_t, unsigned); \
    extern template int32_t launch_encode_mfma_t<KIND, T, 1>(int, bool, int, const EncodeArgs&, dim3, hipStream_t, unsigned);
#define PQHIP_DECL_WIDE(T) \
    extern template int32_t launch_encode_mfma_t<2, T, 2>(int, bool, int, const EncodeArgs&, dim3, hipStream_t, unsigned);
PQHIP_DECL_WIDE(1) PQHIP_DECL_WIDE(2) PQHIP_DECL_WIDE(4) PQHIP_DECL_WIDE(8)
#undef PQHIP_DECL_WIDE
#define PQHIP_DECL_16(T) \
    extern template int32_t launch_encode_mfma_t<3, T, 0>(int, bool, int, const EncodeArgs&, dim3, hipStream_t, unsigned);
PQHIP_DECL_16(2) PQHIP_DECL_16(4) PQHIP_DECL_16(8)
#undef PQHIP_DECL_16
PQHIP_DECL_LAUNCH(0, 1) PQHIP_DECL_LAUNCH(0, 2) PQHIP_DECL_LAUNCH(0, 4) PQHIP_DECL_LAUNCH(0, 8)
PQHIP_DECL_LAUNCH(2, 1) PQHIP_DECL_LAUNCH(2, 2) PQHIP_DECL_LAUNCH(2, 4) PQHIP_DECL_LAUNCH(2, 8)
#undef PQHIP_DECL_LAUNCH

// lds_pad: extra dynamic LDS per workgroup (occupancy experiments of diagnostic builds; 0 in the default build)
inline int32_t launch_encode_mfma(int kind, int T, int DP, bool vec, int code_bytes, const EncodeArgs& a,
                                  dim3 grid, hipStream_t st, unsigned lds_pad = 0)
{
    return pqh::dispatch_int<0, 2, 3>(kind, [&](auto kind_c) {
        return pqh::dispatch_int<1, 2, 4, 8>(T, [&](auto t_c) {
            return pqh::dispatch_int<0, 1, 2>(mfma_dpset(DP), [&](auto set_c) -> int32_t {
                constexpr int KIND = decltype(kind_c)::value, TT = decltype(t_c)::value, DPSET = decltype(set_c)::value;
                if constexpr (mfma_has_unit(KIND, TT, DPSET))
                    return launch_encode_mfma_t<KIND, TT, DPSET>(DP, vec, code_bytes, a, grid, st, lds_pad);
                else
                    return PQHIP_EUNSUPPORTED;
            });
        });
    });
}
}  // namespace pqhip
