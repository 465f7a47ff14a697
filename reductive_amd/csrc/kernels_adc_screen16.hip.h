// kernels_adc_screen16.hip.h -- the conservative range screen of kernels_adc_screen.hip.h with a 16-BIT table image
// (include/pqhip.h: pqhip_adc_screen16_f32_dev; DESIGN.md §5g has what changes in the bound of §5e and why its proof
// survives).  Same contract, same output, a finer image: a returned regular row lies at most M s beyond the threshold
// with s = num / (L - 1), L = floor(65,535 / M) levels per entry instead of 255 -- 3.5 % of thr' - base at M = 48 where
// the u8 image allows 19 %.  (Instantiated by pqhip_adc_screen16.hip.)
//
// The level count is chosen so that the sums need no second accumulator: every entry is at most L, so a row's sum
// U = sum_m u[m][code m] <= M L <= 65,535 fits the 16 bits it is summed in.  Preparation is adc_screen_prep_slot with
// the entry type uint16_t and `levels` = L: the same lo_m, base, E, num, B, s32 and thresholds, the step num / (L - 1),
// the saturation value L, U_lim = min(65,535, floor(num / s (1 + kAdcScreenF64))).  The epilogue of the scaled form
// (adc_screen_keep) takes U as it is: (float)U is exact up to 2^24.
//
// Kernel.  The image of a pass sits in LDS as [M][K][NQ] u16, interleaved by query, so the entries of a code for 8
// queries are 16 consecutive bytes: one ds_read_b128 (two for NQ = 16, one ds_read_b64 for NQ = 4).  A fetched dword
// holds the entries of queries 2j and 2j + 1, and the accumulator dword j their sums: ONE packed add (v_pk_add_u16) per
// fetched dword, half an instruction per (row, query, subquantizer), and after the last m the low and high halves of
// dword j ARE the sums of queries 2j and 2j + 1 -- nothing is unpacked, nothing carries from the low half into the high
// one because no low half exceeds 65,535.  Two bytes per entry halve the queries per stream of the codes against the u8
// image: NQ = 16, 8 or 4, the most whose image and parameters fit the 160 KB.
// Units, order, passes, row fetch, allow bits, predicate, ballots, hit words and counts are those of k_adc_screen_u8, so
// the scan (k_adc_range_scan) and the fill (k_adc_screen_fill) are that kernel's.
#pragma once
#include "kernels_adc_screen.hip.h"

namespace pqhip {

// levels per entry of the 16-bit image: the largest L with M L <= 65,535
constexpr int adc_screen16_levels(int M) { return 65535 / M; }
constexpr bool adc_screen16_sums_fit()
{
    for (int m = 1; m <= kAdcScreenMaxM; ++m)
        if (m * adc_screen16_levels(m) > 65535) return false;
    return true;
}
static_assert(adc_screen16_sums_fit(), "M L <= 65,535 for every M <= kAdcScreenMaxM: the packed u16 sums never wrap");

constexpr size_t adc_screen16_image_bytes(int M, int K, int nq) { return ((size_t)M * K * nq * 2 + 15) / 16 * 16; }
constexpr size_t adc_screen16_lds_bytes(int M, int K, int nq) { return adc_screen16_image_bytes(M, K, nq) + (size_t)nq * sizeof(AdcScreenPrm); }

// One query slot per workgroup, into the image of a pass: img [M][K][NQ] u16, interleaved by query, prm [NQ]; slots
// >= nq_pass are padding.
inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_prep16(const float* __restrict__ tables, int nq_pass, int M, int K, int NQ,
                                                                      const float* __restrict__ thr, int ip, int scaled,
                                                                      const unsigned* __restrict__ cmax_bits,
                                                                      uint16_t* __restrict__ img, AdcScreenPrm* __restrict__ prm)
{
    const int slot = blockIdx.x;
    adc_screen_prep_slot(tables + (size_t)slot * M * K, slot < nq_pass, M, K, thr + slot, ip, scaled, cmax_bits, adc_screen16_levels(M),
                         img + slot, (size_t)NQ, prm + slot);
}

// the u16 entries of one code for 2 ND query slots, ND dwords from a 4 ND-byte aligned LDS address
template <int ND>
__device__ __forceinline__ void adc_screen16_entry(const uint8_t* p, unsigned (&d)[ND])
{
    static_assert(ND == 2 || ND == 4 || ND == 8, "dwords per entry fetch");
    if constexpr (ND == 2) {
        const as_u32x2 a = *reinterpret_cast<const as_u32x2*>(p);
        d[0] = a[0]; d[1] = a[1];
    } else {
#pragma unroll
        for (int h = 0; h < ND / 4; ++h) {
            const as_u32x4 a = *reinterpret_cast<const as_u32x4*>(p + 16 * h);
            d[4 * h] = a[0]; d[4 * h + 1] = a[1]; d[4 * h + 2] = a[2]; d[4 * h + 3] = a[3];
        }
    }
}

// The integer sums of one row (fetched by adc_fetch_row, shift sh = a & 3) against the interleaved image lm [M][K][2 ND]
// u16 in LDS, KQB = 4 ND K bytes per subquantizer: acc[j] = the packed sums of query slots 2j (low half) and 2j + 1 (high
// half).  A code >= K sets `bad` and reads entry 0.
template <int NV, int ND>
__device__ __forceinline__ void adc_screen16_row_sums(const unsigned (&w)[NV + 1], unsigned sh, const uint8_t* lm, int M, int K, int KQB,
                                                      bool& bad, unsigned (&acc)[ND])
{
    as_u16x2 a[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) a[j] = (as_u16x2){0, 0};
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);   // bytes 4k .. 4k+3 of the row
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * k + e < M) {
                unsigned c = (v >> (8 * e)) & 0xffu;
                if (c >= (unsigned)K) { bad = true; c = 0; }
                unsigned d[ND];
                adc_screen16_entry<ND>(lm + c * (4 * ND), d);
#pragma unroll
                for (int j = 0; j < ND; ++j) a[j] += __builtin_bit_cast(as_u16x2, d[j]);
                lm += KQB;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) acc[j] = __builtin_bit_cast(unsigned, a[j]);
}

// The count pass, NQ query slots per pass: the decomposition, arguments and outputs of k_adc_screen_u8 (see there);
// img is the pass's u16 image with its parameters behind (16-byte aligned).
template <int NV, int NQ>
__global__ __launch_bounds__(1024) void k_adc_screen_u16(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                         const uint32_t* __restrict__ allow /* or null */,
                                                         const float* __restrict__ scales /* [n] or null */,
                                                         const uint8_t* __restrict__ img, int M, int K, int64_t rows_per_wg,
                                                         int nq_pass, int64_t words, int64_t* __restrict__ part,
                                                         unsigned long long* __restrict__ hits, int* __restrict__ err)
{
    static_assert(NQ == 4 || NQ == 8 || NQ == 16, "query slots per pass");
    constexpr int NW = NV + 1, ND = NQ / 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_u[];
    const int img_bytes = (int)adc_screen16_image_bytes(M, K, NQ);
    {
        const int chunks = (img_bytes + NQ * (int)sizeof(AdcScreenPrm)) / 16;
        const as_u32x4* src = reinterpret_cast<const as_u32x4*>(img);
        as_u32x4* dst = reinterpret_cast<as_u32x4*>(lds_u);
        for (int c = threadIdx.x; c < chunks; c += 1024) dst[c] = src[c];
    }
    __syncthreads();
    const AdcScreenPrm* prm = reinterpret_cast<const AdcScreenPrm*>(lds_u + img_bytes);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t sub = rows_per_wg / kRangeWaves;                  // a multiple of 64
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    const int KQB = K * NQ * 2;
    int64_t cnt = 0;                                                // lane q < nq_pass: the unit's hits of query q
    bool bad = false;
    for (int64_t b0 = row_begin; b0 < row_end; b0 += 64) {          // wave-uniform: the ballots are wave-wide
        const int64_t row = b0 + lane;
        bool valid = row < row_end;
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        unsigned acc[ND];                                           // dword j: the sums of slots 2j (low) and 2j + 1 (high)
#pragma unroll
        for (int j = 0; j < ND; ++j) acc[j] = 0u;
        float sc = 1.f;
        if (valid) {
            if (scales) sc = scales[row];                           // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            adc_screen16_row_sums<NV, ND>(w, (unsigned)(a & 3), lds_u, M, K, KQB, bad, acc);
        }
        unsigned long long mine = 0ull;                             // lane q: the hit word of query q
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int U = (int)((q & 1) ? acc[q >> 1] >> 16 : acc[q >> 1] & 0xffffu);
            const bool keep = adc_screen_keep(U, prm[q], sc);
            const unsigned long long bl = __ballot(valid && keep && q < nq_pass);
            if (lane == q) mine = bl;
        }
        if (lane < NQ) {
            hits[(int64_t)lane * words + (b0 >> 6)] = mine;
            cnt += (int64_t)__popcll(mine);
        }
    }
    if (lane < nq_pass) part[(int64_t)lane * units + unit] = cnt;
    if (bad) atomicOr(err, 1);
}

}  // namespace pqhip
