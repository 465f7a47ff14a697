// kernels_adc_screen_packed4.hip.h -- the u8 table screen of kernels_adc_screen.hip.h over 4-BIT PACKED rows, as a matrix
// product on the i8 matrix cores (include/pqhip.h: pqhip_adc_screen_packed4_f32_dev).  (Instantiated by
// pqhip_adc_screen_packed4.hip.)
//
// Definition.  For K <= 16 the integer sum of a row is a matrix product,
//     U[row][q] = sum_m u[q][m][code(row, m)] = onehot(row) . IMG[q],
// onehot(row) the 0/1 vector of 16 M entries that a packed row is the compressed form of.  The image u and the
// parameters of a query are those of the u8 screen (adc_screen_prep_slot<uint8_t>), the predicate is adc_screen_keep, the
// units, part[query][unit] and hits[query][word of 64 rows] are those of k_adc_screen_u8 -- so k_adc_range_scan and
// k_adc_screen_fill follow unchanged and the call returns, bit for bit, what pqhip_adc_screen_f32_dev returns on the
// unpacked codes.  The sums are exact int32.
//
// Layout.  v_mfma_i32_32x32x32_i8 multiplies 32 rows x 32 k by 32 k x 32 queries: one instruction adds TWO subquantizers
// (16 codes each) for 32 x 32 (row, query) pairs.  Lane l of the A operand holds, for row l % 32, its 16 bytes of k-half
// l / 32: the one-hot of nibble l / 32 of packed byte j -- four dwords, dword c >> 2 = 1 << 8 (c & 3), the others 0.  One
// packed byte feeds both lane halves.  Lane l of the B operand holds, for query l % 32, the 16 image entries of
// subquantizer 2 j + l / 32.  The prep kernel writes the image of a pass in exactly that order,
//     [query block of 32][k-step j = 0 .. PB - 1][lane][16 bytes],        PB = ceil(M / 2),
// so staging is a straight copy and an operand is one ds_read_b128 per lane.  The one-hot of a k-step is built once per
// tile of 32 rows and used for every query block of the pass (1 or 2: up to 64 queries per stream of the codes).
//
// Signedness.  The instruction's bytes are signed and the image is 0 .. 255: an entry is stored as u - 128 and every
// accumulator starts at 128 M.  A row selects exactly one entry per real subquantizer, so the sum is
// 128 M + sum_m (u_m - 128) = U, exactly.  The 16 entries of the pad subquantizer of an odd M are 0 (whatever the pad
// nibble holds it adds nothing); the entries k >= K of a real subquantizer are -128, i.e. u = 0: a nibble >= K can only
// make its row more likely to be returned, and it raises the range flag when the row is allowed.
//
// Epilogue.  Accumulator r of lane l is query l % 32 and row 8 (r / 4) + 4 (l / 32) + r % 4 of the tile: the query's
// parameters sit in one register each, lanes l and l + 32 hold complementary rows of one query and join their 16 bits each
// by one cross-lane move; lane l < 32 alone stores the 32-bit half of query l's hit word -- plain vector stores, no atomics
// -- and adds its popcount to the unit's count of that query.  A disallowed row and a row past n are never loaded: their
// one-hot is built from zeros and their bits are cleared by the ballot of the valid lanes.
#pragma once
#include "kernels_adc_screen.hip.h"

namespace pqhip {

typedef int p4s_i32x4 __attribute__((ext_vector_type(4)));
typedef int p4s_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kP4ScreenMaxBlocks = 2;            // query blocks of 32 per pass: 32 accumulators; four blocks spill, and two at NV = 13

constexpr size_t p4_screen_image_bytes(int M, int blocks) { return (size_t)blocks * ((M + 1) / 2) * 1024; }
constexpr size_t p4_screen_lds_bytes(int M, int blocks) { return p4_screen_image_bytes(M, blocks) + (size_t)blocks * 32 * sizeof(AdcScreenPrm); }

// One query slot per workgroup, into the image of a pass in B-operand order; slots >= nq_pass are padding.  The u8 image
// of the slot is adc_screen_prep_slot's, left in LDS and moved to its place with the bias of -128.
inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_p4_prep(const float* __restrict__ tables, int nq_pass, int M, int K,
                                                                       const float* __restrict__ thr, int ip, int scaled,
                                                                       const unsigned* __restrict__ cmax_bits,
                                                                       int8_t* __restrict__ img, AdcScreenPrm* __restrict__ prm)
{
    __shared__ uint8_t s_u[kAdcScreenMaxM * 16];
    const int slot = blockIdx.x;
    adc_screen_prep_slot<uint8_t>(tables + (size_t)slot * M * K, slot < nq_pass, M, K, thr + slot, ip, scaled, cmax_bits,
                                  kAdcScreenSteps + 1, s_u, (size_t)1, prm + slot);
    __syncthreads();
    const int PB = (M + 1) >> 1;
    int8_t* dst = img + ((size_t)(slot >> 5) * PB * 64 + (slot & 31)) * 16;
    for (int i = threadIdx.x; i < PB * 32; i += kAsPrepThreads) {
        const int m = i >> 4, k = i & 15;
        const int v = m < M ? (k < K ? (int)s_u[m * K + k] : 0) - 128 : 0;
        dst[((size_t)(m >> 1) * 64 + (m & 1) * 32) * 16 + k] = (int8_t)v;
    }
}

// The count pass, QB query blocks of 32 slots per pass; NV packed dwords per row (>= ceil(PB / 4)).  Rows, units and
// outputs as k_adc_screen_u8: workgroup b owns rows [b rows_per_wg, (b + 1) rows_per_wg), its wave w the sub-range
// [w rows_per_wg / 16, (w + 1) rows_per_wg / 16) (a multiple of 64): unit u = 16 b + w, two tiles of 32 rows per hit
// word.  img: the pass's image and parameters (16-byte aligned).  part [nq_pass][units] and hits [32 QB][words] out;
// every word of the unit's rows is written.  scales null: no epilogue.
template <int NV, int QB>
__global__ __launch_bounds__(1024) void k_adc_screen_p4(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                        const uint32_t* __restrict__ allow /* or null */,
                                                        const float* __restrict__ scales /* [n] or null */,
                                                        const uint8_t* __restrict__ img, int M, int K, int64_t rows_per_wg,
                                                        int nq_pass, int64_t words, int64_t* __restrict__ part,
                                                        unsigned long long* __restrict__ hits, int* __restrict__ err)
{
    static_assert(QB >= 1 && QB <= kP4ScreenMaxBlocks, "query blocks per pass");
    constexpr int NW = NV + 1;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_p[];
    const int PB = (M + 1) >> 1;
    const int img_bytes = (int)p4_screen_image_bytes(M, QB);
    {
        const int chunks = (int)(p4_screen_lds_bytes(M, QB) / 16);
        const as_u32x4* src = reinterpret_cast<const as_u32x4*>(img);
        as_u32x4* dst = reinterpret_cast<as_u32x4*>(lds_p);
        for (int c = threadIdx.x; c < chunks; c += 1024) dst[c] = src[c];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t sub = rows_per_wg / kRangeWaves;                  // a multiple of 64
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + PB);     // one past the last code byte
    const bool full = K == 16;
    const int step_bytes = PB * 1024;                               // one query block's image
    const uint8_t* lb = lds_p + lane * 16;                          // this lane's B operand of k-step 0, block 0
    unsigned* hw = reinterpret_cast<unsigned*>(hits) + (int64_t)l32 * words * 2;   // query l32's 32-bit halves of the hit words (little-endian)
    const int64_t hblock = 64 * words;                              // halves of one query block
    int64_t cnt[QB];                                                // lane l < 32: the unit's hits of query 32 qb + l
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) cnt[qb] = 0;
    bool bad = false;
    for (int64_t tb = row_begin; tb < ((row_end + 63) & ~(int64_t)63); tb += 32) {   // wave-uniform; both halves of a word
        const int64_t row = tb + l32;
        bool valid = row < row_end;
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        const unsigned vmask = (unsigned)__ballot(valid);           // bit i: row tb + i (both lane halves agree)
        const int64_t hword = (tb >> 6) * 2 + ((tb >> 5) & 1);
        if (vmask == 0u) {                                          // no row to screen: the half words are still written
            if (lane < 32) {
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) hw[qb * hblock + hword] = 0u;
            }
            continue;
        }
        unsigned w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0u;
        unsigned sh = 0u;
        float scm = 1.f;
        if (valid) {
            if (scales) scm = scales[row];                          // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            adc_fetch_row<NW>(a, lo, hi, PB, w);
            sh = (unsigned)(a & 3);
        }
        p4s_i32x16 acc[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qb][r] = 128 * M;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);   // bytes 4k .. 4k+3 of the row: k-steps 4k .. 4k+3
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * k + e;
                if (j < PB) {
                    const unsigned c = (v >> (8 * e + 4 * half)) & 0xfu;
                    if (!full) {
                        if (valid && c >= (unsigned)K && 2 * j + half < M) bad = true;   // the pad nibble is nobody's code
                    }
                    const unsigned bit = 1u << (8u * (c & 3u)), d = c >> 2;
                    const p4s_i32x4 onehot = {d == 0u ? (int)bit : 0, d == 1u ? (int)bit : 0, d == 2u ? (int)bit : 0, d == 3u ? (int)bit : 0};
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        const p4s_i32x4 b = *reinterpret_cast<const p4s_i32x4*>(lb + qb * step_bytes + j * 1024);
                        acc[qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(onehot, b, acc[qb], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);              // no operand of a later k-step is fetched ahead: the registers are the accumulators'
                }
            }
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const int q = qb * 32 + l32;
            int po = q * (int)sizeof(AdcScreenPrm);
            asm volatile("" : "+v"(po));                            // read per tile: four registers, not four per query block kept over the loop
            const AdcScreenPrm p = *reinterpret_cast<const AdcScreenPrm*>(lds_p + img_bytes + po);
            unsigned bits = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = 8 * (r >> 2) + (r & 3) + 4 * half;   // the accumulator's row of the tile
                const float sc = scales ? __shfl(scm, ri) : 1.f;    // lane ri < 32 holds row ri; 1 for a row not loaded
                if (adc_screen_keep(acc[qb][r], p, sc)) bits |= 1u << ri;
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four rows in flight: the other accumulators keep their registers
            }
            bits |= (unsigned)__shfl_xor((int)bits, 32);            // the complementary rows of the same query
            bits = q < nq_pass ? bits & vmask : 0u;
            if (lane < 32) {
                hw[qb * hblock + hword] = bits;
                cnt[qb] += (int64_t)__popc(bits);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (lane < 32) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
            if (qb * 32 + lane < nq_pass) part[(int64_t)(qb * 32 + lane) * units + unit] = cnt[qb];
    }
    if (bad) atomicOr(err, 1);
}

}  // namespace pqhip
