// kernels_mfma16_screen.hip.h -- the body of k_encode_mfma16<8, 20, IdxT>: screen all 256 centroids on
// v_mfma_f32_16x16x32_bf16, then resolve the rows the screen cannot decide exactly.
//
// Screening value A(c, r) = cc(c) - 2 c.x(r), computed entirely in the accumulator by two bf16 matrix instructions per
// 16 x 16 block.  x and c are split into bf16 hi + lo parts (RNE), cc into hi + lo; along k:
//     A operand (centroid):  [-2 ch (20) | -2 cl (20) | -2 ch (20) | cc_hi | cc_lo | 0 0]
//     B operand (row):       [   xh (20) |    xh (20) |    xl (20) |   1   |   1   | 0 0]
// xx is the same for every centroid of a row and is left out.  |A(c) - (D(c) - xx)| <= E_r for every c, D the
// CANON-F32 distance, with E_r = kScreenRel / 2 * (xx + max cc) + kScreenAbs / 2 (the proof and its terms: DESIGN.md §5).
// The key of a value is its f32 bits with the low 6 mantissa bits replaced by the lane-local centroid number
// 4 cb + v (that moves a value by < 2^-17 |A|, part of the bound).  Per (lane, row block) the loop keeps the smallest
// key m and the second smallest s (v_min_f32 + v_med3_f32, three vector instructions per value); the four lane groups
// of a row are merged after the 16 centroid blocks.  When the second smallest key S of the row exceeds the smallest
// M by more than 2 E_r, the centroid of M is the first minimum of D and its code is stored: no FP32 arithmetic.
// When two to four keys are within that margin, one per lane group (every lane group's second key is above it), those
// lanes evaluate their candidate with the CANON-F32 operations and the row takes the first minimum of them, in the loop.
// Every other row -- more candidates, |M| tiny, huge / NaN norms, a bad codebook -- is recorded in need_s and
// re-evaluated after the loop by encode_rows_slow_v, as in the FP32 body.
//
// Layout (16x16x32 bf16): lane (i16, q) supplies A[i16][k = 8q .. 8q + 7] and B[k = 8q .. 8q + 7][i16] per 32-k
// half h and receives D[4q + v][i16].  A = 16 centroids (block cb), B = 16 rows (block rb).  The split codebook
// image (256 rows of 64 bf16 = 128 B, no padding) is built by the workgroup from cb / cc; chunk j (16 B) of row r is
// stored at chunk j ^ ((r >> 1) & 7), which puts the 16 lanes of every ds_read_b128 lane group on 16 different 16-B
// bank slots.  The B operand of a lane is two 8-element windows of its row's k layout,
// x[(8q + j) mod 20] and x[(12 + 8q + j) mod 20], loaded as four 4-float chunks and split in registers.
// Schedule: the 16 centroid blocks are software-pipelined -- block cb + 1's four matrix instructions are issued before
// the selection on block cb's accumulators, A fragments are read two blocks ahead, the next tile's rows are split
// into bf16 operands in the middle of the current tile, and its first block is issued before the lane-group merge.
#pragma once
#include "kernels_mfma.hip.h"

namespace pqhip {

// the screen's constants: accept a row when S > M + kScreenRel * (xx + max cc) + kScreenAbs
// and |M| > kScreenTiny
constexpr float kScreenRel = 0x1p-12f;    // >= 2 E_r + 2 key perturbation: (10.3 + 2.0) 2^-16 needed, 16 2^-16 taken
constexpr float kScreenAbs = 0x1p-100f;   // flushed subnormal products and operands
constexpr float kScreenTiny = 0x1p-100f;  // keeps the index bits of M out of the subnormal range

// instantiations that take the screen body (the others keep the FP32 body of k_encode_mfma16)
template <int T, int DP> constexpr bool mfma16_screens() { return mfma16_screen_shape(T, DP); }

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// two f32 -> packed bf16 pair, RNE, NaN stays NaN (v_cvt_pk_bf16_f32); a in the low half
__device__ __forceinline__ unsigned pk_bf16(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2_t));
}
__device__ __forceinline__ float bf16_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// plain v_min / v_max / v_med3: the operands are keys built with integer instructions, and the compiler would
// canonicalize them before fminf / fmaxf
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// two keys k1, k2 into the running (smallest m, second smallest s), m and s updated in place (tied operands, so the
// unrolled blocks need no register copies): the second smallest of {m, s, k1, k2} is min(s, med3(m, k1, k2)) when
// m <= s, and the smallest is min3(m, k1, k2) -- five instructions per two keys with the two that build them, against
// three per key one at a time.  The keys of a lane are distinct (index bits), and for the rows the screen decides they
// are finite, so m and s are exactly the two smallest keys either way.
__device__ __forceinline__ void keep2(float& m, float& s, float k1, float k2)
{
    float t;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(t) : "v"(m), "v"(k1), "v"(k2));
    asm("v_min_f32 %0, %0, %1" : "+v"(s) : "v"(t));
    asm("v_min3_f32 %0, %0, %1, %2" : "+v"(m) : "v"(k1), "v"(k2));
}

template <typename IdxT>
__device__ __forceinline__ void encode_mfma16_screen(const EncodeArgs& a)
{
    constexpr int DP = 20;
    constexpr int kRow = 64;  // bf16 per image row, eight 16-B chunks, chunk j of row r at j ^ ((r >> 1) & 7)
    __shared__ __attribute__((aligned(16))) unsigned short img_s[256 * kRow];
    __shared__ unsigned need_s[4][kMfma16MaxTiles];
    __shared__ unsigned maxcc_s;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16 = lane & 15;
    const int q = lane >> 4;

    // ---- workgroup -> (row group, m), as the FP32 body
    const int64_t b = blockIdx.x;
    const int xcd = (int)(b & 7);
    const int64_t qq = b >> 3;
    const int64_t g_local = qq / a.M;
    const int m = (int)(qq - g_local * a.M);
    const int64_t group = g_local * 8 + xcd;
    const bool wg_active = (g_local < a.chunks_per_xcd) && (group < a.n_chunks);

    const unsigned long long st_s0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
    if (wg_active && threadIdx.x == 0) maxcc_s = 0u;
    __syncthreads();
    if (wg_active) {
        // one thread per centroid: the split image row and the largest real ||c||^2 (bits order = value order for
        // cc >= +0; a NaN norm comes out above +inf)
        const int c = threadIdx.x;
        const float ccv = a.cc[(int64_t)m * a.k_pad + c];
        unsigned w[32];
        if (c < a.K) {
            const float* cp = a.cb + ((int64_t)m * a.K + c) * DP;
#pragma unroll
            for (int j = 0; j < DP / 2; ++j) {
                const float c0 = cp[2 * j], c1 = cp[2 * j + 1];
                const unsigned h = pk_bf16(c0, c1);
                const float h0 = bf16_lo(h), h1 = bf16_hi(h);
                const unsigned l = pk_bf16(c0 - h0, c1 - h1);
                w[j] = pk_bf16(-2.f * h0, -2.f * h1);                  // exact
                w[DP / 2 + j] = pk_bf16(-2.f * bf16_lo(l), -2.f * bf16_hi(l));
                w[DP + j] = w[j];
            }
            const float cch = bf16_lo(pk_bf16(ccv, 0.f));
            w[30] = pk_bf16(cch, ccv - cch);
            atomicMax(&maxcc_s, __float_as_uint(ccv));
        } else {
            // padding centroid: A = the largest finite bf16, never a candidate
#pragma unroll
            for (int j = 0; j < 30; ++j) w[j] = 0u;
            w[30] = 0x7f7fu;
        }
        w[31] = 0u;
        u32x4_t* dst = reinterpret_cast<u32x4_t*>(&img_s[c * kRow]);
        const int swz = (c >> 1) & 7;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j ^ swz] = (u32x4_t){w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
    }
    __syncthreads();
    const unsigned long long st_stage = a.stamps ? __builtin_amdgcn_s_memtime() - st_s0 : 0;   // image staging
    const int64_t row_begin = (group * 4 + wave) * a.rows_per_item;
    if (!wg_active || row_begin >= a.n) return;
    int64_t row_end = row_begin + a.rows_per_item;
    if (row_end > a.n) row_end = a.n;
    const bool bad_codebook = a.bad_flag != nullptr && *a.bad_flag != 0;  // wave-uniform
    const float maxcc = __uint_as_float(maxcc_s);
    const bool cb_ok = !bad_codebook && maxcc < kBigNorm;                // wave-uniform

    // x windows of lane (i16, q): chunks of 4 floats starting at c0 .. c3 (c3 of q = 3 is loaded, then replaced by
    // the [1 1 0 0] tail)
    const int c0 = (8 * q) % 20, c1 = (8 * q + 4) % 20, c2 = (12 + 8 * q) % 20, c3 = (16 + 8 * q) % 20;
    const float* const xsub = a.x + (int64_t)m * a.dsub;
    const float* const plast = xsub + (a.n - 1) * a.x_rs;
    auto load_tile = [&](float (&v)[2][16], int64_t tile_row0) {
        const int left = (int)((a.n - tile_row0 < 32) ? a.n - tile_row0 : 32);  // wave-uniform
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const float* p = (16 * rb + i16 < left) ? xsub + (tile_row0 + 16 * rb + i16) * a.x_rs : plast;
            const f32x4 v0 = *reinterpret_cast<const f32x4_u*>(p + c0), v1 = *reinterpret_cast<const f32x4_u*>(p + c1);
            const f32x4 v2 = *reinterpret_cast<const f32x4_u*>(p + c2), v3 = *reinterpret_cast<const f32x4_u*>(p + c3);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[rb][j] = v0[j]; v[rb][4 + j] = v1[j]; v[rb][8 + j] = v2[j]; v[rb][12 + j] = v3[j]; }
        }
    };
    // window 0 is hi parts; window 1 is hi parts in lane group 0 (xh 12..19) and lo parts elsewhere
    const float rmask = q > 0 ? 1.f : 0.f;
    const bool tail = q == 3;
    auto split = [&](const float (&v)[2][16], u32x4_t (&bop)[2][2], float (&xx)[2]) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            unsigned w0[4], w1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w0[j] = pk_bf16(v[rb][2 * j], v[rb][2 * j + 1]);
                const float e0 = v[rb][8 + 2 * j], e1 = v[rb][9 + 2 * j];
                const unsigned h = pk_bf16(e0, e1);
                w1[j] = pk_bf16(fmaf(-rmask, bf16_lo(h), e0), fmaf(-rmask, bf16_hi(h), e1));  // x - xh is exact
            }
            if (tail) { w1[2] = 0x3f803f80u; w1[3] = 0u; }
            bop[rb][0] = (u32x4_t){w0[0], w0[1], w0[2], w0[3]};
            bop[rb][1] = (u32x4_t){w1[0], w1[1], w1[2], w1[3]};
            // ||x||^2 for the bound and the huge-norm test (not rule 1: any f32 sum will do): window 0 of lane
            // groups 0, 1 and the first half of group 2 cover the row once
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s0 = fmaf(v[rb][j], v[rb][j], s0); s1 = fmaf(v[rb][4 + j], v[rb][4 + j], s1); }
            const float own = (q < 3 ? s0 : 0.f) + (q < 2 ? s1 : 0.f);
            float u[4];
            gather_groups(own, u);
            xx[rb] = (u[0] + u[1]) + (u[2] + u[3]);
        }
    };

    const unsigned kKeyMask = 0xffffffc0u;
    unsigned long long flagged = 0;                                     // wave-uniform: tiles with rows for the exact path
    unsigned long long st_tiles = 0, st_steps = 0, st_rows = 0;   // st_rows: {exact-path rows, resolved rows}
    const unsigned long long st_t0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0, st_r0 = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    // A fragments of block cb: rows 16 cb + i16, chunks q and 4 + q (k = 8q .. 8q + 7 of each 32-k half), swizzled
    const int swz = (i16 >> 1) & 7;
    const unsigned short* const arow0 = &img_s[i16 * kRow + 8 * (q ^ swz)];
    const unsigned short* const arow1 = &img_s[i16 * kRow + 8 * ((4 + q) ^ swz)];
    auto load_a = [&](int cb, u32x4_t (&af)[2]) {
        af[0] = *reinterpret_cast<const u32x4_t*>(arow0 + cb * 16 * kRow);
        af[1] = *reinterpret_cast<const u32x4_t*>(arow1 + cb * 16 * kRow);
    };
    auto screen = [&](const u32x4_t (&af)[2], const u32x4_t (&bop)[2][2], f32x4 (&acc)[2]) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[0]), __builtin_bit_cast(bf16x8_t, bop[rb][0]),
                                                              (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[1]), __builtin_bit_cast(bf16x8_t, bop[rb][1]), acc[rb], 0, 0, 0);
        }
    };

    // prologue: the first tile's operands, A fragments of blocks 0 and 1, block 0
    float xv[2][16];
    u32x4_t bop[2][2];
    float xx[2];
    load_tile(xv, row_begin);
    split(xv, bop, xx);
    u32x4_t af[2][2];
    f32x4 acc[2][2];
    load_a(0, af[0]);
    load_a(1, af[1]);
    screen(af[0], bop, acc[0]);
    // one 32-row tile; bop / xx hold its split rows, bnext / xxn receive the next tile's.  The loop below alternates two
    // operand sets, so no operand is copied at the seam.
    auto tile = [&](int64_t row0, int tile_idx, const u32x4_t (&bop)[2][2], const float (&xx)[2], u32x4_t (&bnext)[2][2], float (&xxn)[2]) {
        const unsigned long long st_a = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
        // row0 stays a scalar: the per-lane row addresses are formed where they are used instead of being carried
        // from tile to tile in vector registers
        asm("" : "+s"(row0));
        // the next tile's rows (past row_end the loads are clamped like a short tile's, and their result is never used)
        load_tile(xv, row0 + 32);
        float mk[2] = {__builtin_inff(), __builtin_inff()}, sk[2] = {__builtin_inff(), __builtin_inff()};
        // step cb: issue block cb + 1, read the A fragments of block cb + 2 (mod 16: the next tile's blocks 0, 1),
        // then select on block cb
#pragma unroll
        for (int cb = 0; cb < 16; ++cb) {
            if (cb < 15) screen(af[(cb + 1) & 1], bop, acc[(cb + 1) & 1]);
            load_a((cb + 2) & 15, af[cb & 1]);
            if (cb == 8) split(xv, bnext, xxn);                          // the loads have landed by now
            auto key = [&](int rb, int v) { return __uint_as_float((__float_as_uint(acc[cb & 1][rb][v]) & kKeyMask) | (unsigned)(4 * cb + v)); };
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                keep2(mk[rb], sk[rb], key(rb, 0), key(rb, 1));
                keep2(mk[rb], sk[rb], key(rb, 2), key(rb, 3));
            }
        }
        // the next tile's block 0 runs under the merge
        screen(af[0], bnext, acc[0]);
        // ---- merge the four lane groups of each row; store the decided rows, resolve the few-candidate rows, record the
        // others
        unsigned need = 0, few_rows = 0;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            float mq[4], sq[4];
            gather_groups(mk[rb], mq);
            gather_groups(sk[rb], sq);
            const float lo01 = vmin(mq[0], mq[1]), hi01 = vmax(mq[0], mq[1]);
            const float lo23 = vmin(mq[2], mq[3]), hi23 = vmax(mq[2], mq[3]);
            const float M = vmin(lo01, lo23);
            const float S2 = vmin(vmin(sq[0], sq[1]), vmin(sq[2], sq[3]));   // smallest second key of a lane group
            const float S = vmin(vmin(vmax(lo01, lo23), vmin(hi01, hi23)), S2);
            const float tau = M + (kScreenRel * (xx[rb] + maxcc) + kScreenAbs);
            const int64_t row = row0 + 16 * rb + i16;
            const bool valid = row < a.n;
            const bool plain = valid && cb_ok && xx[rb] < kBigNorm && __builtin_fabsf(M) > kScreenTiny;
            const bool one = plain && S > tau;                           // a single candidate
            // two to four candidates, at most one per lane group (every lane group's second key is above tau): the
            // candidate set is exactly {m_q <= tau}; each such lane evaluates its centroid with the CANON-F32 operations
            // and the four lane groups take the first minimum of {ord_key(d), index}
            const bool few = plain && !one && S2 > tau;
            if (one && mk[rb] == M) {                                    // the one lane group that holds M
                const unsigned kb = __float_as_uint(M) & 63u;
                reinterpret_cast<IdxT*>(a.out)[row * a.o_rs + m] = (IdxT)(16 * (kb >> 2) + 4 * q + (kb & 3));
            }
            const unsigned few_b = (unsigned)__builtin_amdgcn_ballot_w64(q == 0 && few) & 0xffffu;
            if (few_b) {                                                 // wave-uniform
                unsigned kh = 0xffffffffu, kl = 0xffffffffu;
                if (few && mk[rb] <= tau) {
                    const unsigned kb = __float_as_uint(mk[rb]) & 63u;
                    const int j = 16 * (kb >> 2) + 4 * q + (kb & 3);
                    const float* xs = xsub + row * a.x_rs;
                    const float xxe = norm_unrolled_global(xs, DP);
                    const float dp = chain_dot_global(xs, 1, a.cb + ((int64_t)m * a.K + j) * DP, 1, DP);
                    kh = ord_key(fsub(fadd(xxe, a.cc[(int64_t)m * a.k_pad + j]), fadd(dp, dp)));
                    kl = (unsigned)j;
                }
                float hq[4], lq[4];
                gather_groups(__uint_as_float(kh), hq);
                gather_groups(__uint_as_float(kl), lq);
                unsigned bh = __float_as_uint(hq[0]), bl = __float_as_uint(lq[0]);
#pragma unroll
                for (int g = 1; g < 4; ++g) {
                    const unsigned h = __float_as_uint(hq[g]), l = __float_as_uint(lq[g]);
                    if (h < bh || (h == bh && l < bl)) { bh = h; bl = l; }
                }
                if (few && q == 0) reinterpret_cast<IdxT*>(a.out)[row * a.o_rs + m] = (IdxT)bl;
                few_rows |= few_b << (16 * rb);
            }
            need |= ((unsigned)__builtin_amdgcn_ballot_w64(q == 0 && valid && !one && !few) & 0xffffu) << (16 * rb);
        }
        if (need) {                                                     // wave-uniform
            if (lane == 0) need_s[wave][tile_idx] = need;
            flagged |= 1ull << tile_idx;
        }
        if (a.stamps) st_rows += (unsigned long long)__builtin_popcount(few_rows) | ((unsigned long long)__builtin_popcount(need) << 32);
        if (a.stamps) { st_tiles += 1; st_steps += __builtin_amdgcn_s_memtime() - st_a; }
    };
    u32x4_t bop2[2][2];
    float xx2[2];
    for (int64_t row0 = row_begin, tile_idx = 0;; row0 += 64, tile_idx += 2) {
        if (row0 >= row_end) break;
        tile(row0, (int)tile_idx, bop, xx, bop2, xx2);
        if (row0 + 32 >= row_end) break;
        tile(row0 + 32, (int)tile_idx + 1, bop2, xx2, bop, xx);
    }
    // ---- rows for the exact path: nothing is live here
    while (flagged) {                                                   // wave-uniform
        const int ti = __builtin_ctzll(flagged);
        flagged &= flagged - 1;
        const unsigned nd = __builtin_amdgcn_readfirstlane(need_s[wave][ti]);
        encode_rows_slow_v<IdxT, DP>(a.x, a.x_rs, a.out, a.o_rs, a.cb, a.cc, a.K, DP, a.k_pad, 0, m, row_begin + 32 * (int64_t)ti, nd);
    }
    if (a.stamps && lane == 0) {
        unsigned long long* o = a.stamps + ((size_t)blockIdx.x * 4 + wave) * kScreenStampWords;
        o[0] = st_tiles; o[1] = st_steps; o[2] = st_rows;
        o[3] = __builtin_amdgcn_s_memtime() - st_t0; o[4] = __builtin_amdgcn_s_memrealtime() - st_r0; o[5] = st_stage;
    }
}

}  // namespace pqhip
