// kernels_mfma16_screen.hip.h -- the body of k_encode_mfma16<8, 20, IdxT>: screen all 256 centroids on
// v_mfma_f32_32x32x16_f16, then resolve the rows the screen cannot decide exactly.
//
// Screening value A(c, r) = s^2 (cc(c) - 2 c.x(r)), computed entirely in the accumulator by f16 matrix
// instructions.  s = 2^e is one power of two per subquantizer, chosen from max cc so that s^2 max cc is in [2^12, 2^14);
// x and c are scaled by it (exact) and rounded to f16 (RNE), cc~ = s^2 cc is split into f16 hi + lo; along k:
//     A operand (centroid):  [-2 c~ (20) | cc~_hi | cc~_lo | 0 | 0 ...]      (a padding centroid: [0 ... | 0 | 0 | 65504 | 0 ...])
//     B operand (row):       [   x~ (20) |    1   |    1   | 65504 | 0 ...]
// xx is the same for every centroid of a row and is left out.  |A(c) - s^2 (D(c) - xx)| <= E_r for every c, D the CANON-F32
// distance, with E_r = kScreenRel / 2 * (xx~ + max cc~) + kScreenAbs / 2 (the proof and its terms: DESIGN.md §5).
// The loop screens on v_mfma_f32_32x32x16_f16 (round 12): a block is 32 centroids x the tile's 32 rows, its 32 k
// positions are two instructions chained through the accumulator, and an instruction holds the vector issue as long as a
// 16x16x32 one for four times the values.  The chain adds the second instruction's products to the first's sum: one
// more f32 addition than a single instruction's, inside the bound's term for an arbitrary accumulation order.
// The key of a value is its f32 bits with the low 7 mantissa bits replaced by the lane-local centroid number
// half-block << 3 | column (that moves a value by < 2^-16 |A|, part of the bound).  Per lane a tile has 128 values
// d[b][i], block b = 0..7, accumulator register i = 0..15; registers 0..7 and 8..15 of block b are half-blocks 2b and
// 2b + 1, and i & 7 is the column.  The loop hands the merge the smallest key mk and a lower bound sk of every other
// value (less a key's perturbation) without keying every value (rounds 9 and 12): 21 vector instructions
// per 16 values,
//     block side    hb[j] = min of half-block j, raw (three v_min3_f32 + one v_min_f32); kb[j] = (bits(hb[j]) & ~15) | j;
//                   (mB, sB) = the two smallest kb (keep2 on the block's two keys)
//     column side   mv[c] = min over the half-blocks of column c, raw: one v_min3_f32 per column folds both half-blocks
//     end of tile   kv[c] = (bits(mv[c]) & ~7) | c; (mA, sA) = the two smallest kv;
//                   mk = (mB & ~127) | ((mB & 15) << 3) | (mA & 7),  sk = min(sA, sB)
// Every value but the smallest differs from it in column (then sA is at or below it, up to the 3 index bits) or in
// half-block (then sB is, up to the 4 index bits); exact ties give sk = mk up to those bits; and when sk exceeds mk by the
// margin below, the smallest value is unique, mB is its half-block's key, mA its column's, and mk is bit for bit its
// 7-bit key.  The two lane halves of a row are merged once per trip of two tiles, 64 rows, one row per lane.  When the
// second smallest S of the row exceeds the smallest key M by more than 2 E_r, the centroid of M is the first minimum of
// D and its code is stored: no FP32 arithmetic.
// Every other row is recorded in the loop and resolved after it, where nothing is live: rows with at most one candidate
// per lane half (both halves' second value above tau) by encode_rows_few, one row per lane, from the merge's two keys;
// the other rows with two or more candidates (|M| tiny included) by encode_rows_cand_f16, 16 rows at a time on the
// 16x16x32 instruction and the same image, at a cost proportional to their candidates; rows whose scaled norm is beyond
// f16's range, or under a bad codebook, by encode_rows_slow_v, as in the FP32 body.
//
// Layout (32x32x16 f16): lane (n32 = lane & 31, h = lane >> 5) supplies A[n32][k = 8h .. 8h + 7] and
// B[k = 8h .. 8h + 7][n32] and receives D[8 (i >> 2) + 4h + (i & 3)][n32] in register i.  A = 32 centroids (block b),
// B = the tile's 32 rows.  The f16 codebook image (256 rows of 32 f16 = 64 B, no padding) is built once per codebook from
// cb / cc (k_build_screen_image) and copied into LDS by the workgroup; chunk j (16 B) of row r is stored at chunk
// j ^ ((r >> 2) & 3).  k step ks of block b reads row 32 b + n32, chunk 2 ks + h: the 16 lanes of a quarter wave are 16
// rows in a row and land on 16 different 16-B bank slots, as under the 16x16x32 reads.
// The B operands of a lane are x[8h .. 8h + 7] of its row for k step 0 and, for k step 1, x[16 .. 19] and the
// [1 1 65504 0] tail in half 0, zeros in half 1: three 4-float chunks, scaled and converted in registers
// (v_cvt_pk_f16_f32).
// Schedule: a selection step works on one block, 16 values per lane.  The steps are software-pipelined over two
// accumulator sets of 16 registers: before the selection on block b the two matrix instructions of block b + 1 are
// issued into the other set, their A fragments read in front of them; the next tile's rows are loaded and converted
// into f16 operands in the middle of the current tile, and its first block is issued before the selection on the last,
// so it runs under the trip's merge.
#pragma once
#include "kernels_mfma.hip.h"

namespace pqhip {

// the screen's constants, on the scaled values (xx~ = s^2 xx, max cc~ = s^2 max cc, M): accept a row when
// S > M + kScreenRel * (xx~ + max cc~) + kScreenAbs and |M| > kScreenTiny
constexpr float kScreenRel = 0x1.2p-9f;   // >= 2 E_r + 2 key perturbation: (132.6 + 4.04) 2^-16 needed, 144 2^-16 taken
constexpr float kScreenAbs = 0x1p-100f;   // flushed f32 subnormal products and partial sums
constexpr float kScreenTiny = 0x1p-100f;  // keeps the index bits of M out of the subnormal range
// the scale: s^2 max cc in [2^kScreenScaleLo, 2^(kScreenScaleLo + 2)); rows with xx~ >= kScreenMaxXX take the exact path
// (then every |x~_k| < 2^15 and no f16 operand overflows); codebooks with max cc outside [2^-100, 2^100) do too
constexpr int kScreenScaleLo = 12;
constexpr float kScreenMaxXX = 0x1p30f;
constexpr float kScreenMinCC = 0x1p-100f;
// the key of a value: its f32 bits with the low 7 mantissa bits replaced by half-block << 3 | column (round 12).
// kKeyMask is the 6-bit mask of the block / column rule of rounds 9 and 10 on the 16x16x32 instruction, which the 7-bit
// rule extends; tests/test_screen_select_model.py and tests/test_screen_pairs_model.py state that rule with it
constexpr unsigned kKey7Mask = 0xffffff80u;
[[maybe_unused]] constexpr unsigned kKeyMask = 0xffffffc0u;

// instantiations that take the screen body (the others keep the FP32 body of k_encode_mfma16)
template <int T, int DP> constexpr bool mfma16_screens() { return mfma16_screen_shape(T, DP); }

// The f16 codebook image of the screen, built once per codebook by k_build_screen_image (kernels_prep.hip.h) and copied
// into LDS by every workgroup: per subquantizer kScreenImageBytes in LDS order (256 rows of 32 f16, chunk j of row r at
// chunk j ^ ((r >> 2) & 3), padding rows included), and behind the M images one 16-byte header per subquantizer whose
// first word holds the bits of max cc.
constexpr int kScreenImageBytes = 256 * 32 * 2;
constexpr int kScreenHeaderBytes = 16;
constexpr size_t screen_image_bytes(int64_t M) { return (size_t)M * (kScreenImageBytes + kScreenHeaderBytes); }

// max cc -> the scale, the one rule of the kernel that builds the image and the kernel that screens with it
struct ScreenScale {
    bool cc_range;   // max cc in [kScreenMinCC, kBigNorm): the screen applies (false for NaN)
    float sc, sc2;   // s and s^2
};
__device__ __forceinline__ ScreenScale screen_scale(float maxcc)
{
    ScreenScale r;
    r.cc_range = maxcc >= kScreenMinCC && maxcc < kBigNorm;
    // s = 2^e with e = floor((kScreenScaleLo + 1 - log2 max cc) / 2): s^2 max cc in [2^12, 2^14), e in [-43, 56]
    const int escale = r.cc_range ? (kScreenScaleLo + 1 - ((int)(__float_as_uint(maxcc) >> 23) - 127)) >> 1 : 0;
    r.sc = __uint_as_float((unsigned)(127 + escale) << 23);
    r.sc2 = __uint_as_float((unsigned)(127 + 2 * escale) << 23);
    return r;
}

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// two f32 -> packed f16 pair, RNE (v_cvt_pk_f16_f32); a in the low half
__device__ __forceinline__ unsigned pk_f16(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, f16x2_t));
}
__device__ __forceinline__ float f16_lo(unsigned p) { return (float)__builtin_bit_cast(f16x2_t, p)[0]; }
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
// raw screening values folded two at a time (accumulator bits as they are: no canonicalization, as for the keys)
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ void fold2(float& m, float a, float b) { asm("v_min3_f32 %0, %0, %1, %2" : "+v"(m) : "v"(a), "v"(b)); }

// The two functions below that resolve rows after the loop receive generic pointers, and an out-of-line one would load
// and store through flat instructions, which also count against the LDS counter.  They address x, the codebook, the
// norms and the codes through global-address-space pointers and their LDS records through LDS ones: global_load /
// global_store / ds_read, same addresses, same values.
#define PQHIP_GLOBAL_AS __attribute__((address_space(1)))
#define PQHIP_LDS_AS __attribute__((address_space(3)))
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef f32x4_u PQHIP_GLOBAL_AS const* gf32x4_p;
// a row or a centroid of 20 floats
__device__ __forceinline__ void load20_global(const PQHIP_GLOBAL_AS float* p, float (&v)[20])
{
#pragma unroll
    for (int e = 0; e < 20; e += 4) {
        const f32x4 t = *reinterpret_cast<gf32x4_p>(p + e);
        v[e] = t[0]; v[e + 1] = t[1]; v[e + 2] = t[2]; v[e + 3] = t[3];
    }
}
// chain_dot_global (common.hip.h) of two register vectors of 20 floats: one chain (20 < kKC), the same operations in the
// same order
__device__ __forceinline__ float chain_dot20(const float (&a)[20], const float (&b)[20])
{
    float ab = 0.f;
#pragma unroll
    for (int k = 0; k < 20; ++k) ab = ffma(a[k], b[k], ab);
    return ab;
}

// The rows the screen's loop does not decide, after it: 16 at a time from all of the wave's tiles, the
// f16 screen again on them, then the CANON-F32 distance of every centroid whose value is within thr of the row's smallest
// value -- that set holds the first minimum, since A(c*) <= A(c) + 2 E_r for every c -- and the first minimum of those
// (ties to the lower index).  The cost is two passes of 16 matrix instructions per 16 rows plus one distance per candidate,
// against K distances per row on encode_rows_slow_v.  img: the workgroup's f16 image; tiles[t]: the rows of tile t.
// Inline: out of line it took more registers than a callee may use freely and saved 48 of them on the stack, its whole
// 280-byte frame; in the kernel, behind the loop, nothing is live and nothing is saved.
template <typename IdxT>
__device__ __forceinline__ void encode_rows_cand_f16(const float* x, int64_t x_rs, void* out, int64_t o_rs, const float* cbk,
                                                  const float* ccn, int K, int k_pad, int dsub, int64_t n, int m,
                                                  int64_t row_begin, const unsigned short* img, const unsigned* tiles,
                                                  unsigned long long flagged_c, float sc, float maxcct)
{
    constexpr int DP = 20, kRow = 32;
    const int lane = threadIdx.x & 63;
    const int i16 = lane & 15;
    const int q = lane >> 4;
    const int c0 = (8 * q) % 20, c1 = (8 * q + 4) % 20;
    const PQHIP_GLOBAL_AS float* const xsub = (const PQHIP_GLOBAL_AS float*)x + (int64_t)m * dsub;
    const PQHIP_GLOBAL_AS float* const plast = xsub + (n - 1) * x_rs;
    const PQHIP_GLOBAL_AS float* const cbm = (const PQHIP_GLOBAL_AS float*)cbk + (int64_t)m * K * DP;
    const PQHIP_GLOBAL_AS float* const ccm = (const PQHIP_GLOBAL_AS float*)ccn + (int64_t)m * k_pad;
    const PQHIP_LDS_AS unsigned* const tiles_l = (const PQHIP_LDS_AS unsigned*)tiles;
    const float sl = q < 3 ? sc : 0.f;
    const float sc2 = sc * sc;
    const PQHIP_LDS_AS unsigned short* const arow = (const PQHIP_LDS_AS unsigned short*)img + (i16 * kRow + 8 * (q ^ ((i16 >> 2) & 3)));
    unsigned cur = 0;
    int cur_ti = 0;
    while (cur || flagged_c) {                                          // wave-uniform
        int rel = -1;                                                   // row of lane i16: row_begin + rel, or none
        for (int t = 0; t < 16; ++t) {
            while (!cur && flagged_c) {
                cur_ti = __builtin_ctzll(flagged_c);
                flagged_c &= flagged_c - 1;
                cur = __builtin_amdgcn_readfirstlane(tiles_l[cur_ti]);
            }
            if (!cur) break;
            const int r = 32 * cur_ti + __builtin_ctz(cur);
            cur &= cur - 1;
            if (i16 == t) rel = r;
        }
        const bool rv = rel >= 0;
        const int64_t row = row_begin + rel;
        const PQHIP_GLOBAL_AS float* p = rv ? xsub + row * x_rs : plast;
        const f32x4 v0 = *reinterpret_cast<gf32x4_p>(p + c0), v1 = *reinterpret_cast<gf32x4_p>(p + c1);
        // the B operand and s^2 xx exactly as the loop builds them
        unsigned w[4] = {pk_f16(sl * v0[0], sl * v0[1]), pk_f16(sl * v0[2], sl * v0[3]), pk_f16(sl * v1[0], sl * v1[1]),
                         pk_f16(sl * v1[2], sl * v1[3])};
        if (q == 2) { w[2] = 0x3c003c00u; w[3] = 0x7bffu; }
        const u32x4_t bo = (u32x4_t){w[0], w[1], w[2], w[3]};
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { s0 = fmaf(v0[j], v0[j], s0); s1 = fmaf(v1[j], v1[j], s1); }
        float u[4];
        gather_groups((q < 3 ? s0 : 0.f) + (q < 2 ? s1 : 0.f), u);
        const float xxs = sc2 * ((u[0] + u[1]) + (u[2] + u[3]));
        // Two passes of 16 matrix instructions, neither of which keeps the 64 values: the first folds every block into the
        // lane's smallest value, the second computes the blocks again -- the same instruction on the same operands, the
        // same bits -- and tests a block's four values against tau while they are live.  The second pass reads its A
        // fragments through a pointer the compiler cannot see through, so that it does not merge the passes and carry
        // the values (or the fragments) from one to the other.
        auto block = [&](const PQHIP_LDS_AS unsigned short* ar, int cb) {
            const u32x4_t af = *reinterpret_cast<const PQHIP_LDS_AS u32x4_t*>(ar + cb * 16 * kRow);
            return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, af), __builtin_bit_cast(f16x8_t, bo),
                                                          (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        };
        // the values are no NaN for a row that is resolved here (finite operands); the minimum of a lane with no row is not used
        float mn = __builtin_inff();
#pragma unroll
        for (int cb = 0; cb < 16; ++cb) {
            // four blocks in flight at a time: all sixteen fragments read ahead are 64 registers more
            if (cb % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            const f32x4 d = block(arow, cb);
            mn = __builtin_elementwise_minimum(mn, __builtin_elementwise_minimum(__builtin_elementwise_minimum(d[0], d[1]),
                                                                                 __builtin_elementwise_minimum(d[2], d[3])));
        }
        float mq[4];
        gather_groups(mn, mq);
        // (a lane with no row tests against NaN: no candidate, and no branch around the tests for the compiler to sink
        // them into, behind all sixteen blocks)
        const float tau = rv ? fminf(fminf(mq[0], mq[1]), fminf(mq[2], mq[3])) + (kScreenRel * (xxs + maxcct) + kScreenAbs)
                             : __builtin_nanf("");
        const PQHIP_LDS_AS unsigned short* arow2 = arow;
        asm volatile("" : "+v"(arow2) : "v"(tau));                     // (and not before tau is there to test against)
        unsigned cw[2] = {0u, 0u};                                      // bit 4 cb + v of the two words: centroid 16 cb + 4 q + v
#pragma unroll
        for (int cb = 0; cb < 16; ++cb) {
            if (cb % 4 == 0) __builtin_amdgcn_sched_barrier(0);
            const f32x4 d = block(arow2, cb);
#pragma unroll
            for (int v = 0; v < 4; ++v) cw[cb >> 3] |= (d[v] <= tau ? 1u : 0u) << (4 * (cb & 7) + v);
            // the four blocks' bits are there before the next four are issued (the tests would otherwise move down to
            // the word's first use, after the last block)
            if (cb % 4 == 3) asm volatile("" : "+v"(cw[cb >> 3]));
        }
        unsigned long long cm = ((unsigned long long)cw[1] << 32) | cw[0];
        float xr[DP];
        load20_global(xsub + (rv ? row : 0) * x_rs, xr);
        const float xxe = rv ? norm_unrolled_static<DP>(xr) : 0.f;
        unsigned bh = 0xffffffffu, bl = 0xffffffffu;
        // the candidates of a lane two at a time, lowest index first: a lane with one left (or none) evaluates centroid 0
        // in the empty slot and drops the result
        while (__builtin_amdgcn_ballot_w64(cm != 0)) {                 // wave-uniform
            int j[2];
            bool cv[2];
            float ce[2][DP], ccj[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int bit = cm ? __builtin_ctzll(cm) : 0;
                j[s] = 16 * (bit >> 2) + 4 * q + (bit & 3);
                cv[s] = cm != 0 && j[s] < K;
                cm &= cm - 1;
                const int jj = cv[s] ? j[s] : 0;
                load20_global(cbm + (int64_t)jj * DP, ce[s]);
                ccj[s] = ccm[jj];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float dp = chain_dot20(xr, ce[s]);
                const unsigned kh = ord_key(fsub(fadd(xxe, ccj[s]), fadd(dp, dp)));
                if (cv[s] && (kh < bh || (kh == bh && (unsigned)j[s] < bl))) { bh = kh; bl = (unsigned)j[s]; }
            }
        }
        float hq[4], lq[4];
        gather_groups(__uint_as_float(bh), hq);
        gather_groups(__uint_as_float(bl), lq);
        bh = __float_as_uint(hq[0]);
        bl = __float_as_uint(lq[0]);
#pragma unroll
        for (int g = 1; g < 4; ++g) {
            const unsigned h = __float_as_uint(hq[g]), l = __float_as_uint(lq[g]);
            if (h < bh || (h == bh && l < bl)) { bh = h; bl = l; }
        }
        if (rv && q == 0) ((PQHIP_GLOBAL_AS IdxT*)out)[row * o_rs + m] = (IdxT)bl;
    }
}

// The few-candidate rows of a wave (rounds 10 and 12): rows off the screen in which the second value of
// both lane halves is above tau, so each half holds at most one candidate and its key names it.  The trip's merge appends
// {key of half 0, key of half 1, tau, the row's offset in the wave} (16 bytes) to a list in LDS; a row that finds the
// list full keeps its bit in the candidate record and is resolved by encode_rows_cand_f16.
constexpr int kScreenFewCap = 96;           // rows per wave
constexpr int kScreenFewWords = 2;          // uint2 per entry

// centroid of a 7-bit key kb = half-block << 3 | column in lane half h (accumulator register i = 8 (half-block & 1) +
// column of block half-block >> 1 is centroid 32 b + 8 (i >> 2) + 4 h + (i & 3))
__device__ __forceinline__ unsigned screen_key_centroid(unsigned kb, unsigned h)
{
    return 16u * (kb >> 3) + 8u * ((kb >> 2) & 1u) + 4u * h + (kb & 3u);
}

// The listed rows after the loop, 64 at a time, one row per lane and no cross-lane step: the candidates are the lane
// halves g with key[g] <= tau, centroid screen_key_centroid(key & 127, g); their CANON-F32 distances with the operations
// of encode_rows_cand_f16, the first minimum of those (ties to the lower index).  That set holds the first minimum of D
// (DESIGN.md §5, round 10); a key whose index bits are off names one centroid more, which cannot win.  A half that is
// no candidate (or names a padding centroid) evaluates centroid 0 and drops the result.
template <typename IdxT>
__device__ __noinline__ void encode_rows_few(const float* x, int64_t x_rs, void* out, int64_t o_rs, const float* cbk,
                                             const float* ccn, int K, int k_pad, int dsub, int m, int64_t row_begin,
                                             const uint2* list, int count)
{
    constexpr int DP = 20;
    const int lane = threadIdx.x & 63;
    const PQHIP_GLOBAL_AS float* const xsub = (const PQHIP_GLOBAL_AS float*)x + (int64_t)m * dsub;
    const PQHIP_GLOBAL_AS float* const cbm = (const PQHIP_GLOBAL_AS float*)cbk + (int64_t)m * K * DP;
    const PQHIP_GLOBAL_AS float* const ccm = (const PQHIP_GLOBAL_AS float*)ccn + (int64_t)m * k_pad;
    const PQHIP_LDS_AS u32x4_t* const list_l = (const PQHIP_LDS_AS u32x4_t*)list;
    for (int e0 = 0; e0 < count; e0 += 64) {                            // wave-uniform
        const bool rv = e0 + lane < count;
        const u32x4_t en = list_l[rv ? e0 + lane : 0];                  // entry 0 exists: count > 0
        const unsigned key[2] = {en[0], en[1]};
        const float tau = __uint_as_float(en[2]);
        const int64_t row = row_begin + en[3];
        float xr[DP];
        load20_global(xsub + row * x_rs, xr);
        const float xxe = norm_unrolled_static<DP>(xr);
        unsigned bh = 0xffffffffu, bl = 0xffffffffu;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int j = (int)screen_key_centroid(key[g] & 127u, (unsigned)g);
            const bool cg = __uint_as_float(key[g]) <= tau && j < K;
            const int jj = cg ? j : 0;
            float ce[DP];
            load20_global(cbm + (int64_t)jj * DP, ce);
            const float dp = chain_dot20(xr, ce);
            const unsigned kh = ord_key(fsub(fadd(xxe, ccm[jj]), fadd(dp, dp)));
            if (cg && (kh < bh || (kh == bh && (unsigned)j < bl))) { bh = kh; bl = (unsigned)j; }
        }
        if (rv) ((PQHIP_GLOBAL_AS IdxT*)out)[row * o_rs + m] = (IdxT)bl;
    }
}

template <typename IdxT>
__device__ __forceinline__ void encode_mfma16_screen(const EncodeArgs& a)
{
    constexpr int DP = 20;
    constexpr int kRow = 32;  // f16 per image row, four 16-B chunks, chunk j of row r at j ^ ((r >> 2) & 3)
    __shared__ __attribute__((aligned(16))) unsigned short img_s[256 * kRow];
    __shared__ unsigned need_s[4][kMfma16MaxTiles];   // rows for encode_rows_slow_v
    __shared__ unsigned cand_s[4][kMfma16MaxTiles];   // rows for the candidate path
    __shared__ __attribute__((aligned(16))) uint2 few_s[4][kScreenFewCap * kScreenFewWords];   // rows for encode_rows_few

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n32 = lane & 31;                // the lane's row in a tile
    const int h = lane >> 5;                  // its half of the k range and of every block's centroids

    // ---- workgroup -> (row group, m), as the FP32 body
    const int64_t b = blockIdx.x;
    const int xcd = (int)(b & 7);
    const int64_t qq = b >> 3;
    const int64_t g_local = qq / a.M;
    const int m = (int)(qq - g_local * a.M);
    const int64_t group = g_local * 8 + xcd;
    const bool wg_active = (g_local < a.chunks_per_xcd) && (group < a.n_chunks);

    const unsigned long long st_s0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
    // the subquantizer's image, as k_build_screen_image left it: thread t copies the 16-byte chunks t, t + 256, t + 512 and
    // t + 768; max cc comes from the header with one wave-uniform load
    unsigned maxcc_bits = 0u;
    if (wg_active) {
        const u32x4_t* src = reinterpret_cast<const u32x4_t*>(a.screen_img) + (int64_t)m * (kScreenImageBytes / 16) + threadIdx.x;
        u32x4_t* dst = reinterpret_cast<u32x4_t*>(img_s) + threadIdx.x;
        u32x4_t ch[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ch[j] = src[256 * j];
        maxcc_bits = a.screen_img[(int64_t)a.M * (kScreenImageBytes / 4) + m * (kScreenHeaderBytes / 4)];
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[256 * j] = ch[j];
    }
    const float maxcc = __uint_as_float(maxcc_bits);
    const ScreenScale scale = screen_scale(maxcc);
    const bool cc_range = scale.cc_range;
    const float sc = scale.sc, sc2 = scale.sc2;
    __syncthreads();
    const unsigned long long st_stage = a.stamps ? __builtin_amdgcn_s_memtime() - st_s0 : 0;   // image staging
    const int64_t row_begin = (group * 4 + wave) * a.rows_per_item;
    if (!wg_active || row_begin >= a.n) return;
    int64_t row_end = row_begin + a.rows_per_item;
    if (row_end > a.n) row_end = a.n;
    const bool bad_codebook = a.bad_flag != nullptr && *a.bad_flag != 0;  // wave-uniform
    // strides too long for the loop's 32-bit row offsets (below) send every row to the exact path, like a bad codebook
    const bool near_rows = (uint64_t)a.x_rs < (1ull << 24) && (uint64_t)a.o_rs < (1ull << 24);   // wave-uniform
    const bool cb_ok = !bad_codebook && cc_range && near_rows;            // wave-uniform
    const float maxcct = sc2 * maxcc;                                    // max cc~, exact

    // x chunks of lane (n32, h): x[8h .. 8h + 7] for the first k step and one chunk of 4 floats for the second, x[16 .. 19]
    // in half 0; half 1 carries zeros there and reads x[8 .. 11] again, inside the sub-vector, to multiply it by zero
    const float* const xsub = a.x + (int64_t)m * a.dsub;
    // Addresses: a tile's base tile_row0 * x_rs is wave-uniform and stays in scalar registers; a lane adds the
    // loop-invariant 32-bit byte offset of its row and chunk (global_load with a scalar base), and the trip's store
    // adds lane * o_rs the same way: no 64-bit vector arithmetic in the steady state.
    // Under strides too long for that (rows 64 MiB apart) every lane reads its tile's first row, the loop decides
    // nothing, and encode_rows_slow_v, which addresses in 64 bits, encodes every row.
    // The loop keeps two sets of 16 accumulators, and few vector registers are left for values that stay the same from
    // trip to trip: the lane number, the offset of its first chunk and its two LDS addresses.  Everything else that
    // depends on the lane -- the third chunk's offset, the store's offset, the ragged tile's row -- is formed again
    // where it is used, from values the compiler cannot hoist (the empty asm statements).
    const unsigned xrs4 = near_rows ? (unsigned)a.x_rs * 4u : 0u;
    const unsigned ors = near_rows ? (unsigned)a.o_rs * (unsigned)sizeof(IdxT) : 0u;   // scalar
    const unsigned xoff0 = (unsigned)n32 * xrs4 + 32u * (unsigned)h;
    auto load_rows = [&](float (&v)[12], const char* base, unsigned o0) {
        // the offset stays a 32-bit value of this block, so that the loads take it next to the scalar base
        asm volatile("" : "+v"(o0));
        const unsigned o1 = h ? o0 : o0 + 64u;                           // x[16 .. 19], or x[8 .. 11] again
        const f32x4 v0 = *reinterpret_cast<const f32x4_u*>(base + o0), v1 = *reinterpret_cast<const f32x4_u*>(base + o0 + 16);
        const f32x4 v2 = *reinterpret_cast<const f32x4_u*>(base + o1);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = v0[j]; v[4 + j] = v1[j]; v[8 + j] = v2[j]; }
    };
    auto load_tile = [&](float (&v)[12], int64_t tile_row0) {
        if (tile_row0 + 32 <= a.n) {                                     // wave-uniform: every row of the tile exists
            load_rows(v, reinterpret_cast<const char*>(xsub + tile_row0 * a.x_rs), xoff0);
        } else {
            // the ragged last tile, or one past the end: rows >= n read the last row instead (never stored or recorded)
            const int64_t r0 = tile_row0 < a.n ? tile_row0 : a.n - 1;   // scalar
            int last = (int)(a.n - 1 - r0);                             // 0 .. 30
            asm volatile("" : "+s"(last));
            const int nl = lane & 31;
            load_rows(v, reinterpret_cast<const char*>(xsub + r0 * a.x_rs), (unsigned)(nl < last ? nl : last) * xrs4 + (h ? 32u : 0u));
        }
    };
    // own: the lane's part of ||x||^2 of its row; the trip's merge sums the two halves
    auto split = [&](const float (&v)[12], u32x4_t (&bop)[2], float& own) {
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = pk_f16(sc * v[2 * j], sc * v[2 * j + 1]);
        bop[0] = (u32x4_t){w[0], w[1], w[2], w[3]};
        // half 1 carries zeros in the second k step
        const unsigned t0 = pk_f16(sc * v[8], sc * v[9]), t1 = pk_f16(sc * v[10], sc * v[11]);
        bop[1] = (u32x4_t){h ? 0u : t0, h ? 0u : t1, h ? 0u : 0x3c003c00u, h ? 0u : 0x7bffu};
        // s^2 ||x||^2 for the bound and the range test (not rule 1: any f32 sum will do): the two halves' first chunks
        // and the third chunk of half 0 cover the row once
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { s0 = fmaf(v[j], v[j], s0); s1 = fmaf(v[4 + j], v[4 + j], s1); s2 = fmaf(v[8 + j], v[8 + j], s2); }
        own = (s0 + s1) + (h ? 0.f : s2);
    };

    const unsigned kHalfMask = 0xfffffff0u, kColMask = 0xfffffff8u;
    unsigned long long flagged = 0, flagged_c = 0;                      // wave-uniform: tiles with rows for the two exact paths
    uint2* few_w = few_s[wave];                                         // wave-uniform: the list's next entry
    int few_room = kScreenFewCap;
    unsigned long long st_tiles = 0, st_steps = 0, st_rows = 0;   // st_rows: {other rows off the screen, two-candidate rows}
    unsigned long long st_full = 0;                               // few-candidate rows that found the list full
    const unsigned long long st_t0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0, st_r0 = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    // A fragments of block b: row 32 b + n32, chunks h (k step 0) and 2 + h (k step 1), swizzled
    const unsigned short* const arow0 = &img_s[n32 * kRow + 8 * (h ^ ((n32 >> 2) & 3))];
    const unsigned short* const arow1 = &img_s[n32 * kRow + 8 * ((2 + h) ^ ((n32 >> 2) & 3))];
    auto load_a = [&](int b, u32x4_t (&af)[2]) {
        af[0] = *reinterpret_cast<const u32x4_t*>(arow0 + b * 32 * kRow);
        af[1] = *reinterpret_cast<const u32x4_t*>(arow1 + b * 32 * kRow);
    };
    // one block of 32 centroids on the tile's 32 rows: two k steps chained through the accumulator
    auto screen = [&](const u32x4_t (&af)[2], const u32x4_t (&b)[2], f32x16& acc) {
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const f32x16 t = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, af[0]), __builtin_bit_cast(f16x8_t, b[0]), z, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, af[1]), __builtin_bit_cast(f16x8_t, b[1]), t, 0, 0, 0);
    };

    // prologue: the first tile's operands, block 0's values, the A fragments of block 1
    float xv[12];
    u32x4_t bop[2];
    float own;
    load_tile(xv, row_begin);
    split(xv, bop, own);
    u32x4_t af[2];
    f32x16 acc[2];
    load_a(0, af);
    screen(af, bop, acc[0]);
    // the first block has no selection step between its issue and its read (see the fence in tile): wait it out, once
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7");
    __builtin_amdgcn_sched_barrier(0);
    // The selection of one 32-row tile; bop holds its split rows, bnext / ownn receive the next tile's, mk / sk the
    // smallest key and a lower bound of every other value of the lane.  A trip of the loop below is two tiles on
    // alternating operand sets (no operand is copied at the seam) and ONE merge of its 64 rows, one row per lane.
    auto tile = [&](int64_t row0, const u32x4_t (&bop)[2], u32x4_t (&bnext)[2], float& ownn, float& mk, float& sk) {
        // row0 stays a scalar: the tile's base address is formed from it in scalar registers
        asm("" : "+s"(row0));
        float mB, sB, mv[8];
        // step b: issue block b + 1 (mod 8: the next tile's first, which then runs under the trip's second tile or the
        // merge) into the other accumulator set, read the A fragments of block b + 2, then select on block b's 16 values
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            load_a((b + 1) & 7, af);
            // the next tile's rows (past row_end the loads are clamped like a short tile's, and their result is never
            // used): loaded and converted in the middle of the tile, between the merges
            if (b == 1) load_tile(xv, row0 + 32);
            if (b == 5) split(xv, bnext, ownn);                         // the loads have landed by now
            screen(af, b < 7 ? bop : bnext, acc[(b + 1) & 1]);
            // The raw values go straight into inline assembly, and the compiler inserts the wait states between a
            // matrix instruction and a vector read of its result only in front of instructions of its own.  Nothing
            // crosses this fence, so a block issued in one step is read a whole step's selection (21 vector
            // instructions, 20 in a tile's first) and the next block's issue later, however the steps are scheduled
            // inside (tools/mfma_read_distance.py checks the compiled kernel)
            __builtin_amdgcn_sched_barrier(0);
            const f32x16 d = acc[b & 1];
            // block side: the raw minimum of each half-block (registers 0..7 and 8..15), keyed by its number in 4 bits
            const float b0 = vmin3(vmin3(d[0], d[1], d[2]), vmin3(d[3], d[4], d[5]), vmin(d[6], d[7]));
            const float b1 = vmin3(vmin3(d[8], d[9], d[10]), vmin3(d[11], d[12], d[13]), vmin(d[14], d[15]));
            const float k0 = __uint_as_float((__float_as_uint(b0) & kHalfMask) | (unsigned)(2 * b));
            const float k1 = __uint_as_float((__float_as_uint(b1) & kHalfMask) | (unsigned)(2 * b + 1));
            // column side: the raw minimum of every column (register & 7) over the half-blocks
            if (b == 0) {
                mB = vmin(k0, k1);
                sB = vmax(k0, k1);
#pragma unroll
                for (int c = 0; c < 8; ++c) mv[c] = vmin(d[c], d[8 + c]);
            } else {
                keep2(mB, sB, k0, k1);
#pragma unroll
                for (int c = 0; c < 8; ++c) fold2(mv[c], d[c], d[8 + c]);
            }
        }
        // end of tile: the smallest value is the smallest half-block minimum and the smallest column minimum at once,
        // which names its half-block and its column; every other value lies in another column or in another half-block
        float kv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = __uint_as_float((__float_as_uint(mv[c]) & kColMask) | (unsigned)c);
        float mA = vmin(kv[0], kv[1]), sA = vmax(kv[0], kv[1]);
        keep2(mA, sA, kv[2], kv[3]);
        keep2(mA, sA, kv[4], kv[5]);
        keep2(mA, sA, kv[6], kv[7]);
        const unsigned mb = __float_as_uint(mB);
        mk = __uint_as_float((mb & kKey7Mask) | (((mb & 15u) << 3) | (__float_as_uint(mA) & 7u)));
        sk = vmin(sA, sB);
    };
    u32x4_t bop2[2];
    float own2, ownn = 0.f;
    float mk, sk, mk2, sk2;
    for (int64_t row0 = row_begin, tile_idx = 0; row0 < row_end; row0 += 64, tile_idx += 2) {
        const unsigned long long st_a = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
        tile(row0, bop, bop2, own2, mk, sk);
        // rows_per_item is a multiple of 32, not of 64: a wave's last trip can be one tile.  Lanes 32 .. 63 then stand
        // for rows of the next wave; their keys are set here and their rows are masked by row_end below.
        const bool two = row0 + 32 < row_end;                            // wave-uniform
        if (two) tile(row0 + 32, bop2, bop, ownn, mk2, sk2);
        else mk2 = sk2 = __builtin_inff();
        // ---- merge, once per trip: one half exchange per quantity brings both halves of row row0 + 32 t + n32 into
        // lane 32 t + n32 -- the row's offset in the trip is the lane number -- then decide the row in that one lane;
        // store the decided rows, record the others
        const auto xm = __builtin_amdgcn_permlane32_swap(__float_as_uint(mk), __float_as_uint(mk2), false, false);
        const auto xs = __builtin_amdgcn_permlane32_swap(__float_as_uint(sk), __float_as_uint(sk2), false, false);
        const auto xu = __builtin_amdgcn_permlane32_swap(__float_as_uint(own), __float_as_uint(own2), false, false);
        const float m0 = __uint_as_float(xm[0]), m1 = __uint_as_float(xm[1]);   // the keys of half 0 and half 1
        const float xx = sc2 * (__uint_as_float(xu[0]) + __uint_as_float(xu[1]));
        const float M = vmin(m0, m1);
        const float S2 = vmin(__uint_as_float(xs[0]), __uint_as_float(xs[1]));   // smaller second key of the two halves
        const float S = vmin(vmax(m0, m1), S2);
        const float tau = M + (kScreenRel * (xx + maxcct) + kScreenAbs);
        const bool valid = lane < (int)(row_end - row0 < 64 ? row_end - row0 : 64);   // scalar bound
        const bool in_range = valid && cb_ok && xx < kScreenMaxXX;       // the f16 operands are exact enough
        const bool plain = in_range && __builtin_fabsf(M) > kScreenTiny;
        const bool one = plain && S > tau;                               // a single candidate
        if (one) {
            // the half that holds M: only one does, since a tie between the two would make S = M
            const unsigned Mb = __float_as_uint(M);
            const unsigned hw = Mb == __float_as_uint(m0) ? 0u : 1u;
            char* ob = reinterpret_cast<char*>(reinterpret_cast<IdxT*>(a.out) + (row0 * a.o_rs + m));   // scalar
            unsigned os = ors;
            asm volatile("" : "+s"(os));                                 // lane * o_rs once per trip, not a register held
            unsigned oo = (unsigned)lane * os;
            asm volatile("" : "+v"(oo));                                 // as in load_rows
            *reinterpret_cast<IdxT*>(ob + oo) = (IdxT)screen_key_centroid(Mb & 127u, hw);
        }
        // few-candidate rows go to the wave's list (encode_rows_few): the second value of both halves is above tau, so
        // the candidates are the keys m0, m1 <= tau.  None of them may be tiny (index bits in the subnormal range): they
        // lie in [M, tau], which is clear of [-kScreenTiny, kScreenTiny] when tau is below it or M above it; a row this
        // holds back only takes the other path.
        const bool few = plain && !one && S2 > tau && (tau < -kScreenTiny || M > kScreenTiny);
        const unsigned long long fewm = __builtin_amdgcn_ballot_w64(few);
        // the list position: few_w points past the few-candidate rows met so far, few_room is what is left of the
        // capacity; a row that does not fit keeps its cand bit (few_room is then zero or negative for the rest of the
        // wave and few_w, past the list's end, is not used again)
        const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(fewm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)fewm, 0u));
        const bool listed = few && pos < few_room;
        if (listed)                                                     // skipped when no lane has one
            *reinterpret_cast<u32x4_t*>(few_w + kScreenFewWords * pos) =
                (u32x4_t){__float_as_uint(m0), __float_as_uint(m1), __float_as_uint(tau), (unsigned)(row0 - row_begin) + (unsigned)lane};
        const int few_k = __builtin_popcountll(fewm);                   // scalar
        few_w += kScreenFewWords * few_k;
        few_room -= few_k;
        // bit l of a ballot is row row0 + l: the low word is tile tile_idx's record, the high word the next tile's
        const unsigned long long need = __builtin_amdgcn_ballot_w64(valid && !in_range);
        const unsigned long long cand = __builtin_amdgcn_ballot_w64(in_range && !one && !listed);
        auto record = [&](unsigned* rec, unsigned long long& tiles, unsigned long long rows) {
            const unsigned lo = (unsigned)rows, hi = (unsigned)(rows >> 32);
            if (lo) {                                                   // wave-uniform
                if (lane == 0) rec[tile_idx] = lo;
                tiles |= 1ull << tile_idx;
            }
            if (hi) {                                                   // wave-uniform
                if (lane == 0) rec[tile_idx + 1] = hi;
                tiles |= 2ull << tile_idx;
            }
        };
        record(need_s[wave], flagged, need);
        record(cand_s[wave], flagged_c, cand);
        if (a.stamps) {
            // the rows with at most one candidate per half (the second key of both halves is above tau): one or two
            // candidates, which the list takes; the other rows off the screen keep the candidate or the exact path
            const int nfew = __builtin_popcountll(__builtin_amdgcn_ballot_w64(plain && !one && S2 > tau));
            const int off = __builtin_popcountll(need | __builtin_amdgcn_ballot_w64(in_range && !one));
            st_rows += (unsigned long long)nfew | ((unsigned long long)(off - nfew) << 32);
            st_full += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(few && !listed));
            st_tiles += two ? 2 : 1;
            st_steps += __builtin_amdgcn_s_memtime() - st_a;
        }
        own = ownn;
    }
    const unsigned long long st_p0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
    // ---- rows the screen does not decide (nothing is live here): the listed few-candidate rows one per lane, the others
    // 16 at a time
    if (few_room < kScreenFewCap)                                       // wave-uniform
        encode_rows_few<IdxT>(a.x, a.x_rs, a.out, a.o_rs, a.cb, a.cc, a.K, a.k_pad, a.dsub, m, row_begin, few_s[wave],
                              kScreenFewCap - (few_room > 0 ? few_room : 0));
    const unsigned long long st_p1 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
    if (flagged_c)                                                      // wave-uniform
        encode_rows_cand_f16<IdxT>(a.x, a.x_rs, a.out, a.o_rs, a.cb, a.cc, a.K, a.k_pad, a.dsub, a.n, m, row_begin,
                                   img_s, cand_s[wave], flagged_c, sc, sc2 * maxcc);
    const unsigned long long st_p2 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
    // ---- rows outside the f16 range or under a bad codebook: every centroid exactly
    while (flagged) {                                                   // wave-uniform
        const int ti = __builtin_ctzll(flagged);
        flagged &= flagged - 1;
        const unsigned nd = __builtin_amdgcn_readfirstlane(need_s[wave][ti]);
        encode_rows_slow_v<IdxT, DP>(a.x, a.x_rs, a.out, a.o_rs, a.cb, a.cc, a.K, DP, a.k_pad, 0, m, row_begin + 32 * (int64_t)ti, nd);
    }
    if (a.stamps && lane == 0) {
        unsigned long long* o = a.stamps + ((size_t)blockIdx.x * 4 + wave) * kScreenStampWords;
        o[0] = st_tiles; o[1] = st_steps; o[2] = st_rows;
        const unsigned long long st_end = __builtin_amdgcn_s_memtime();
        o[3] = st_end - st_t0; o[4] = __builtin_amdgcn_s_memrealtime() - st_r0; o[5] = st_stage;
        o[6] = st_full; o[7] = st_end - st_p0;
        o[8] = st_p1 - st_p0; o[9] = st_p2 - st_p1;                     // encode_rows_few, encode_rows_cand_f16
    }
}

}  // namespace pqhip
