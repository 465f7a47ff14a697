// kernels_flat_screen.hip.h -- conservative range screen over resident vectors on the matrix cores (include/pqhip.h:
// pqhip_flat_screen_f32_dev; DESIGN.md §5c has the bound and its proof).  For a batch of queries it returns, per query, a
// SUPERSET of what pqhip_flat_range_f32_dev returns at the same thresholds, as ascending row ids: a row is left out only
// when the f16 product sum proves that its exact value misses the threshold.  One stream of the matrix serves up to 64
// queries.  (Instantiated by pqhip_flat_screen.hip.)
//
// Screening value.  X_j = 2^x_exp x_j and Q_j = 2^e_q q_j (e_q one power of two per query: max |Q_j| in [2^13, 2^14))
// are rounded to f16 (RNE); a(q, r) = sum_j Q~_j X~_j is ONE chain of v_mfma_f32_32x32x16_f16 through one accumulator, in
// ascending trips of kFsKStep = 32 elements, two instructions per trip.  Inside a trip the k positions are permuted the
// same way for both operands (lane half h supplies elements 16 h + 8 s .. + 7 in step s), so that a lane loads 64
// consecutive bytes of its row.  Nothing in the chain depends on the grid or on the other queries of a pass.
//     L2:  v^ = xx + qq - s_q a,  s_q = 2^(1 - e_q - x_exp);   IP:  v^ = s_q a,  s_q = 2^(-e_q - x_exp)
// xx = ||x||^2 is accumulated in f32 from the elements as loaded; qq = ||q||^2 and ||q||_1 are f64 sums of the prep
// kernel.  |v^ - v| <= E = kFlatScreenRel (xx + qq) + kFlatScreenAbsX 2^-x_exp ||q||_1 + kFlatScreenAbs for the exact f32
// value v (half of each for the inner product).  The comparison is arranged so that the per-query part is one number:
//     w = fma(-s_q, a, c xx)   (c = 1 - kFlatScreenRel resp. -kFlatScreenRel / 2)
//     a row is PROVABLY OUTSIDE  iff  w > tau_q and w < +Inf,   tau_q = thr_q + B_q - qq  resp.  B_q - thr_q, rounded up,
// and it is returned iff it is allowed and not provably outside: a NaN anywhere (a non-finite element, Inf - Inf in the
// accumulator, a NaN threshold) and an infinite w (an f16 operand that overflowed, xx beyond f32) compare false and pass.
// A query the proof does not cover (a non-finite element, a largest element outside [2^-kFlatScreenMaxExp,
// 2^kFlatScreenMaxExp) unless it is the zero vector, |x_exp| > kFlatScreenMaxExp) gets tau = NaN: every allowed row.
//
// Layout (32x32x16 f16, kernels_mfma16_screen.hip.h): lane (n32 = lane & 31, h = lane >> 5) supplies A[n32][8h .. 8h + 7]
// and B[8h .. 8h + 7][n32] and receives D[8 (i >> 2) + 4h + (i & 3)][n32] in register i.  A = 32 queries of the image,
// B = the tile's 32 rows: a lane holds 16 queries x its own row per block of 32 queries.  The image of a pass is
// [32 NB][dp + kFsRowPad] f16 (dp = d rounded up to 32, zeros beyond d and beyond the pass's queries; the pad shifts
// consecutive rows by 16 bytes, so the 16 lanes of a quarter wave read 16 different bank slots), followed by one
// (s_q, tau_q) pair per query; k_flat_screen_prep builds it in scratch once per pass and every workgroup copies it.
//
// Units, order, passes.  The unit is a wave with a contiguous sub-range of its workgroup's rows (a multiple of 32: a
// tile is one mask word).  The count pass leaves the hit bitmap hits[tile][query] (one 32-bit word per tile of 32 rows
// and query, the queries of a tile side by side) and the unit's counts part[query][unit]; k_adc_range_scan turns them into
// first slots; k_flat_screen_fill walks the bitmap -- lane = query, tiles ascending, bits ascending -- and stores the row
// ids below `capacity`.  It does not read the matrix.  A disallowed row, a row past n and a tile without an allowed row
// are never loaded.
#pragma once
#include "kernels_adc_range.hip.h"

namespace pqhip {

// the bound's constants; tests/flat_screen_ref.py parses them
constexpr float kFlatScreenRel = 0x1.8p-10f;    // >= 1.354e-3 needed (operand rounding, accumulation, xx, the exact value, the epilogue)
constexpr double kFlatScreenAbsX = 0x1p-13;     // x 2^-x_exp ||q||_1: row elements below f16's normal range, rounded or flushed
constexpr float kFlatScreenAbs = 0x1p-100f;     // flushed f32 subnormals in the epilogue
constexpr int kFlatScreenQueryTop = 13;         // the largest scaled query element lies in [2^13, 2^14)
constexpr int kFlatScreenMaxExp = 40;           // |x_exp| and |log2 max |q_j|| the proof covers
constexpr int kFlatScreenMaxD = 2048;           // the accumulation term of the bound is stated for <= 2,048 products

constexpr int kFsWaves = 8;                     // waves (producer units) per 512-thread workgroup
constexpr int kFsTile = 32;                     // rows of a tile: one matrix instruction's N
constexpr int kFsKStep = 32;                    // elements of a trip of the k loop: two matrix instructions
constexpr int kFsRowPad = 8;                    // f16 of padding per image row
constexpr int kFsPrepThreads = 256;

typedef _Float16 fs_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 fs_f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned fs_u32x4 __attribute__((ext_vector_type(4)));

constexpr int flat_screen_dp(int d) { return (d + kFsKStep - 1) / kFsKStep * kFsKStep; }
constexpr size_t flat_screen_image_bytes(int qp, int d)
{
    return (size_t)qp * (flat_screen_dp(d) + kFsRowPad) * 2 + (size_t)qp * 8;
}

// the least f32 >= t (t itself when it is one; NaN and the infinities as they are)
__device__ __forceinline__ float flat_screen_round_up(double t)
{
    float f = (float)t;
    if ((double)f < t) {
        const unsigned b = __float_as_uint(f);
        f = f > 0.f ? __uint_as_float(b + 1u) : f < 0.f ? __uint_as_float(b - 1u) : __uint_as_float(1u);
    }
    return f;
}

// The image row and the (s, tau) pair of one query slot per workgroup; slots >= nq_pass are padding (zeros, tau = NaN).
// The three sums are reduced by a fixed tree over the 256 threads' partials (thread t owns j = t, t + 256, ..).
__global__ __launch_bounds__(kFsPrepThreads) void k_flat_screen_prep(const float* __restrict__ queries, int64_t q_rs, int nq_pass,
                                                                     int d, int ldq, const float* __restrict__ thr, int ip,
                                                                     int x_exp, unsigned short* __restrict__ img,
                                                                     float* __restrict__ prm /* [slots][2] */)
{
    __shared__ double s_qq[kFsPrepThreads], s_q1[kFsPrepThreads];
    __shared__ float s_mx[kFsPrepThreads];
    __shared__ int s_bad[kFsPrepThreads];
    const int slot = blockIdx.x, t = threadIdx.x;
    const bool real = slot < nq_pass;
    const float* qrow = queries + (int64_t)slot * q_rs;
    double qq = 0.0, q1 = 0.0;
    float mx = 0.f;
    int bad = 0;
    if (real) {
        for (int j = t; j < d; j += kFsPrepThreads) {
            const float v = qrow[j];
            if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad = 1;
            const float a = __builtin_fabsf(v);
            qq += (double)v * (double)v;
            q1 += (double)a;
            mx = a > mx ? a : mx;
        }
    }
    s_qq[t] = qq; s_q1[t] = q1; s_mx[t] = mx; s_bad[t] = bad;
    __syncthreads();
    for (int s = kFsPrepThreads / 2; s >= 1; s >>= 1) {
        if (t < s) {
            s_qq[t] += s_qq[t + s];
            s_q1[t] += s_q1[t + s];
            s_mx[t] = s_mx[t + s] > s_mx[t] ? s_mx[t + s] : s_mx[t];
            s_bad[t] |= s_bad[t + s];
        }
        __syncthreads();
    }
    qq = s_qq[0]; q1 = s_q1[0]; mx = s_mx[0]; bad = s_bad[0];
    const bool x_ok = x_exp >= -kFlatScreenMaxExp && x_exp <= kFlatScreenMaxExp;
    const bool zero = mx == 0.f;
    const int ex = (int)(__float_as_uint(mx) >> 23) - 127;       // floor(log2 max |q_j|) of a normal number
    const bool regular = real && !bad && x_ok && (zero || (ex >= -kFlatScreenMaxExp && ex < kFlatScreenMaxExp));
    const int e_q = zero ? 0 : kFlatScreenQueryTop - ex;         // in [-26, 53]
    const float sq = __uint_as_float((unsigned)(127 + (regular ? e_q : 0)) << 23);
    unsigned short* row = img + (size_t)slot * ldq;
    for (int j = t; j < ldq; j += kFsPrepThreads) {
        const _Float16 hv = regular && j < d ? (_Float16)(qrow[j] * sq) : (_Float16)0.f;
        row[j] = __builtin_bit_cast(unsigned short, hv);
    }
    if (t == 0) {
        float s = 0.f, tau = __builtin_nanf("");
        if (regular) {
            const double cx = __builtin_ldexp(1.0, -x_exp);
            const double half = ip ? 0.5 : 1.0;
            const double B = half * ((double)kFlatScreenRel * qq + kFlatScreenAbsX * cx * q1) + (double)kFlatScreenAbs;
            const double th = (double)thr[slot];
            s = __uint_as_float((unsigned)(127 + (ip ? 0 : 1) - e_q - x_exp) << 23);   // exponent in [-93, 67]
            tau = flat_screen_round_up(ip ? B - th : th + B - qq);
        }
        prm[2 * slot] = s;
        prm[2 * slot + 1] = tau;
    }
}

// 16 consecutive elements of a row from p, of which the first `valid` exist (<= 0: none): zeros beyond.  When all 16
// exist they are loaded with the widest loads the rows allow -- al = 16, 8 or 4: base and row stride are multiples of
// that many bytes (d = 300 in f16 has rows 600 bytes apart: 8) -- else one element at a time; never a byte past the
// row's d elements.
typedef _Float16 fs_f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void flat_screen_load16(const float* p, int valid, int al, float (&v)[16])
{
    if (valid >= 16 && al >= 16) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * c);
            v[4 * c] = t[0]; v[4 * c + 1] = t[1]; v[4 * c + 2] = t[2]; v[4 * c + 3] = t[3];
        }
    } else if (valid >= 16 && al >= 8) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x2 t = *reinterpret_cast<const f32x2*>(p + 2 * c);
            v[2 * c] = t[0]; v[2 * c + 1] = t[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = e < valid ? p[e] : 0.f;
    }
}
__device__ __forceinline__ void flat_screen_load16(const _Float16* p, int valid, int al, float (&v)[16])
{
    if (valid >= 16 && al >= 16) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const fs_f16x8 t = *reinterpret_cast<const fs_f16x8*>(p + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * c + e] = (float)t[e];
        }
    } else if (valid >= 16 && al >= 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const fs_f16x4 t = *reinterpret_cast<const fs_f16x4*>(p + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * c + e] = (float)t[e];
        }
    } else if (valid >= 16 && al >= 4) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const fs_f16x2 t = *reinterpret_cast<const fs_f16x2*>(p + 2 * c);
            v[2 * c] = (float)t[0]; v[2 * c + 1] = (float)t[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = e < valid ? (float)p[e] : 0.f;
    }
}

__device__ __forceinline__ unsigned flat_screen_pk(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, fs_f16x2));
}

// The count pass.  Workgroup b owns rows [b rows_per_wg, (b + 1) rows_per_wg) (rows_per_wg a multiple of 256), its wave w
// the sub-range [w rows_per_wg / 8, (w + 1) rows_per_wg / 8): unit u = 8 b + w.  img: the pass's image and pairs
// (16-byte aligned).  cx = 2^x_exp; cxx = the coefficient of xx in w; al: the alignment of the rows in bytes (16, 8, 4 or less).  part [nq_pass][units] and hits [tiles][32 NB] out.
template <typename T, int NB>
__global__ __launch_bounds__(64 * kFsWaves) void k_flat_screen(const T* __restrict__ x, int64_t n, int d, int64_t x_rs,
                                                               const uint32_t* __restrict__ allow,
                                                               const unsigned short* __restrict__ img, int ldq, float cx,
                                                               float cxx, int al, int64_t rows_per_wg, int nq_pass,
                                                               int64_t* __restrict__ part, uint32_t* __restrict__ hits)
{
    constexpr int QP = 32 * NB;
    extern __shared__ __attribute__((aligned(16))) unsigned short lds_img[];
    {
        const int chunks = (QP * ldq * 2 + QP * 8) / 16;
        const fs_u32x4* src = reinterpret_cast<const fs_u32x4*>(img);
        fs_u32x4* dst = reinterpret_cast<fs_u32x4*>(lds_img);
        for (int c = threadIdx.x; c < chunks; c += 64 * kFsWaves) dst[c] = src[c];
    }
    __syncthreads();
    const float2* prm = reinterpret_cast<const float2*>(lds_img + QP * ldq);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n32 = lane & 31, h = lane >> 5;
    const int64_t units = (int64_t)gridDim.x * kFsWaves;
    const int64_t unit = (int64_t)blockIdx.x * kFsWaves + wave;
    const int64_t sub = rows_per_wg / kFsWaves;                     // a multiple of 32
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    const int dp = flat_screen_dp(d);
    const float inf = __builtin_inff();
    int64_t cnt[NB];                                                // lane l < 32: the unit's hits of query 32 b + l
#pragma unroll
    for (int b = 0; b < NB; ++b) cnt[b] = 0;
    for (int64_t row0 = row_begin; row0 < row_end; row0 += kFsTile) {   // wave-uniform; row0 is a multiple of 32
        const int64_t left = row_end - row0;
        unsigned bits = left >= kFsTile ? 0xffffffffu : (1u << (int)left) - 1u;
        if (allow) bits &= allow[row0 >> 5];
        bits = (unsigned)__builtin_amdgcn_readfirstlane((int)bits);
        unsigned mine[NB];                                          // lane l < 32: the tile's mask of query 32 b + l
#pragma unroll
        for (int b = 0; b < NB; ++b) mine[b] = 0u;
        if (bits != 0u) {                                           // a tile without an allowed row loads nothing
            const bool ok = (bits >> n32) & 1u;
            const T* rp = x + (row0 + n32) * x_rs + 16 * h;         // dereferenced only when ok
            f32x16 acc[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
            float xx = 0.f;
            const unsigned short* arow = lds_img + n32 * ldq + 16 * h;
            for (int k0 = 0; k0 < dp; k0 += kFsKStep) {
                float v[16];
                flat_screen_load16(rp + k0, ok ? d - k0 - 16 * h : 0, al, v);
                unsigned w[8];
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    xx = __builtin_fmaf(v[e], v[e], xx);
                    xx = __builtin_fmaf(v[e + 1], v[e + 1], xx);
                    w[e >> 1] = flat_screen_pk(v[e] * cx, v[e + 1] * cx);
                }
                const fs_u32x4 b0 = (fs_u32x4){w[0], w[1], w[2], w[3]}, b1 = (fs_u32x4){w[4], w[5], w[6], w[7]};
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const fs_u32x4 a0 = *reinterpret_cast<const fs_u32x4*>(arow + b * 32 * ldq + k0);
                    const fs_u32x4 a1 = *reinterpret_cast<const fs_u32x4*>(arow + b * 32 * ldq + k0 + 8);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(fs_f16x8, a0), __builtin_bit_cast(fs_f16x8, b0),
                                                                    acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(fs_f16x8, a1), __builtin_bit_cast(fs_f16x8, b1),
                                                                    acc[b], 0, 0, 0);
                }
            }
            xx += __shfl_xor(xx, 32);                               // the row's two halves: the same sum in both lanes
            const float xk = cxx * xx;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int q0 = 8 * (i >> 2) + (i & 3);          // the query of half 0 in register i; half 1: q0 + 4
                    const float2 p = prm[b * 32 + q0 + 4 * h];
                    const float wv = __builtin_fmaf(-p.x, acc[b][i], xk);
                    const bool outside = wv > p.y && wv < inf;      // NaN and +-Inf: not proved, returned
                    const unsigned long long bl = __ballot(ok && !outside);
                    if (lane == q0) mine[b] = (unsigned)bl;
                    if (lane == q0 + 4) mine[b] = (unsigned)(bl >> 32);
                }
            }
        }
        if (lane < 32) {
            uint32_t* hrow = hits + (row0 >> 5) * QP;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (b * 32 + lane >= nq_pass) mine[b] = 0u;         // a padding query
                hrow[b * 32 + lane] = mine[b];
                cnt[b] += (int64_t)__popc(mine[b]);
            }
        }
    }
    if (lane < 32) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b * 32 + lane < nq_pass) part[(int64_t)(b * 32 + lane) * units + unit] = cnt[b];
    }
}

// The fill pass: the decomposition of the count pass, lane = query of the pass (qp = 32 or 64 per tile), the unit's
// tiles in ascending order, a word's bits in ascending order.  part: the first slot of every (query, unit), absolute.
__global__ __launch_bounds__(64 * kFsWaves) void k_flat_screen_fill(const uint32_t* __restrict__ hits, int qp, int nq_pass,
                                                                    int64_t n, int64_t rows_per_wg,
                                                                    const int64_t* __restrict__ part, int64_t capacity,
                                                                    int64_t* __restrict__ out_i)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kFsWaves;
    const int64_t unit = (int64_t)blockIdx.x * kFsWaves + wave;
    const int64_t sub = rows_per_wg / kFsWaves;
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    if (lane >= nq_pass || lane >= qp) return;                      // no cross-lane step below
    for (int q = lane; q < nq_pass; q += 64) {
        int64_t slot = part[(int64_t)q * units + unit];
#pragma unroll 4
        for (int64_t row0 = row_begin; row0 < row_end; row0 += kFsTile) {
            unsigned w = hits[(row0 >> 5) * qp + q];
            while (w) {
                const int b = __builtin_ctz(w);
                w &= w - 1;
                if (slot < capacity) out_i[slot] = row0 + b;
                ++slot;
            }
        }
    }
}

}  // namespace pqhip
