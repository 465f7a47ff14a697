// kernels_adc_screen.hip.h -- conservative range screen over resident u8 codes with u8 table images (include/pqhip.h:
// pqhip_adc_screen_f32_dev; DESIGN.md §5e has the bound and its proof).  For a batch of queries it returns, per query, a
// SUPERSET of what pqhip_adc_range_f32_dev resp. pqhip_adc_ip_range_f32_dev returns at the same thresholds, as ascending
// row ids: a row is left out only when an integer sum proves that its exact f32 value misses the threshold.  One stream
// of the codes serves up to 32 queries.  (Instantiated by pqhip_adc_screen.hip.)
//
// One form serves both metrics: the inner product is the distance form on the negated tables and the negated threshold
// (t' = -t, thr' = -thr; the f32 chain of the negated entries is the negated chain).  Per query, k_adc_screen_prep
// derives from the f32 tables, in f64:
//     lo_m   = min_k t'[m][k],  hi_m = max_k t'[m][k],  a_m = max_k |t[m][k]|
//     base   = sum_m lo_m - kAdcScreenF64 sum_m |lo_m|                 (a lower bound of the real sum of the minima)
//     E      = kAdcScreenRel M sum_m a_m + kAdcScreenAbs               (>= |v - R|: the f32 chain v of a row against
//                                                                       its real sum R, M - 1 rounded additions)
//     num    = thr' + E - base (+ the f64 slack kAdcScreenF64 (|thr'| + |base|)),   s = max(num / 254, kAdcScreenMinStep)
//     u[m][k] = min(255, floor((t'[m][k] - lo_m) / s (1 - kAdcScreenF64)))          (the u8 image)
//     U_lim  = min(65535, floor(num / s (1 + kAdcScreenF64))),   -1 when num <= 0
// so that lo_m + s u[m][k] <= t'[m][k] in the reals, saturated or not, and for a row with U = sum_m u[m][code m]
//     base + s U <= R,  hence  U > U_lim  =>  R > thr' + E  =>  v' > thr':  the row is PROVABLY OUTSIDE.
// Every other allowed row is returned.  With s = num / 254 a single entry 255 s above its minimum saturates and
// disqualifies its row alone.  A regular row is returned only while v' <= thr' + M s + 2 E (+ the f64 slack).
// A query the proof does not cover (a NaN or infinite entry, sum_m a_m > kAdcScreenMaxSum, a NaN threshold)
// gets U_lim = 65535: every allowed row.  Over finite tables a threshold of -Inf (ip: +Inf) returns nothing.
//
// Scaled inner products (value fl(v c), c = scales[row]).  The integer sum gives B - s U >= v with B = E - base, and the
// comparison needs the row's scale, so it is made per (row, query) in f32: w^ >= B - s32 U (an fma, widened by 2^-22 |w|
// + 2^-100; B rounded up, s32 = s rounded down), p = fl(w^ c) >= fl(v c) by the monotonicity of rounding for c >= 0, and
// the row is provably outside iff c is finite, c >= 0 and p < thr.  A negative, NaN or infinite scale is returned.  The
// step covers the values from thr / c_max (c_max: the largest finite scale, one reduction per call) up to the largest sum.
//
// Kernel.  The image of a pass sits in LDS as [M][K][NQ] bytes, interleaved by query: one ds_read_b128 brings a code's
// entries for 16 queries.  The sums are packed u16 and the bytes are never unpacked: per fetched dword w,
// acc_a += w and acc_h += w >> 8 (both per 16-bit lane, wrapping), and after the last m the even bytes' sums are
// acc_a - 256 acc_h mod 2^16, the odd bytes' acc_h: every true sum is <= 255 M <= 65,535 for M <= 257 (kAdcScreenMaxM = 100:
// what the row fetch serves).
// Units, order, passes are those of the range searches: the unit is a wave with a contiguous sub-range of its
// workgroup's rows (a multiple of 64), one row per lane; the count pass leaves one 64-bit hit word per (query, 64 rows)
// -- hits[query][word] -- and the unit's counts part[query][unit]; k_adc_range_scan turns them into first slots;
// k_adc_screen_fill walks the bitmap -- lane = query, words ascending, bits ascending -- and stores the row ids below
// `capacity`.  It does not read the codes.  A disallowed row and a row past n are never loaded.
#pragma once
#include "kernels_adc_range.hip.h"

namespace pqhip {

// the bound's constants; tests/adc_screen_ref.py states them again
constexpr double kAdcScreenRel = 0x1.01p-24;      // per addition of the f32 chain: gamma_(M-1) <= kAdcScreenRel M for M <= 257
constexpr double kAdcScreenAbs = 0x1p-100;        // additions that flush an f32 subnormal
constexpr double kAdcScreenF64 = 0x1p-40;         // the f64 arithmetic of the preparation, rounded in the safe direction
constexpr double kAdcScreenMaxSum = 0x1p126;      // sum_m max_k |t|: beyond it the f32 chain may overflow
constexpr double kAdcScreenMinStep = 0x1p-120;    // the step is never 0 and stays a normal f32
constexpr int kAdcScreenSteps = 254;              // U_lim of a query whose step is num / 254
constexpr int kAdcScreenMaxM = 4 * kAdcMaxValueWords;   // 100, the row fetch of the searches; the packed u16 sums hold to 257
static_assert(255 * kAdcScreenMaxM <= 65535, "the packed u16 sums must not wrap past their value");
constexpr int kAdcScreenKeepAll = 65535;          // U_lim of a query the proof does not cover
constexpr int kAdcScreenPerRow = -2;              // U_lim of a scaled query: the f32 epilogue decides

constexpr int kAsPrepThreads = 256;

struct AdcScreenPrm {      // one per query slot of a pass, behind the image
    int ulim;              // a row is returned iff U <= ulim (kAdcScreenPerRow: iff the epilogue does not prove it outside)
    float b, s, thr;       // the epilogue's B (rounded up), step (rounded down) and the caller's threshold
};

typedef unsigned short as_u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned as_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned as_u32x2 __attribute__((ext_vector_type(2)));

constexpr size_t adc_screen_image_bytes(int M, int K, int nq) { return ((size_t)M * K * nq + 15) / 16 * 16; }
constexpr size_t adc_screen_lds_bytes(int M, int K, int nq) { return adc_screen_image_bytes(M, K, nq) + (size_t)nq * sizeof(AdcScreenPrm); }

// the least f32 >= t resp. the greatest f32 <= t, for a finite t inside f32's normal range
__device__ __forceinline__ float adc_screen_f32_up(double t)
{
    float f = (float)t;
    if ((double)f < t) f = f > 0.f ? __uint_as_float(__float_as_uint(f) + 1u) : f < 0.f ? __uint_as_float(__float_as_uint(f) - 1u) : __uint_as_float(1u);
    return f;
}
__device__ __forceinline__ float adc_screen_f32_down(double t) { return -adc_screen_f32_up(-t); }

// The largest finite scale >= 0 of the call, as the bits of an f32 (they order like unsigned integers); *out starts at 0.
inline __global__ __launch_bounds__(256) void k_adc_screen_scale_max(const float* __restrict__ scales, int64_t n, unsigned* __restrict__ out)
{
    unsigned m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float c = scales[i];
        if (c >= 0.f && c < __builtin_inff()) {
            const unsigned b = __float_as_uint(c) & 0x7fffffffu;      // -0 counts as 0
            m = b > m ? b : m;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// The image and the parameters of one query slot, by one workgroup of kAsPrepThreads: the body of both prep kernels, so
// that a query has the same image and parameters wherever it is screened.  A slot that is not `real` is padding (zeros,
// nothing returned; tq and thr are then not dereferenced).  Wave w takes the subquantizers w, w + 4, ..; minima and
// maxima do not depend on the order.  The sums over m are one thread's, in ascending m.  Entry i = m K + k goes to
// dst[i dst_stride].  ET is the entry type and `levels` the value an entry saturates at, one step more than the steps
// num is cut into: uint8_t with kAdcScreenSteps + 1 = 255 here, uint16_t with floor(65,535 / M) in
// kernels_adc_screen16.hip.h; the arithmetic is the same expression for both.
// floor_sum (scaled mode only): null, or the least chain value that can still qualify, which ends the step's span in
// the place of thr / c_max (kernels_adc_screen_lists_residual.hip.h); cmax_bits is then not read.  -Inf
// or NaN: no floor, the step spans all sums.
template <typename ET>
__device__ __forceinline__ void adc_screen_prep_slot(const float* __restrict__ tq, bool real, int M, int K, const float* __restrict__ thr,
                                                     int ip, int scaled, const unsigned* __restrict__ cmax_bits, int levels,
                                                     ET* __restrict__ dst, size_t dst_stride, AdcScreenPrm* __restrict__ prm,
                                                     const double* floor_sum = nullptr)
{
    const double steps = (double)(levels - 1), sat = (double)levels;
    __shared__ float s_lo[kAdcScreenMaxM], s_hi[kAdcScreenMaxM], s_am[kAdcScreenMaxM];
    __shared__ int s_bad, s_live;
    __shared__ double s_step;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const float sg = ip ? -1.f : 1.f;
    const float inf = __builtin_inff();
    if (t == 0) { s_bad = 0; s_live = 0; s_step = 1.0; }
    __syncthreads();
    if (real) {
        for (int m = wave; m < M; m += kAsPrepThreads / 64) {
            float lo = inf, hi = -inf, am = 0.f;
            bool bad = false;
            for (int k = lane; k < K; k += 64) {
                const float v = sg * tq[(size_t)m * K + k];
                if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad = true;
                const float a = __builtin_fabsf(v);
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
                am = a > am ? a : am;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float l2 = __shfl_xor(lo, d), h2 = __shfl_xor(hi, d), a2 = __shfl_xor(am, d);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
                am = a2 > am ? a2 : am;
            }
            if (bad) s_bad = 1;
            if (lane == 0) { s_lo[m] = lo; s_hi[m] = hi; s_am[m] = am; }
        }
    }
    __syncthreads();
    if (t == 0) {
        AdcScreenPrm p{-1, 0.f, 0.f, real ? *thr : 0.f};
        if (real) {
            p.ulim = kAdcScreenKeepAll;
            double sum = 0.0, absum = 0.0, A = 0.0, spread = 0.0;
            for (int m = 0; m < M; ++m) {
                sum += (double)s_lo[m];
                absum += __builtin_fabs((double)s_lo[m]);
                A += (double)s_am[m];
                spread += (double)s_hi[m] - (double)s_lo[m];
            }
            const double th = (double)(sg * p.thr);
            // an infinite threshold needs no proof: nothing lies at or below -Inf, every number at or below +Inf; the
            // scaled form keeps its epilogue for +Inf, which fl(v c) reaches by overflow alone
            const bool thr_nan = p.thr != p.thr, thr_inf = !thr_nan && __builtin_fabsf(p.thr) == inf;
            if (!s_bad && !thr_nan && A <= kAdcScreenMaxSum && !scaled && thr_inf) {
                p.ulim = th < 0.0 ? -1 : kAdcScreenKeepAll;
            } else if (!s_bad && !thr_nan && A <= kAdcScreenMaxSum && !(scaled && p.thr == -inf)) {
                const double E = kAdcScreenRel * (double)M * A + kAdcScreenAbs;
                const double base = sum - kAdcScreenF64 * absum;
                if (!scaled) {
                    const double num = (th - base) + E + kAdcScreenF64 * (__builtin_fabs(th) + __builtin_fabs(base));
                    if (!(num > 0.0)) {
                        p.ulim = -1;                                // thr' + E < base: no row can qualify
                    } else {
                        const double step = num / steps > kAdcScreenMinStep ? num / steps : kAdcScreenMinStep;
                        const double lim = __builtin_floor(num / step * (1.0 + kAdcScreenF64));
                        p.ulim = lim < (double)kAdcScreenKeepAll ? (int)lim : kAdcScreenKeepAll;
                        s_step = step;
                        s_live = 1;
                    }
                } else {
                    const double B = (E - base) + kAdcScreenF64 * __builtin_fabs(base);
                    double num = spread + 2.0 * E;                  // the whole span of the sums
                    double least = -(double)inf;                    // the sums below it cannot qualify
                    if (floor_sum) {
                        least = *floor_sum;
                    } else {
                        const float cmax = __uint_as_float(*cmax_bits);
                        if (p.thr > 0.f && cmax > 0.f)              // fl(v c) >= thr needs v >= thr / c_max (1 - 2^-23)
                            least = (double)p.thr / (double)cmax * (1.0 - 0x1p-20);
                    }
                    if (least > -(double)inf) {
                        const double span = B - least;
                        num = span < num ? span : num;
                    }
                    const double step = num / steps > kAdcScreenMinStep ? num / steps : kAdcScreenMinStep;
                    p.ulim = kAdcScreenPerRow;
                    p.b = adc_screen_f32_up(B);
                    p.s = adc_screen_f32_down(step);
                    s_step = step;
                    s_live = 1;
                }
            }
        }
        *prm = p;
    }
    __syncthreads();
    const bool live = s_live != 0;
    const double step = s_step;
    const int MK = M * K;
    for (int i = t; i < MK; i += kAsPrepThreads) {
        ET u = 0;
        if (live) {
            const int m = i / K;
            const double x = (double)(sg * tq[i]) - (double)s_lo[m];
            const double qv = x / step * (1.0 - kAdcScreenF64);
            u = qv >= sat ? (ET)levels : (ET)(int)qv;
        }
        dst[(size_t)i * dst_stride] = u;
    }
}

// One query slot per workgroup, into the image of a pass: img [M][K][NQ] bytes, interleaved by query, prm [NQ]; slots
// >= nq_pass are padding.
inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_prep(const float* __restrict__ tables, int nq_pass, int M, int K, int NQ,
                                                                    const float* __restrict__ thr, int ip, int scaled,
                                                                    const unsigned* __restrict__ cmax_bits,
                                                                    uint8_t* __restrict__ img, AdcScreenPrm* __restrict__ prm)
{
    const int slot = blockIdx.x;
    adc_screen_prep_slot(tables + (size_t)slot * M * K, slot < nq_pass, M, K, thr + slot, ip, scaled, cmax_bits, kAdcScreenSteps + 1,
                         img + slot, (size_t)NQ, prm + slot);
}

template <int ND>
__device__ __forceinline__ void adc_screen_entry(const uint8_t* p, unsigned (&d)[ND])
{
    if constexpr (ND == 8) {
        const as_u32x4 a = *reinterpret_cast<const as_u32x4*>(p), b = *reinterpret_cast<const as_u32x4*>(p + 16);
        d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3]; d[4] = b[0]; d[5] = b[1]; d[6] = b[2]; d[7] = b[3];
    } else if constexpr (ND == 4) {
        const as_u32x4 a = *reinterpret_cast<const as_u32x4*>(p);
        d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3];
    } else if constexpr (ND == 2) {
        const as_u32x2 a = *reinterpret_cast<const as_u32x2*>(p);
        d[0] = a[0]; d[1] = a[1];
    } else {
        d[0] = *reinterpret_cast<const unsigned*>(p);
    }
}

// The integer sums of one row (fetched by adc_fetch_row, shift sh = a & 3) against the interleaved image lm [M][K][4 ND]
// in LDS, KQ = 4 ND K: per dword j of an entry the packed u16 sums of its bytes 0, 2 (even[j]) and 1, 3 (odd[j]).  A code
// >= K sets `bad` and reads entry 0.  The count passes of the exhaustive and of the list screen share it.
template <int NV, int ND>
__device__ __forceinline__ void adc_screen_row_sums(const unsigned (&w)[NV + 1], unsigned sh, const uint8_t* lm, int M, int K, int KQ,
                                                    bool& bad, unsigned (&even)[ND], unsigned (&odd)[ND])
{
    as_u16x2 acc_a[ND], acc_h[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) { acc_a[j] = (as_u16x2){0, 0}; acc_h[j] = (as_u16x2){0, 0}; }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);   // bytes 4k .. 4k+3 of the row
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * k + e < M) {
                unsigned c = (v >> (8 * e)) & 0xffu;
                if (c >= (unsigned)K) { bad = true; c = 0; }
                unsigned d[ND];
                adc_screen_entry<ND>(lm + c * (4 * ND), d);
#pragma unroll
                for (int j = 0; j < ND; ++j) {
                    const as_u16x2 x = __builtin_bit_cast(as_u16x2, d[j]);
                    acc_a[j] += x;
                    acc_h[j] += x >> (as_u16x2){8, 8};
                }
                lm += KQ;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        even[j] = __builtin_bit_cast(unsigned, (as_u16x2)(acc_a[j] - (acc_h[j] << (as_u16x2){8, 8})));
        odd[j] = __builtin_bit_cast(unsigned, acc_h[j]);
    }
}

// U of query slot q (a constant after unrolling) from the packed sums
template <int ND>
__device__ __forceinline__ int adc_screen_sum_of(const unsigned (&even)[ND], const unsigned (&odd)[ND], int q)
{
    const unsigned pair = (q & 1) ? odd[q >> 2] : even[q >> 2];
    return (int)((q & 2) ? pair >> 16 : pair & 0xffffu);
}

// The f32 upper bound of the chain of a row with integer sum U: B - s32 U by one fma, widened by 2^-22 |w| + 2^-100.
// Non-increasing in U.
__device__ __forceinline__ float adc_screen_chain_bound(int U, const AdcScreenPrm& p)
{
    const float wv = __builtin_fmaf(-p.s, (float)U, p.b);
    return fadd(__builtin_fmaf(__builtin_fabsf(wv), 0x1p-22f, wv), 0x1p-100f);
}

// Is a row with integer sum U and scale sc returned for the query of p?  (p is wave-uniform.)
__device__ __forceinline__ bool adc_screen_keep(int U, const AdcScreenPrm& p, float sc)
{
    bool keep = U <= p.ulim;
    if (p.ulim == kAdcScreenPerRow) {
        const float wu = adc_screen_chain_bound(U, p);
        const float pv = fmul(wu, sc);
        keep = !(sc >= 0.f && sc < __builtin_inff() && pv < p.thr);   // NaN anywhere: not proved, returned
    }
    return keep;
}

// The count pass, NQ query slots per pass.  Workgroup b owns rows [b rows_per_wg, (b + 1) rows_per_wg) (rows_per_wg a
// multiple of 1,024), its wave w the sub-range [w rows_per_wg / 16, (w + 1) rows_per_wg / 16): unit u = 16 b + w.
// img: the pass's image and parameters (16-byte aligned).  part [nq_pass][units] and hits [NQ][words] out
// (words = ceil(n / 64)); every word of the unit's rows is written.  scales null: no epilogue.
template <int NV, int NQ>
__global__ __launch_bounds__(1024) void k_adc_screen_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                        const uint32_t* __restrict__ allow /* or null */,
                                                        const float* __restrict__ scales /* [n] or null */,
                                                        const uint8_t* __restrict__ img, int M, int K, int64_t rows_per_wg,
                                                        int nq_pass, int64_t words, int64_t* __restrict__ part,
                                                        unsigned long long* __restrict__ hits, int* __restrict__ err)
{
    static_assert(NQ == 4 || NQ == 8 || NQ == 16 || NQ == 32, "query slots per pass");
    constexpr int NW = NV + 1, ND = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_u[];
    const int img_bytes = (int)adc_screen_image_bytes(M, K, NQ);
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
    const int KQ = K * NQ;
    int64_t cnt = 0;                                                // lane q < nq_pass: the unit's hits of query q
    bool bad = false;
    for (int64_t b0 = row_begin; b0 < row_end; b0 += 64) {          // wave-uniform: the ballots are wave-wide
        const int64_t row = b0 + lane;
        bool valid = row < row_end;
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        unsigned even[ND], odd[ND];                                 // per dword of an entry: the packed u16 sums of its bytes 0, 2 / 1, 3
#pragma unroll
        for (int j = 0; j < ND; ++j) { even[j] = 0u; odd[j] = 0u; }
        float sc = 1.f;
        if (valid) {
            if (scales) sc = scales[row];                           // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            adc_screen_row_sums<NV, ND>(w, (unsigned)(a & 3), lds_u, M, K, KQ, bad, even, odd);
        }
        unsigned long long mine = 0ull;                             // lane q: the hit word of query q
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bool keep = adc_screen_keep(adc_screen_sum_of<ND>(even, odd, q), prm[q], sc);
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

// The fill pass: the decomposition of the count pass, lane = query of the pass, the unit's words in ascending order, a
// word's bits in ascending order.  part: the first slot of every (query, unit), absolute.
inline __global__ __launch_bounds__(1024) void k_adc_screen_fill(const unsigned long long* __restrict__ hits, int64_t words, int nq_pass,
                                                          int64_t n, int64_t rows_per_wg, const int64_t* __restrict__ part,
                                                          int64_t capacity, int64_t* __restrict__ out_i)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t sub = rows_per_wg / kRangeWaves;
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    if (lane >= nq_pass) return;                                    // no cross-lane step below
    int64_t slot = part[(int64_t)lane * units + unit];
    for (int64_t b0 = row_begin; b0 < row_end; b0 += 64) {
        unsigned long long w = hits[(int64_t)lane * words + (b0 >> 6)];
        while (w) {
            const int b = __builtin_ctzll(w);
            w &= w - 1;
            if (slot < capacity) out_i[slot] = b0 + b;
            ++slot;
        }
    }
}

}  // namespace pqhip
