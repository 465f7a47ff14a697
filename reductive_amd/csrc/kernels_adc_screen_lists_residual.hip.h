// kernels_adc_screen_lists_residual.hip.h -- the u8 table screen of kernels_adc_screen_lists.hip.h over RESIDUAL codes
// in probed lists (include/pqhip.h: pqhip_adc_screen_lists_residual_f32_dev; DESIGN.md §5h has the bound and its proof).
// Per query it returns a superset of what pqhip_adc_range_lists_residual_f32_dev (IP = false) resp.
// pqhip_adc_ip_range_lists_residual_f32_dev (IP = true, the same scales) returns at the same thresholds, as positions in
// that call's order.  Only u8 images: a 16-bit image and 4-bit packed codes are not served here.
// (Instantiated by pqhip_adc_screen_lists_residual.hip.)
//
// The value of a (row i, query q, probe slot p) is not a table sum:
//     dist = fl(fl(bias[q][p] + term[i]) - fl(s + s))          score = fl(fl(bias[q][p] + s) scale[i])
// with s the f32 chain over the query's INNER-PRODUCT table, so no integer limit per query decides a row.
//
// Screening value.  The image of a query is the existing one of the NEGATED table in the scaled mode of
// adc_screen_prep_slot: (B, s32) with  w = adc_screen_chain_bound(U) >= s  for every row, saturated or not (§5e).  Every
// operation of the two formulas is one rounded f32 operation, hence monotone in each operand, so
//     lower = fl(fl(bias + term) - fl(w + w)) <= dist           upper = fl(fl(bias + w) scale) >= score  (0 <= scale < Inf)
// and a row is left out iff  lower > thr  resp.  upper < thr  (adc_screen_res_outside).  A NaN anywhere makes the
// comparison false: the row is returned, as is a row with a negative, NaN or infinite scale, and a query whose tables
// the proof does not cover (kAdcScreenKeepAll from the prep: a NaN or infinite entry, sums beyond 2^126, a NaN threshold).
//
// The step.  Sums that can still qualify start at a per-query floor (k_adc_screen_lists_residual_prep):
//     IP = false:  (min_p bias[q][p] + min_i term[i] - thr) / 2         IP = true:  thr / c_max - max_p bias[q][p]
// over the query's valid slots and the call's rows (c_max = 1 without scales; with scales only for thr >= 2^-100),
// lowered by 2^-19 of the magnitudes involved + 2^-98, so that a row with a saturated entry (w <= floor - step) is
// provably outside in f32 as well.  The step is (B - floor) / 254, never more than the whole span of the sums.
// Tightness: a regular row is returned only while, with G = M step + 2 E (E of §5e) + 2^-39 (|thr| + |base|) +
// 2^-22 (|B| + 255 step) (the roundings of B and s32 U),
//     dist - thr <= 2 G + 2^-20 (|bias + term| + 2 |s| + 2 G)      resp.      thr - score <= (G + 2^-20 (|bias| + |s| + G)) scale.
//
// Kernels.  Inversion, units, groups and the byte-transpose staging are those of k_adc_screen_lists.  The count pass
// stages beside a slot's parameters its bias and an INTEGER LIMIT: the largest U at which the epilogue, evaluated with
// the call-wide least term resp. largest scale, does not prove a row outside (adc_screen_res_limit: a bisection over the
// epilogue itself, which is monotone in U and in the term).  A row's term or scale is loaded with its code words.  Per
// (wave step, slot) one ballot asks whether any lane is at or under the limit (or carries a NaN term / a bad scale);
// if none, the f32 epilogue is skipped -- it would have answered "outside" in every lane.  The fill pass forms the
// words of a pair beyond the budget again with the same predicate.
#pragma once
#include "kernels_adc_screen_lists.hip.h"

namespace pqhip {

// dynamic LDS of the count pass: that of k_adc_screen_lists, then per slot the bias (4) and the integer limit (4)
constexpr size_t adc_screen_lists_residual_lds_bytes(int M, int K, int nq) { return adc_screen_lists_lds_bytes(M, K, nq) + (size_t)nq * 8; }

// the bits of an f32 as an int that orders like the value (its own inverse); -0 sorts below +0
__device__ __forceinline__ int adc_screen_f32_key(float v)
{
    const int b = __float_as_int(v);
    return b < 0 ? b ^ 0x7fffffff : b;
}
__device__ __forceinline__ float adc_screen_key_f32(int k) { return __int_as_float(k < 0 ? k ^ 0x7fffffff : k); }

// The least non-NaN row term of the call, as a key; *out starts at the key of +Inf.
inline __global__ __launch_bounds__(256) void k_adc_screen_term_min(const float* __restrict__ terms, int64_t n, int* __restrict__ out)
{
    int m = 0x7f800000;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = terms[i];
        if (v == v) {
            const int k = adc_screen_f32_key(v);
            m = k < m ? k : m;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(m, d);
        m = o < m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(out, m);
}

// Is the row with integer sum U provably outside for the slot (p, bias)?  x: the row's term (IP false) resp. its scale
// (IP true; 1 without scales, which multiplies exactly).  The numpy model of tests/adc_screen_residual_ref.py states it again.
template <bool IP>
__device__ __forceinline__ bool adc_screen_res_outside(int U, const AdcScreenPrm& p, float bias, float x)
{
    const float w = adc_screen_chain_bound(U, p);
    if constexpr (IP) return x >= 0.f && x < __builtin_inff() && fmul(fadd(bias, w), x) < p.thr;
    else return fsub(fadd(bias, x), fadd(w, w)) > p.thr;
}

template <bool IP>
__device__ __forceinline__ bool adc_screen_res_keep(int U, const AdcScreenPrm& p, float bias, float x)
{
    return p.ulim == kAdcScreenKeepAll || (p.ulim == kAdcScreenPerRow && !adc_screen_res_outside<IP>(U, p, bias, x));
}

// The largest U in [-1, 255 M] that the epilogue does not prove outside for EVERY row of the call: above it the
// epilogue answers "outside" whatever the row's term >= tmin resp. scale in [0, cmax] is (a NaN term and a bad scale
// are the caller's `special` lanes).  By bisection over the predicate itself, which is monotone in U: w does not
// increase with U, and each f32 operation is monotone.  One thread per slot runs it -- at most 15 evaluations -- each time
// a (list, group) is staged, while the rest of the workgroup waits at the barrier; what that costs has not been measured.
template <bool IP>
__device__ __forceinline__ int adc_screen_res_limit(const AdcScreenPrm& p, float bias, float tmin, float cmax, bool scaled, int M)
{
    if (p.ulim != kAdcScreenPerRow) return p.ulim == kAdcScreenKeepAll ? kAdcScreenKeepAll : -1;
    int lo = -1, hi = 255 * M + 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        bool out;
        if constexpr (IP) {
            if (scaled) {                                           // y c <= max(0, y cmax); -Inf times a zero scale is a NaN: returned
                const float y = fadd(bias, adc_screen_chain_bound(mid, p));
                out = p.thr > 0.f && y > -__builtin_inff() && (y <= 0.f || fmul(y, cmax) < p.thr);
            } else {
                out = adc_screen_res_outside<true>(mid, p, bias, 1.f);
            }
        } else {
            out = adc_screen_res_outside<false>(mid, p, bias, tmin);
        }
        if (out) hi = mid; else lo = mid;
    }
    return lo;
}

// a lane whose row the limit must not skip: the epilogue returns it whatever U is
template <bool IP>
__device__ __forceinline__ bool adc_screen_res_special(float x)
{
    if constexpr (IP) return !(x >= 0.f && x < __builtin_inff());
    else return x != x;
}

// Preparation: one workgroup per query of the chunk.  The extreme bias over the query's valid slots (a slot is valid
// iff its list id is in range and the list has rows; a NaN bias is passed over) and the call-wide values ext[0] (the
// largest scale, bits) / ext[1] (the least term, key) give the floor; the image and parameters are adc_screen_prep_slot's
// of the negated table in its scaled mode.
inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_lists_residual_prep(
    const float* __restrict__ tables, int M, int K, const float* __restrict__ thr, int ip, int scaled, const int* __restrict__ ext,
    const int64_t* __restrict__ list_off, int64_t n_lists, int64_t n, const int64_t* __restrict__ probes, int n_probe, int64_t p_rs,
    const float* __restrict__ bias, int64_t b_rs, uint8_t* __restrict__ imgq, int64_t pitch, AdcScreenPrm* __restrict__ prm)
{
    __shared__ float s_red[kAsPrepThreads / 64];
    __shared__ double s_floor;
    __shared__ float s_thr;
    const int64_t q = blockIdx.x;
    const float inf = __builtin_inff();
    float e = inf;                                                  // min of bias (ip: of -bias)
    for (int j = threadIdx.x; j < n_probe; j += kAsPrepThreads) {
        const int64_t l = probes[q * p_rs + j];
        if (l >= 0 && l < n_lists) {
            const FslRange r = fsl_list_range(list_off, l, n);
            if (r.hi > r.lo) {
                const float b = bias[q * b_rs + j];
                const float v = ip ? -b : b;
                e = v < e ? v : e;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(e, d);
        e = o < e ? o : e;
    }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kAsPrepThreads / 64; ++w) e = s_red[w] < e ? s_red[w] : e;
        // a distance threshold of -Inf is screened at the least finite f32: still a superset, and nearly nothing of it
        s_thr = !ip && thr[q] == -inf ? -0x1.fffffep127f : thr[q];
        const double th = (double)s_thr;
        double fr, mag;
        if (!ip) {
            const double mb = (double)e, mt = (double)adc_screen_key_f32(ext[1]);
            fr = (mb + mt - th) * 0.5;
            mag = __builtin_fabs(mb) + __builtin_fabs(mt) + __builtin_fabs(th);
        } else {
            const double mb = -(double)e;
            double t = th;
            bool ok = true;
            if (scaled) {
                const double cmax = (double)__int_as_float(ext[0]);
                ok = th >= 0x1p-100 && cmax > 0.0;
                t = ok ? th / cmax : 0.0;
            }
            fr = ok ? t - mb : -(double)inf;
            mag = __builtin_fabs(t) + __builtin_fabs(mb);
        }
        s_floor = fr - 0x1p-19 * mag - 0x1p-98;
    }
    __syncthreads();
    adc_screen_prep_slot(tables + (size_t)q * M * K, true, M, K, &s_thr, 1, 1, (const unsigned*)nullptr, kAdcScreenSteps + 1,
                         imgq + q * pitch, (size_t)1, prm + q, &s_floor);
}

// The count pass: k_adc_screen_lists with the slot's bias and limit staged beside its parameters and the f32 epilogue
// per (row, pair).  xrow: the row terms (IP false) resp. the scales or null (IP true).  bias_g [queries][b_rs]: the
// chunk's probe biases; entry e = q n_probe + p has bias_g[q b_rs + p].
template <int NV, int NQ, bool IP>
__global__ __launch_bounds__(1024) void k_adc_screen_lists_residual(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow /* or null */,
    const float* __restrict__ xrow, const float* __restrict__ bias_g, int64_t b_rs, const int* __restrict__ ext,
    const int64_t* __restrict__ list_off, int64_t n_lists, const unsigned* __restrict__ lcnt, const unsigned* __restrict__ pair_off,
    const int64_t* __restrict__ unit_off, const unsigned* __restrict__ pairs, int n_probe, const uint8_t* __restrict__ imgq,
    int64_t pitch, const AdcScreenPrm* __restrict__ prm_g, int M, int K, int64_t unit_rows, const int64_t* __restrict__ hoff,
    int64_t budget, uint32_t* __restrict__ hits, unsigned long long* __restrict__ cnt, int* __restrict__ err)
{
    static_assert(NQ == 4 || NQ == 8 || NQ == 16 || NQ == 32, "query slots per group");
    constexpr int NW = NV + 1, ND = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_u[];
    const int MK = M * K, KQ = K * NQ;
    AdcScreenPrm* prm = reinterpret_cast<AdcScreenPrm*>(lds_u + adc_screen_image_bytes(M, K, NQ));
    int64_t* s_hb = reinterpret_cast<int64_t*>(prm + NQ);
    int* s_e = reinterpret_cast<int*>(s_hb + NQ);
    int* s_qn = s_e + NQ;
    float* s_bias = reinterpret_cast<float*>(s_qn + NQ);
    int* s_lim = reinterpret_cast<int*>(s_bias + NQ);
    int64_t* s_list = reinterpret_cast<int64_t*>(s_lim + NQ);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    const int64_t total = unit_off[n_lists];
    int64_t held_l = -1, held_g = -1;                               // the (list, group) whose image the LDS holds
    bool bad = false;
    for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
        __syncthreads();                                            // the previous unit is done with the LDS
        if (threadIdx.x == 0) {                                     // the largest l with unit_off[l] <= u
            int64_t a = 0, b = n_lists;
            while (b - a > 1) {
                const int64_t mid = (a + b) >> 1;
                if (unit_off[mid] <= u) a = mid; else b = mid;
            }
            *s_list = a;
        }
        __syncthreads();
        const int64_t l = range_uniform(*s_list);
        const FslRange r = fsl_list_range(list_off, l, n);
        const int64_t chunks = (r.hi - r.lo + unit_rows - 1) / unit_rows;
        const int64_t local = u - unit_off[l];
        const int64_t g = local / chunks, ci = local - g * chunks;
        const int np = __builtin_amdgcn_readfirstlane((int)((int64_t)lcnt[l] - g * NQ < NQ ? (int64_t)lcnt[l] - g * NQ : NQ));
        const int64_t list_tiles = (r.hi - r.lo + kFsTile - 1) / kFsTile;
        if (l != held_l || g != held_g) {                           // workgroup-uniform
            if (threadIdx.x < NQ) {
                const int j = threadIdx.x;
                if (j < np) {
                    const unsigned e = pairs[pair_off[l] + g * NQ + j];
                    const int qn = (int)(e / (unsigned)n_probe);
                    const AdcScreenPrm p = prm_g[qn];
                    const float b = bias_g[(int64_t)qn * b_rs + (int64_t)(e - (unsigned)qn * (unsigned)n_probe)];
                    prm[j] = p;
                    s_hb[j] = hoff[e];
                    s_e[j] = (int)e;
                    s_qn[j] = qn;
                    s_bias[j] = b;
                    s_lim[j] = adc_screen_res_limit<IP>(p, b, adc_screen_key_f32(ext[1]), __int_as_float(ext[0]), IP && xrow != nullptr, M);
                } else {
                    prm[j] = AdcScreenPrm{-1, 0.f, 0.f, 0.f};
                    s_hb[j] = budget;
                    s_e[j] = -1;
                    s_qn[j] = -1;
                    s_bias[j] = 0.f;
                    s_lim[j] = -1;
                }
            }
            __syncthreads();
            adc_screen_lists_stage<NQ>(lds_u, imgq, pitch, MK, s_qn);
            __syncthreads();
            held_l = l;
            held_g = g;
        }
        const int64_t rb = r.lo + ci * unit_rows;
        const int64_t re = rb + unit_rows < r.hi ? rb + unit_rows : r.hi;
        unsigned long long cn = 0ull;                               // lane q < np: the unit's hits of pair q
        for (int64_t row0 = rb + (int64_t)wave * 64; row0 < re; row0 += 64 * kRangeWaves) {   // wave-uniform
            const unsigned long long bits = adc_screen_lists_step_bits(allow, row0, re, n);
            const bool valid = (bits >> lane) & 1ull;
            unsigned even[ND], odd[ND];
#pragma unroll
            for (int j = 0; j < ND; ++j) { even[j] = 0u; odd[j] = 0u; }
            float x = IP ? 1.f : 0.f;
            if (valid) {                                            // a disallowed row and a row past the end load nothing
                const int64_t row = row0 + lane;
                if (xrow) x = xrow[row];                            // issued with the row's code words
                const uintptr_t a = lo + (uintptr_t)(row * c_rs);
                unsigned w[NW];
                adc_fetch_row<NW>(a, lo, hi, M, w);
                adc_screen_row_sums<NV, ND>(w, (unsigned)(a & 3), lds_u, M, K, KQ, bad, even, odd);
            }
            const bool special = adc_screen_res_special<IP>(x);
            unsigned long long mine = 0ull;                         // lane q: the hit word of pair q
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int U = adc_screen_sum_of<ND>(even, odd, q);
                const bool cand = valid && (U <= s_lim[q] || special);
                unsigned long long bl = 0ull;
                if (__ballot(cand) != 0ull)                         // wave-uniform: no lane at or under the slot's limit, no epilogue
                    bl = __ballot(cand && adc_screen_res_keep<IP>(U, prm[q], s_bias[q], x));
                if (lane == q) mine = bl;
            }
            if (lane < np) {                                        // a padding slot has no hits
                const int64_t hb = s_hb[lane];
                const int64_t tile = (row0 - r.lo) >> 5;            // even: units and steps start at multiples of 64
                if (hb + list_tiles <= budget) {
                    hits[hb + tile] = (unsigned)mine;
                    if (tile + 1 < list_tiles) hits[hb + tile + 1] = (unsigned)(mine >> 32);
                }
                cn += (unsigned long long)__popcll(mine);
            }
        }
        if (lane < np && cn != 0ull) atomicAdd(&cnt[s_e[lane]], cn);
    }
    if (bad) atomicOr(err, 1);
}

// The fill pass: that of k_adc_screen_lists; a pair without stored words is formed again with the residual predicate.
template <bool IP>
__global__ __launch_bounds__(64 * kRangeWaves) void k_adc_screen_lists_residual_fill(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow, const float* __restrict__ xrow,
    const float* __restrict__ bias_g, int64_t b_rs, const int64_t* __restrict__ list_off, int64_t n_lists,
    const int64_t* __restrict__ probes, int n_probe, int64_t p_rs, int64_t nq, const uint8_t* __restrict__ imgq, int64_t pitch,
    const AdcScreenPrm* __restrict__ prm_g, int M, int K, const int64_t* __restrict__ hoff, int64_t budget,
    const uint32_t* __restrict__ hits, const int64_t* __restrict__ first, int64_t capacity, int64_t* __restrict__ out_i)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    for (int64_t e = (int64_t)blockIdx.x * kRangeWaves + wave; e < nq * n_probe; e += (int64_t)gridDim.x * kRangeWaves) {   // wave-uniform
        const int64_t q = e / n_probe;
        const int64_t l = probes[q * p_rs + (e - q * n_probe)];
        if (l < 0 || l >= n_lists) continue;
        const FslRange r = fsl_list_range(list_off, l, n);
        if (r.hi <= r.lo) continue;
        const int64_t list_tiles = (r.hi - r.lo + kFsTile - 1) / kFsTile;
        const int64_t hb = hoff[e];
        int64_t run = first[e];
        if (hb + list_tiles <= budget) {
            adc_screen_lists_emit_words(hits, hb, list_tiles, r.lo, run, capacity, out_i, lane);
        } else {                                                    // no stored words: form them again, this query alone
            const AdcScreenPrm p = prm_g[q];
            const float b = bias_g[q * b_rs + (e - q * n_probe)];
            const uint8_t* iq = imgq + q * pitch;
            for (int64_t row0 = r.lo; row0 < r.hi; row0 += 64) {
                const unsigned long long bits = adc_screen_lists_step_bits(allow, row0, r.hi, n);
                const bool valid = (bits >> lane) & 1ull;
                const int64_t row = row0 + lane;
                int U = 0;
                float x = IP ? 1.f : 0.f;
                if (valid) {
                    if (xrow) x = xrow[row];
                    const uint8_t* cr = codes + row * c_rs;         // row < n: bytes 0 .. M - 1 lie inside the matrix
                    for (int m = 0; m < M; ++m) {
                        unsigned c = cr[m];
                        if (c >= (unsigned)K) c = 0;                // the count pass raised the flag
                        U += (int)iq[m * K + c];
                    }
                }
                const bool hit = valid && adc_screen_res_keep<IP>(U, p, b, x);
                const unsigned long long bl = __ballot(hit);
                if (hit) {
                    const int64_t slot = run + (int64_t)range_rank(bl);
                    if (slot < capacity) out_i[slot] = row;
                }
                run += (int64_t)__popcll(bl);
            }
        }
    }
}

}  // namespace pqhip
