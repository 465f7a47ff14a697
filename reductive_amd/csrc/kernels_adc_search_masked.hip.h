// kernels_adc_search_masked.hip.h -- the four search producers with a row mask, and the kernel that packs one.
// (Launched from exactly one translation unit, pqhip_adc_masked.hip.)
//
// A mask is ceil(n / 32) words in the row order of the code matrix; bit i & 31 of word i >> 5 set means that row i may
// be returned.  The result is the unmasked search's on the matrix with every row whose bit is clear removed, indices
// mapped back: the order (key, row) is strict, so leaving rows out of the selection is all a filter has to do.  In every
// producer the bit is one more term of the `valid` that SearchState::offer already takes, formed BEFORE the code fetch:
// the word is loaded when, and only when, the lane's row is in range (so bits at or beyond n are never looked at and no
// word past ceil(n / 32) is read), and a row whose bit is clear loads no code, scale, row term or bias and cannot raise
// the range flag.  The 64 rows of a wave are consecutive in the exhaustive producers (row ranges start on multiples of
// 1,024), so a wave reads two mask words per trip, 1/8 byte per row; in the list producers a wave's rows are consecutive
// inside a list.  The trip count does not depend on the mask (offer is wave-wide).  Everything from offer on is shared:
// search_finish, k_adc_search_merge / k_adc_ip_search_merge and k_adc_lists_plan run unchanged.
// The bodies are restated here rather than reached through a template flag of the unmasked kernels, so that those keep
// their code objects instruction for instruction.
#pragma once
#include "kernels_adc_search.hip.h"

namespace pqhip {

__device__ __forceinline__ bool mask_bit(const uint32_t* __restrict__ allow, int64_t row)
{
    return (allow[row >> 5] >> ((unsigned)row & 31u)) & 1u;
}

// k_adc_search_u8 with a mask: same LDS layout, row ranges and selection
template <int NV, int NQ, int L>
__global__ __launch_bounds__(1024) void k_adc_search_masked_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                               const uint32_t* __restrict__ allow,
                                                               const float* __restrict__ lut /* [NQ][M][K] */, int M, int K,
                                                               int kk, int64_t rows_per_wg, unsigned* __restrict__ part_k,
                                                               uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    static_assert(NQ == 1 || NQ == 4 || NQ == 8, "queries per pass");
    constexpr int NW = NV + 1, NH = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    if (NQ == 1) {
        for (int i = threadIdx.x; i < MK; i += 1024) lds_s[i] = lut[i];
    } else {
        for (int i = threadIdx.x; i < NQ * MK; i += 1024) {
            const int q = i / MK, r = i - q * MK;
            lds_s[((q >> 2) * MK + r) * 4 + (q & 3)] = lut[i];
        }
    }
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + NQ * MK);   // [16][NQ][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * NQ * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = row_begin; base < row_end; base += 1024) {  // wave-uniform trip count: the selection is wave-wide
        const int64_t row = base + threadIdx.x;
        bool valid = row < row_end;
        if (valid) valid = mask_bit(allow, row);                    // before the fetch: a disallowed row is not read
        float dist[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) dist[q] = 0.f;
        if (valid) {
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            if constexpr (NQ == 1) {
                dist[0] = adc_row_sum<NV>(w, sh, lds_s, M, K, bad);
            } else {
                f32x2 s[NH][2];
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) { s[hq][0] = (f32x2){0.f, 0.f}; s[hq][1] = (f32x2){0.f, 0.f}; }
                adc_row_sum_mq<NV, NH>(w, sh, lds_s, M, K, MK, bad, s);
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) {
                    dist[4 * hq + 0] = s[hq][0][0];
                    dist[4 * hq + 1] = s[hq][0][1];
                    dist[4 * hq + 2] = s[hq][1][0];
                    dist[4 * hq + 3] = s[hq][1][1];
                }
            }
        }
        const unsigned off = (unsigned)(row - row_begin);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            st[q].offer(dist[q], off, valid, qk + (wave * NQ + q) * kSearchQueue, qi + (wave * NQ + q) * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<NQ, L>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), row_begin, part_k, part_i);
}

// k_adc_ip_search_u8 with a mask: the scale of a disallowed row is not loaded either
template <int NV, int NQ, int L>
__global__ __launch_bounds__(1024) void k_adc_ip_search_masked_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                                  const uint32_t* __restrict__ allow,
                                                                  const float* __restrict__ lut /* [NQ][M][K] */,
                                                                  const float* __restrict__ scales /* [n] or null */, int M,
                                                                  int K, int kk, int64_t rows_per_wg,
                                                                  unsigned* __restrict__ part_k, uint64_t* __restrict__ part_i,
                                                                  int* __restrict__ err)
{
    static_assert(NQ == 1 || NQ == 4 || NQ == 8, "queries per pass");
    constexpr int NW = NV + 1, NH = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    if (NQ == 1) {
        for (int i = threadIdx.x; i < MK; i += 1024) lds_s[i] = lut[i];
    } else {
        for (int i = threadIdx.x; i < NQ * MK; i += 1024) {
            const int q = i / MK, r = i - q * MK;
            lds_s[((q >> 2) * MK + r) * 4 + (q & 3)] = lut[i];
        }
    }
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + NQ * MK);   // [16][NQ][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * NQ * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = row_begin; base < row_end; base += 1024) {  // wave-uniform trip count: the selection is wave-wide
        const int64_t row = base + threadIdx.x;
        bool valid = row < row_end;
        if (valid) valid = mask_bit(allow, row);                    // before the fetch: a disallowed row is not read
        float neg[NQ];                                              // -score per query
#pragma unroll
        for (int q = 0; q < NQ; ++q) neg[q] = 0.f;
        if (valid) {
            const float sc = scales ? scales[row] : 1.f;
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            if constexpr (NQ == 1) {
                neg[0] = -fmul(adc_row_sum<NV>(w, sh, lds_s, M, K, bad), sc);
            } else {
                f32x2 s[NH][2];
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) { s[hq][0] = (f32x2){0.f, 0.f}; s[hq][1] = (f32x2){0.f, 0.f}; }
                adc_row_sum_mq<NV, NH>(w, sh, lds_s, M, K, MK, bad, s);
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) {
                    neg[4 * hq + 0] = -fmul(s[hq][0][0], sc);
                    neg[4 * hq + 1] = -fmul(s[hq][0][1], sc);
                    neg[4 * hq + 2] = -fmul(s[hq][1][0], sc);
                    neg[4 * hq + 3] = -fmul(s[hq][1][1], sc);
                }
            }
        }
        const unsigned off = (unsigned)(row - row_begin);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            st[q].offer(neg[q], off, valid, qk + (wave * NQ + q) * kSearchQueue, qi + (wave * NQ + q) * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<NQ, L>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), row_begin, part_k, part_i);
}

// k_adc_search_lists_u8 with a mask (positions: the mask is in the row order of the partitioned matrix)
template <bool IP, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_search_lists_masked_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                                     const uint32_t* __restrict__ allow,
                                                                     const float* __restrict__ lut,
                                                                     const float* __restrict__ scales /* IP: [n] or null */,
                                                                     int M, int K, int kk, const int64_t* __restrict__ seg_begin,
                                                                     const int64_t* __restrict__ seg_cum, int n_probe,
                                                                     unsigned* __restrict__ part_k, uint64_t* __restrict__ part_i,
                                                                     int* __restrict__ err)
{
    constexpr int NW = NV + 1;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    const float* tab = lut + (size_t)blockIdx.y * MK;
    for (int i = threadIdx.x; i < MK; i += 1024) lds_s[i] = tab[i];
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + MK);        // [16][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[1];
    st[0].init();
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const int64_t total = sc[n_probe];
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t s0 = (int64_t)blockIdx.x * per < total ? (int64_t)blockIdx.x * per : total;
    const int64_t s1 = s0 + per < total ? s0 + per : total;
    // the segment that holds place s0: the first j with seg_cum[j + 1] > s0 (it exists while s0 < T)
    int j = 0;
    if (s0 < s1) {
        int lo_j = 0, hi_j = n_probe - 1;
        while (lo_j < hi_j) {
            const int mid = (lo_j + hi_j) >> 1;
            if (sc[mid + 1] > s0) hi_j = mid; else lo_j = mid + 1;
        }
        j = lo_j;
    }
    int64_t seg_end = sc[j + 1];
    int64_t delta = sb[j] - sc[j];                                  // row = place + delta inside segment j
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = s0; base < s1; base += 1024) {              // wave-uniform trip count: the selection is wave-wide
        const int64_t c = base + threadIdx.x;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            while (c >= seg_end && j + 1 < n_probe) {               // places < T end inside some segment
                ++j;
                seg_end = sc[j + 1];
                delta = sb[j] - sc[j];
            }
            row = c + delta;
            valid = (uint64_t)row < (uint64_t)n;                    // holds by construction of the plan
        }
        if (valid) valid = mask_bit(allow, row);                    // before the fetch: a disallowed row is not read
        if (valid) {
            float sc = 1.f;
            if constexpr (IP) sc = scales ? scales[row] : 1.f;      // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            v = adc_row_sum<NV>(w, sh, lds_s, M, K, bad);
            if constexpr (IP) v = -fmul(v, sc);
        }
        st[0].offer(v, (unsigned)row, valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), 0, part_k, part_i);
}

// k_adc_search_lists_residual_u8 with a mask: the row term / scale of a disallowed row is not loaded (a NaN there
// reaches nothing); the probe bias is per segment, not per row, and is loaded as before
template <bool IP, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_search_lists_residual_masked_u8(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow,
    const float* __restrict__ lut, const float* __restrict__ bias, int64_t b_rs,
    const float* __restrict__ extra /* [n]: row terms, or scales / null */, int M, int K, int kk,
    const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_cum, int n_probe, unsigned* __restrict__ part_k,
    uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    constexpr int NW = NV + 1;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    const float* tab = lut + (size_t)blockIdx.y * MK;
    for (int i = threadIdx.x; i < MK; i += 1024) lds_s[i] = tab[i];
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + MK);        // [16][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[1];
    st[0].init();
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const float* pb = bias + (int64_t)blockIdx.y * b_rs;
    const int64_t total = sc[n_probe];
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t s0 = (int64_t)blockIdx.x * per < total ? (int64_t)blockIdx.x * per : total;
    const int64_t s1 = s0 + per < total ? s0 + per : total;
    // the segment that holds place s0: the first j with seg_cum[j + 1] > s0 (it exists while s0 < T, and is not empty)
    int j = 0;
    float b = 0.f;
    if (s0 < s1) {
        int lo_j = 0, hi_j = n_probe - 1;
        while (lo_j < hi_j) {
            const int mid = (lo_j + hi_j) >> 1;
            if (sc[mid + 1] > s0) hi_j = mid; else lo_j = mid + 1;
        }
        j = lo_j;
        b = pb[j];
    }
    int64_t seg_end = sc[j + 1];
    int64_t delta = sb[j] - sc[j];                                  // row = place + delta inside segment j
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = s0; base < s1; base += 1024) {              // wave-uniform trip count: the selection is wave-wide
        const int64_t c = base + threadIdx.x;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            if (c >= seg_end) {
                while (c >= seg_end && j + 1 < n_probe) {           // places < T end inside some segment
                    ++j;
                    seg_end = sc[j + 1];
                }
                delta = sb[j] - sc[j];
                b = pb[j];                                          // the segment that holds c: a probed, non-empty list
            }
            row = c + delta;
            valid = (uint64_t)row < (uint64_t)n;                    // holds by construction of the plan
        }
        if (valid) valid = mask_bit(allow, row);                    // before the fetch: a disallowed row is not read
        if (valid) {
            float x = 1.f;
            if constexpr (IP) x = extra ? extra[row] : 1.f;         // issued with the row's code words
            else x = extra[row];
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            const float s = adc_row_sum<NV>(w, sh, lds_s, M, K, bad);
            if constexpr (IP) v = -fmul(fadd(b, s), x);
            else v = fsub(fadd(b, x), fadd(s, s));
        }
        st[0].offer(v, (unsigned)row, valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), 0, part_k, part_i);
}

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
