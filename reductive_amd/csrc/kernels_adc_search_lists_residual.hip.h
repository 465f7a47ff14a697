// kernels_adc_search_lists_residual.hip.h -- the residual producer: ADC search over a partitioned code matrix whose
// codes encode x - c_list(x) (IVFADC with residual encoding).  (Launched from exactly one translation unit, pqhip_adc.hip.)
//
// One table per query, no table per list.  With r^_i the reconstruction of row i's residual code, l its list and c_l
// the coarse centroid,
//   |q - c_l - r^_i|^2 = |q - c_l|^2 + (|r^_i|^2 + 2 <c_l, r^_i>) - 2 <q, r^_i>         <q, c_l + r^_i> = <q, c_l> + <q, r^_i>
// so both searches are the inner-product list scan of kernels_adc_search_lists.hip.h plus one f32 per (query, probe
// slot), the probe bias, and for the distance one f32 per row, the row term, stored beside the codes as the scales are.
// With s the scan's row sum over the query's inner-product table (sequential f32 over m from +0), p the probe slot
// through which the row is reached, every operation one rounded f32 operation:
//   IP = false:  dist  = fl(fl(bias[q][p] + term[i]) - fl(s + s)),   offered as is        (extra = row terms, never null)
//   IP = true:   score = fl(fl(bias[q][p] + s) * scale[i]),          offered as -score    (extra = scales, null: scale 1)
// Plan, slices, segment walk, selection, queue, LDS budget and the 16-wave merge are k_adc_search_lists_u8's, and the
// partial lists go to the same merge kernels.  A lane holds the bias of the segment it stands in and reloads it where
// it reloads seg_end and delta, on a segment change; segments it only steps over (skipped probes and empty lists) are
// never read, so the bias of a skipped probe cannot reach a result.  The body is restated here rather than shared
// through a template flag so that the existing list producers keep their code objects instruction for instruction.
#pragma once
#include "kernels_adc_search_lists.hip.h"

namespace pqhip {

// lut [queries of the launch][M][K] inner-product tables; bias [queries of the launch][b_rs], b_rs >= n_probe;
// part_* [queries][G][64 L].
template <bool IP, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_search_lists_residual_u8(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const float* __restrict__ lut,
    const float* __restrict__ bias, int64_t b_rs, const float* __restrict__ extra /* [n]: row terms, or scales / null */,
    int M, int K, int kk, const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_cum, int n_probe,
    unsigned* __restrict__ part_k, uint64_t* __restrict__ part_i, int* __restrict__ err)
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

}  // namespace pqhip
