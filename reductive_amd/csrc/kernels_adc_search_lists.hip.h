// kernels_adc_search_lists.hip.h -- ADC search over a partitioned code matrix (IVFADC, with or without residual
// encoding): the fused scan + exact top-k of kernels_adc_search.hip.h restricted, per query, to the rows of the lists
// that the query probes.  (pqhip_adc.hip instantiates the plan kernel and the producers without a row mask,
// pqhip_adc_masked.hip those with one.)
//
// List l is rows [list_off[l], list_off[l + 1]) of the code matrix; probe row q names the lists of query q.  S_q is the
// set of rows of those lists, and the result of query q is the first k rows of S_q under the order of the exhaustive
// searches, (key(dist), position) resp. (key(-score), position), the position being the row's index in the code matrix.
// The order is strict, so the result is the exhaustive search's on the matrix with every row outside S_q removed,
// positions mapped back -- whatever the grid.
//
// Two kernels.  k_adc_lists_plan (one workgroup per query) turns a probe row into segments: per probe the first row
// and, as a running sum, the number of probed rows before it.  It is the only reader of list_off and the probes, and it
// checks them: -1 is padding, any other id outside [0, n_lists) is skipped and raises the range flag, a range is
// clamped to [0, n_codes] and an inverted one is empty (both raise the flag).  The producer therefore never forms a
// row outside the matrix.  k_adc_search_lists_u8 (grid (G, queries), 1,024 threads) loads its query's [M][K] table
// into LDS, takes its slice of the T concatenated probed rows (adc_lists_wg_slice) and walks it 1,024 rows at a time:
// the trip count depends on the slice alone (wave-uniform, as SearchState::offer is wave-wide), every lane maps its
// place in the concatenation to a row by stepping through the segments (adc_segment_start / adc_segment_seek: monotone,
// one compare per row while it stays inside a list), so short lists cost no idle lanes.  Row sum, selection, queue and
// the merge of the 16 waves are those of k_adc_search_u8 with NQ = 1; the tie-break value offered with a row is its
// position (32 bits: n_codes <= 2^32 - 2, 0xffffffff stays "empty").  The G partial lists of a query are merged by
// k_adc_search_merge.
//
// Residual codes (RESIDUAL; the codes encode x - c_list(x)).  One table per query, no table per list.  With r^_i the
// reconstruction of row i's residual code, l its list and c_l the coarse centroid,
//   |q - c_l - r^_i|^2 = |q - c_l|^2 + (|r^_i|^2 + 2 <c_l, r^_i>) - 2 <q, r^_i>         <q, c_l + r^_i> = <q, c_l> + <q, r^_i>
// so both searches are the inner-product list scan plus one f32 per (query, probe slot), the probe bias, and for the
// distance one f32 per row, the row term, stored beside the codes as the scales are.  A lane holds the bias of the
// segment it stands in (SegmentPos::bias) and reloads it where it reloads delta, on a segment change; segments it only
// steps over (skipped probes and empty lists) are never read, so the bias of a skipped probe cannot reach a result.
#pragma once
#include "kernels_adc_search.hip.h"

namespace pqhip {

#ifndef PQHIP_ADC_TEMPLATES_ONLY   // not a template: it belongs to one translation unit, pqhip_adc.hip
// seg_begin [nq][n_probe]: first row of the probe's list (clamped); seg_cum [nq][n_probe + 1]: probed rows before the
// probe, seg_cum[q][n_probe] = T_q.  A skipped probe is an empty segment.
__global__ __launch_bounds__(1024) void k_adc_lists_plan(const int64_t* __restrict__ list_off, int64_t n_lists,
                                                         const int64_t* __restrict__ probes, int n_probe, int64_t p_rs,
                                                         int64_t n, int64_t* __restrict__ seg_begin,
                                                         int64_t* __restrict__ seg_cum, int* __restrict__ err)
{
    __shared__ long long wsum[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t* pr = probes + (int64_t)blockIdx.x * p_rs;
    int64_t* sb = seg_begin + (size_t)blockIdx.x * n_probe;
    int64_t* sc = seg_cum + (size_t)blockIdx.x * ((size_t)n_probe + 1);
    long long carry = 0;
    bool bad = false;
    for (int64_t p0 = 0; p0 < n_probe; p0 += 1024) {
        const int64_t p = p0 + threadIdx.x;
        long long begin = 0, len = 0;
        if (p < n_probe) {
            const int64_t l = pr[p];
            if (l >= 0 && l < n_lists) {
                const int64_t lo = list_off[l], hi = list_off[l + 1];
                const int64_t cl = lo < 0 ? 0 : lo > n ? n : lo;
                const int64_t ch = hi < 0 ? 0 : hi > n ? n : hi;
                if (cl != lo || ch != hi || hi < lo) bad = true;
                if (ch > cl) { begin = cl; len = ch - cl; }
            } else if (l != -1) {
                bad = true;
            }
        }
        long long v = len;                                      // inclusive scan over the wave, then over the 16 waves
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(v, d);
            if (lane >= d) v += o;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (p < n_probe) { sb[p] = begin; sc[p] = carry + before + v - len; }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) sc[n_probe] = carry;
    if (bad) atomicOr(err, 1);
}
#endif  // PQHIP_ADC_TEMPLATES_ONLY

// The value offered for a row: s the row sum over the query's table (sequential f32 over m from +0), x = extra[row],
// b the bias of the probe slot through which the row is reached, every operation one rounded f32 operation:
//   plain:     IP = false: s                                         IP = true: -fl(s * x)           (x = 1 when extra == null)
//   RESIDUAL:  IP = false: fl(fl(b + x) - fl(s + s))   (x: row terms, never null)
//              IP = true:  -fl(fl(b + s) * x)          (x: scales, 1 when extra == null)          s over inner-product tables
// MASKED: the row's bit of `allow` (the mask in position order) is tested before the fetch, as in k_adc_search_u8 -- the
// row term / scale of a disallowed row is not loaded (a NaN there reaches nothing); the bias is per segment and is
// loaded as without a mask.  A flag that is off leaves no instruction and no argument load behind.
// lut [queries of the launch][M][K]; bias [queries of the launch][b_rs], b_rs >= n_probe; part_* [queries][G][64 L].
template <bool IP, bool RESIDUAL, bool MASKED, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_search_lists_u8(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const float* __restrict__ lut,
    const float* __restrict__ extra /* [n]: scales (IP) or row terms (RESIDUAL, !IP), or null */, int M, int K, int kk,
    const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_cum, int n_probe, unsigned* __restrict__ part_k,
    uint64_t* __restrict__ part_i, int* __restrict__ err, const float* __restrict__ bias /* RESIDUAL */, int64_t b_rs,
    const uint32_t* __restrict__ allow /* MASKED */)
{
    constexpr int NW = NV + 1;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    adc_stage_tables<1>(lds_s, lut + (size_t)blockIdx.y * MK, MK);
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + MK);        // [16][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[1];
    st[0].init();
    // (sb before sc, the slice after both: the scalar register allocation of these kernels follows the order)
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const float* pb = nullptr;
    if constexpr (RESIDUAL) pb = bias + (int64_t)blockIdx.y * b_rs;
    const ListsSlice slice = adc_lists_wg_slice(sc[n_probe]);
    const int64_t s0 = slice.s0, s1 = slice.s1;
    SegmentPos pos = adc_segment_start<RESIDUAL>(sb, sc, pb, n_probe, s0, s1);
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = s0; base < s1; base += 1024) {              // wave-uniform trip count: the selection is wave-wide
        const int64_t c = base + threadIdx.x;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            pos = adc_segment_seek<!RESIDUAL, RESIDUAL>(pos, c, sb, sc, pb, n_probe);
            row = c + pos.delta;
            valid = (uint64_t)row < (uint64_t)n;                    // holds by construction of the plan
        }
        if constexpr (MASKED) {
            if (valid) valid = adc_mask_bit(allow, row);            // before the fetch: a disallowed row is not read
        }
        if (valid) {
            float x = 1.f;
            if constexpr (IP) x = extra ? extra[row] : 1.f;         // issued with the row's code words
            else if constexpr (RESIDUAL) x = extra[row];
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const float s = adc_row_sum<NV>(w, (unsigned)(a & 3), lds_s, M, K, bad);
            if constexpr (RESIDUAL) v = IP ? -fmul(fadd(pos.bias, s), x) : fsub(fadd(pos.bias, x), fadd(s, s));
            else v = IP ? -fmul(s, x) : s;
        }
        st[0].offer(v, (unsigned)row, valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), 0, part_k, part_i);
}

}  // namespace pqhip
