// kernels_adc_among.hip.h -- ADC search among given rows: the fused scan + exact top-k of kernels_adc_search.hip.h over,
// per query, the rows that a list of candidate ids names (include/pqhip.h: pqhip_adc_among_f32_dev,
// pqhip_adc_ip_among_f32_dev; instantiated by pqhip_adc_among.hip).
//
// C_q is the set of entries of ids[lims[q] .. lims[q + 1]) -- of ids[0 .. n_ids) for every query when lims is null --
// that lie in [0, n); the result of query q is the first k rows of C_q under the order of the other searches,
// (key(dist), row) resp. (key(-score), row).  The order is strict, so for distinct ids the result is the masked
// exhaustive search's with the mask of C_q -- whatever the order of the ids and whatever the grid.
//
// One kernel, k_adc_among_u8 (grid (G, queries), 1,024 threads): the body of k_adc_search_lists_u8 with the segment
// walk replaced.  It loads its query's [M][K] table into LDS, clamps the two lims words of its query itself (no plan
// kernel: both ends to [0, n_ids], an inverted range is empty; workgroup 0 of the query raises the range flag for
// either), takes its slice of the range (adc_lists_wg_slice) and walks it 1,024 places at a time: the trip count
// depends on the slice alone (wave-uniform, as SearchState::offer is wave-wide).  Lane t loads the id of its place --
// consecutive lanes read consecutive 8-byte words -- and checks it: -1 is padding, any other id outside [0, n) is
// skipped and raises the flag.  Only then does it form a row address, so no byte of a row that is not named is read:
// its codes, scale, row term and list id reach nothing.  Row fetch, row sum, selection, queue and the merge of the 16
// waves are those of k_adc_search_lists_u8; the tie-break value offered with a row is the row (32 bits:
// n <= 2^32 - 2).  The G partial lists of a query are merged by k_adc_search_merge.
//
// RESIDUAL: the bias is not per probe slot but per list, bias[q][row_list[row]] -- the lane loads the row's list id with
// its code words and its row term / scale, checks it (outside [0, n_lists): the row is skipped, the flag raised) and
// gathers the bias, a row of n_lists floats per query that stays in L2.
#pragma once
#include "kernels_adc_search.hip.h"

namespace pqhip {

// The value offered for a row is k_adc_search_lists_u8's, operation for operation: s the row sum over the query's table
// (sequential f32 over m from +0), x = extra[row], b = bias[q][row_list[row]]:
//   plain:     IP = false: s                                         IP = true: -fl(s * x)           (x = 1 when extra == null)
//   RESIDUAL:  IP = false: fl(fl(b + x) - fl(s + s))   (x: row terms, never null)
//              IP = true:  -fl(fl(b + s) * x)          (x: scales, 1 when extra == null)          s over inner-product tables
// lut [queries of the launch][M][K]; lims [queries of the launch + 1] or null; bias [queries of the launch][b_rs],
// b_rs >= n_lists; part_* [queries][G][64 L].  A flag that is off leaves no instruction and no argument load behind.
template <bool IP, bool RESIDUAL, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_among_u8(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const float* __restrict__ lut,
    const float* __restrict__ extra /* [n]: scales (IP) or row terms (RESIDUAL, !IP), or null */, int M, int K, int kk,
    const int64_t* __restrict__ lims, const int64_t* __restrict__ ids, int64_t n_ids, unsigned* __restrict__ part_k,
    uint64_t* __restrict__ part_i, int* __restrict__ err, const int64_t* __restrict__ row_list /* RESIDUAL: [n] */,
    int64_t n_lists, const float* __restrict__ bias /* RESIDUAL */, int64_t b_rs)
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
    bool bad = false;
    // the query's range of ids: lims is device memory and is not trusted
    int64_t begin = 0, len = n_ids;
    if (lims) {
        const int64_t b = lims[blockIdx.y], e = lims[blockIdx.y + 1];
        const int64_t cb = b < 0 ? 0 : b > n_ids ? n_ids : b;
        const int64_t ce = e < 0 ? 0 : e > n_ids ? n_ids : e;
        if ((cb != b || ce != e || e < b) && blockIdx.x == 0) bad = true;
        begin = cb;
        len = ce > cb ? ce - cb : 0;
    }
    const float* pb = nullptr;
    if constexpr (RESIDUAL) pb = bias + (int64_t)blockIdx.y * b_rs;
    const ListsSlice slice = adc_lists_wg_slice(len);
    const int64_t s0 = slice.s0, s1 = slice.s1;
    const int64_t* my_ids = ids + begin;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    for (int64_t base = s0; base < s1; base += 1024) {              // wave-uniform trip count: the selection is wave-wide
        const int64_t c = base + threadIdx.x;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            row = my_ids[c];                                        // begin + c < begin + len <= n_ids
            valid = (uint64_t)row < (uint64_t)n;
            if (!valid && row != -1) bad = true;
        }
        if (valid) {
            float x = 1.f;
            int64_t l = 0;
            if constexpr (RESIDUAL) l = row_list[row];              // issued with the row's code words, as x is
            if constexpr (IP) x = extra ? extra[row] : 1.f;
            else if constexpr (RESIDUAL) x = extra[row];
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            float b = 0.f;
            if constexpr (RESIDUAL) {
                if ((uint64_t)l < (uint64_t)n_lists) b = pb[l];
                else { bad = true; valid = false; }
            }
            const float s = adc_row_sum<NV>(w, (unsigned)(a & 3), lds_s, M, K, bad);
            if constexpr (RESIDUAL) v = IP ? -fmul(fadd(b, s), x) : fsub(fadd(b, x), fadd(s, s));
            else v = IP ? -fmul(s, x) : s;
        }
        st[0].offer(v, (unsigned)row, valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), 0, part_k, part_i);
}

}  // namespace pqhip
