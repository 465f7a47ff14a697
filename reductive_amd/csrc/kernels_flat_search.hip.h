// kernels_flat_search.hip.h -- exact search over resident vectors (pqhip_flat_search_f32_dev): the exhaustive top-k of
// every query by the true squared distance or inner product to ALL rows of an f32 / f16 matrix.  The producer of this
// file streams whole vectors where the ADC producers stream codes; selection, combine and merge are theirs, unchanged
// (SearchState, search_finish, k_adc_search_merge of kernels_adc_search.hip.h).
// (Included from exactly one translation unit, pqhip_flat_search.hip.)
//
// Value of a row (include/pqhip.h; the value of pqhip_rerank_f32_dev, operation for operation): lane l of a wave owns the
// chain from +0 over j = l, l + 64, .. and the 64 partials are reduced by the tree p_l <- fl(p_l + p_(l+s)), s = 32 .. 1.
//
// k_flat_search: one 1,024-thread workgroup per contiguous range of rows_per_wg rows (a multiple of 1,024), the NQ
// queries of the pass staged once in LDS as [NQ][d].  A wave takes tiles of kFlatTile = 16 consecutive rows, the 16 waves
// interleaved.  Per 64-element step it issues the 16 coalesced row loads (lane l: element l + 64 i) before the first is
// used; each loaded element serves all NQ queries.  A row that is past the end or whose mask bit is clear is read from
// the first query's own row instead (always readable, its sum never offered), so the loads stay free of branches and no
// byte of a disallowed row is touched; a tile without any allowed row is skipped whole (wave-uniform).
//
// Reduction: a transposed butterfly over the tile (flat_fold).  At step s two registers A and B, each holding rows'
// partials, are folded into one: lanes with bit s clear keep A and receive A of lane l + s, the others keep B and
// receive B of lane l - s, then one add.  The pairs are the tree's (l, l + s) and f32 addition commutes, so every sum
// is the tree's sum, bit for bit (a NaN's payload aside; values are canonical on return).  Folding register u with
// u + 8, then u + 4, u + 2, u + 1 at s = 32, 16, 8, 4 leaves row u of the tile in the lanes with (lane >> 2) == u;
// the steps s = 2, 1 are plain xor exchanges of that one register (every lane of a group of four ends with the
// tree's value of lane 0).  15 + 2 exchange-adds per 16 (row, query) pairs instead of 6 per pair.  The 32- and
// 16-lane exchanges are v_permlane32_swap / v_permlane16_swap: they move exactly the halves that change owner.
// Lanes with (lane & 3) == 0 then offer one row each.
#pragma once
#include "kernels_adc_search.hip.h"
#include "kernels_rerank.hip.h"   // rerank_elem, rerank_step: the element conversion and the chain step of the value

namespace pqhip {

constexpr int kFlatTile = 16;                // rows a wave reduces at once
constexpr int kFlatMaxD = kRerankMaxD;       // one query image of 64 KB in LDS

// One transposed step: the result holds a's tree sums in the lanes with bit S clear and b's in the others.
template <int S>
__device__ __forceinline__ float flat_fold(float a, float b)
{
    if constexpr (S == 32) {
        // lanes 32-63 of a <-> lanes 0-31 of b
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
        return fadd(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else if constexpr (S == 16) {
        // odd rows of 16 lanes of a <-> even rows of b
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
        return fadd(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else {
        const bool hi = (threadIdx.x & S) != 0;
        const float keep = hi ? b : a, send = hi ? a : b;
        return fadd(keep, __shfl_xor(send, S));
    }
}

// p[0 .. 16): the lane partials of the tile's rows -> the value of row (lane >> 2) & 15, in all four lanes of its group
__device__ __forceinline__ float flat_reduce_tile(const float (&p)[kFlatTile])
{
    float r8[8], r4[4], r2[2];
#pragma unroll
    for (int u = 0; u < 8; ++u) r8[u] = flat_fold<32>(p[u], p[u + 8]);
#pragma unroll
    for (int u = 0; u < 4; ++u) r4[u] = flat_fold<16>(r8[u], r8[u + 4]);
#pragma unroll
    for (int u = 0; u < 2; ++u) r2[u] = flat_fold<8>(r4[u], r4[u + 2]);
    float v = flat_fold<4>(r2[0], r2[1]);
    v = fadd(v, __shfl_xor(v, 2));
    v = fadd(v, __shfl_xor(v, 1));
    return v;
}

// LDS: the query image [NQ][d] f32, then the queues [16][NQ][kSearchQueue] keys and indices; later the combine lists.
// allow == null: no mask.  Row ranges start on multiples of 1,024 and tiles on multiples of 16 within them, so a tile's
// mask bits lie in one word.
template <typename T, bool IP, int NQ, int L>
__global__ __launch_bounds__(1024) void k_flat_search(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                      int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow, int kk,
                                                      int64_t rows_per_wg, unsigned* __restrict__ part_k,
                                                      uint64_t* __restrict__ part_i)
{
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        for (int j = threadIdx.x; j < d; j += 1024) lds_f[q * d + j] = queries[(int64_t)q * q_rs + j];
    unsigned* qk = reinterpret_cast<unsigned*>(lds_f + NQ * d);   // [16][NQ][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * NQ * kSearchQueue;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    SearchState<L> st[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    const int n_full = d >> 6, tail = d & 63;
    const T* skip = reinterpret_cast<const T*>(queries);           // d elements of T are readable there
    for (int64_t row0 = row_begin + wave * kFlatTile; row0 < row_end; row0 += kSearchWaves * kFlatTile) {
        const int64_t left = row_end - row0;
        unsigned bits = left >= kFlatTile ? 0xffffu : (1u << (int)left) - 1u;
        if (allow) bits &= allow[row0 >> 5] >> ((unsigned)row0 & 31u);
        bits = (unsigned)__builtin_amdgcn_readfirstlane((int)bits);
        if (bits == 0) continue;                                   // no allowed row in the tile: nothing is loaded
        const T* xr[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) xr[u] = (bits >> u) & 1u ? x + (row0 + u) * x_rs : skip;
        float p[NQ][kFlatTile];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) p[q][u] = 0.f;
        for (int i = 0; i < n_full; ++i) {
            float xv[kFlatTile];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + i * 64 + lane);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float qv = lds_f[q * d + i * 64 + lane];
#pragma unroll
                for (int u = 0; u < kFlatTile; ++u) p[q][u] = rerank_step<IP>(p[q][u], qv, xv[u]);
            }
        }
        if (lane < tail) {
            float xv[kFlatTile];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + n_full * 64 + lane);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float qv = lds_f[q * d + n_full * 64 + lane];
#pragma unroll
                for (int u = 0; u < kFlatTile; ++u) p[q][u] = rerank_step<IP>(p[q][u], qv, xv[u]);
            }
        }
        const int u_mine = lane >> 2;
        const bool valid = (lane & 3) == 0 && ((bits >> u_mine) & 1u);
        const unsigned off = (unsigned)(row0 - row_begin) + (unsigned)u_mine;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float v = flat_reduce_tile(p[q]);
            st[q].offer(IP ? -v : v, off, valid, qk + (wave * NQ + q) * kSearchQueue, qi + (wave * NQ + q) * kSearchQueue, kk);
        }
    }
    search_finish<NQ, L>(st, qk, qi, reinterpret_cast<unsigned*>(lds_f), row_begin, part_k, part_i);
}

}  // namespace pqhip
