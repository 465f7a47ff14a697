// kernels_flat_search_lists.hip.h -- exact search in probed lists (pqhip_flat_search_lists_f32_dev, IVF-Flat): the exact
// top-k of every query by the true squared distance or inner product to the rows of the lists that the query probes, over
// an f32 / f16 matrix stored in list order.  One producer that joins what is there already: the plan of the list searches
// (k_adc_lists_plan: the only reader of the offsets and probes), their slices and segment walk (adc_lists_wg_slice,
// adc_segment_start / adc_segment_seek of kernels_adc.hip.h), the row value and the tile reduction of the exhaustive flat
// search (rerank_step, flat_reduce_tile of kernels_flat_search.hip.h) and the selection, combine and merge of every search
// (SearchState, search_finish, k_adc_search_merge).
// (Included from exactly one translation unit, pqhip_flat_search_lists.hip.)
//
// k_flat_search_lists: grid (G, queries), 1,024 threads, one query per workgroup -- queries probe different lists, so a
// loaded row serves one query.  The query image [d] is staged in LDS.  The workgroup takes its slice [s0, s1) of the T_q
// concatenated probed rows; a wave takes tiles of kFlatTile = 16 consecutive PLACES of the concatenation, the 16 waves
// interleaved, so a tile may straddle any number of list boundaries and short or empty lists cost no idle tile.
//
// Rows of a tile, found once per tile: the four lanes of group u = lane >> 2 all seek place t0 + u (monotone per lane:
// the place of a lane grows by 256 per trip; one compare while it stays inside a list), test the row's mask bit before
// any load, and the 16 row numbers are read back as wave-uniform values (v_readlane of lane 4 u), so the row pointers
// live in scalar registers as in k_flat_search.  Nothing is looked up per element.  A place past the slice or a
// disallowed row reads the query's own row instead (always readable, its sum never offered); a tile without any row to
// offer is skipped whole (wave-uniform: the ballot).  The lanes with (lane & 3) == 0 hold, after flat_reduce_tile, the
// value of the row they sought themselves and offer it with its 32-bit position as the tie-break.
//
// Equivalence with the exhaustive call.  The value of a row depends on the row and the query alone: the lane chains are
// per row, and the transposed butterfly pairs (l, l + s) within one register at every step, whatever the other 15
// registers of the tile hold (tests/flat_search_ref.py models it).  Which rows share a tile therefore changes no bit,
// and the entries offered are (key(value), position) pairs under a strict order: the first k of S_q are one set
// whatever tiles, slices, G or probe order produced them.
#pragma once
#include "kernels_flat_search.hip.h"

namespace pqhip {

// LDS: the query image [d] f32, then the queues [16][kSearchQueue] keys and indices; later the combine lists.
// seg_begin [queries of the launch][n_probe], seg_cum [queries of the launch][n_probe + 1]: k_adc_lists_plan's, with
// n = n_rows, so every row it yields lies in [0, n).  allow == null: no mask.  part_* [queries][G][64 L].
template <typename T, bool IP, int L>
__global__ __launch_bounds__(1024) void k_flat_search_lists(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                            int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow, int kk,
                                                            const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_cum,
                                                            int n_probe, unsigned* __restrict__ part_k, uint64_t* __restrict__ part_i)
{
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    const float* qrow = queries + (int64_t)blockIdx.y * q_rs;
    for (int j = threadIdx.x; j < d; j += 1024) lds_f[j] = qrow[j];
    unsigned* qk = reinterpret_cast<unsigned*>(lds_f + d);         // [16][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    SearchState<L> st[1];
    st[0].init();
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const ListsSlice slice = adc_lists_wg_slice(sc[n_probe]);
    const int64_t s0 = slice.s0, s1 = slice.s1;
    SegmentPos pos = adc_segment_start(sb, sc, nullptr, n_probe, s0, s1);
    const int n_full = d >> 6, tail = d & 63;
    const T* skip = reinterpret_cast<const T*>(qrow);              // d elements of T are readable there
    const int u_mine = lane >> 2;
    for (int64_t t0 = s0 + wave * kFlatTile; t0 < s1; t0 += kSearchWaves * kFlatTile) {   // wave-uniform trip count
        const int64_t c = t0 + u_mine;
        bool ok = c < s1;
        int64_t row = 0;
        if (ok) {
            pos = adc_segment_seek<true>(pos, c, sb, sc, nullptr, n_probe);
            row = c + pos.delta;
            ok = (uint64_t)row < (uint64_t)n;                      // holds by construction of the plan
        }
        if (allow && ok) ok = adc_mask_bit(allow, row);            // before any load: a disallowed row is not read
        const unsigned long long have = __ballot(ok);              // bit 4 u: row u of the tile is offered
        if (have == 0) continue;                                   // no row to offer in the tile: nothing is loaded
        const unsigned row32 = (unsigned)row;                      // n <= 2^32 - 2
        const T* xr[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) {
            const unsigned r = (unsigned)__builtin_amdgcn_readlane((int)row32, 4 * u);
            xr[u] = (have >> (4 * u)) & 1ull ? x + (int64_t)r * x_rs : skip;
        }
        float p[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) p[u] = 0.f;
        for (int i = 0; i < n_full; ++i) {
            float xv[kFlatTile];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + i * 64 + lane);
            const float qv = lds_f[i * 64 + lane];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) p[u] = rerank_step<IP>(p[u], qv, xv[u]);
        }
        if (lane < tail) {
            float xv[kFlatTile];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + n_full * 64 + lane);
            const float qv = lds_f[n_full * 64 + lane];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) p[u] = rerank_step<IP>(p[u], qv, xv[u]);
        }
        const float v = flat_reduce_tile(p);
        st[0].offer(IP ? -v : v, row32, ok && (lane & 3) == 0, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_f), 0, part_k, part_i);
}

}  // namespace pqhip
