// kernels_flat_among.hip.h -- exact search among given rows (include/pqhip.h: pqhip_flat_among_f32_dev,
// pqhip_flat_range_among_f32_dev): the exact top-k and the exact range result of every query over the rows that a list of
// candidate ids names, by the true squared distance or inner product to resident f32 / f16 vectors.  One producer in front
// of both consumers, joined from what is there already: the candidate rules of k_adc_among_u8 (the two lims words of a
// query clamped in the kernel, no plan kernel; -1 is padding, any other id outside [0, n) is skipped and raises the range
// flag, and no address is formed for it: kernels_adc_among.hip.h), the tile producer of k_flat_search_lists (the query
// image in LDS, tiles of kFlatTile = 16 consecutive PLACES, the 16 row numbers read back as wave-uniform values,
// rerank_elem / rerank_step, flat_reduce_tile), and then either the selection, combine and merge of every search
// (SearchState, search_finish, k_adc_search_merge) or the count / scan / fill with hit bitmaps of k_flat_range_lists
// (flat_range_tile, flat_range_mask16, range_emit, k_adc_range_scan: kernels_flat_range.hip.h).
// (Included from exactly one translation unit, pqhip_flat_among.hip.)
//
// Places, not rows.  The places of query q are ids[lims[q] .. lims[q + 1]) after clamping, or ids[0 .. n_ids) for every
// query when lims is null.  The four lanes of group u = lane >> 2 load the id of place t0 + u -- one 8-byte word, the 16
// groups of a wave 128 consecutive bytes -- and check it BEFORE any address is formed; the 16 row numbers then become
// wave-uniform (v_readlane of lane 4 u), so the row pointers live in scalar registers as in the list kernel.  A padding,
// out-of-range or past-the-slice place reads the query's own row instead (always readable, its sum never offered), and a
// tile with nothing to offer is skipped whole (wave-uniform: the ballot).
//
// Equivalence with the masked exhaustive call.  The value of a row depends on the row and the query alone: the lane
// chains are per row, and the transposed butterfly pairs (l, l + s) within one register at every step, whatever the
// other 15 registers of the tile hold (tests/flat_search_ref.py models it).  Which rows share a tile -- neighbours in the
// matrix there, neighbours in the id list here -- therefore changes no bit.  Top-k: the entries offered are
// (key(value), row) pairs under a strict order, so the first k of C_q are one list whatever the order of the ids, the
// tiles, the slices or G.  Range: units (waves with a contiguous sub-range of places), tiles and lanes all ascend, so the
// hits leave in the order in which they were named.
#pragma once
#include "kernels_flat_range.hip.h"

namespace pqhip {

// The clamped range of ids of the workgroup's query (blockIdx.y): lims is device memory and is not trusted -- both ends
// go to [0, n_ids], an inverted range is empty, and workgroup 0 of the query reports either (k_adc_among_u8's rules).
struct AmongRange {
    int64_t begin, len;
    bool bad;
};
__device__ __forceinline__ AmongRange flat_among_range(const int64_t* __restrict__ lims, int64_t n_ids)
{
    AmongRange r{0, n_ids, false};
    if (lims) {
        const int64_t b = lims[blockIdx.y], e = lims[blockIdx.y + 1];
        const int64_t cb = b < 0 ? 0 : b > n_ids ? n_ids : b;
        const int64_t ce = e < 0 ? 0 : e > n_ids ? n_ids : e;
        r.bad = (cb != b || ce != e || e < b) && blockIdx.x == 0;
        r.begin = cb;
        r.len = ce > cb ? ce - cb : 0;
    }
    return r;
}

// The row of place c (the caller holds c < the end of its slice): false for padding and for an id outside [0, n), which
// also sets bad.  No address is formed from `row` unless the result is true.
__device__ __forceinline__ bool flat_among_row(const int64_t* __restrict__ my_ids, int64_t c, int64_t n, int64_t& row, bool& bad)
{
    row = my_ids[c];                                                // begin + c < begin + len <= n_ids
    const bool valid = (uint64_t)row < (uint64_t)n;
    if (!valid && row != -1) bad = true;
    return valid;
}

// LDS: the query image [d] f32, then the queues [16][kSearchQueue] keys and indices; later the combine lists.
// lims [queries of the launch + 1] or null; part_* [queries][G][64 L].
template <typename T, bool IP, int L>
__global__ __launch_bounds__(1024) void k_flat_among(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                     int64_t n, int d, int64_t x_rs, int kk, const int64_t* __restrict__ lims,
                                                     const int64_t* __restrict__ ids, int64_t n_ids, unsigned* __restrict__ part_k,
                                                     uint64_t* __restrict__ part_i, int* __restrict__ err)
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
    const AmongRange r = flat_among_range(lims, n_ids);
    bool bad = r.bad;
    const ListsSlice slice = adc_lists_wg_slice(r.len);
    const int64_t s0 = slice.s0, s1 = slice.s1;
    const int64_t* my_ids = ids + r.begin;
    const int n_full = d >> 6, tail = d & 63;
    const T* skip = reinterpret_cast<const T*>(qrow);              // d elements of T are readable there
    const int u_mine = lane >> 2;
    for (int64_t t0 = s0 + wave * kFlatTile; t0 < s1; t0 += kSearchWaves * kFlatTile) {   // wave-uniform trip count
        const int64_t c = t0 + u_mine;
        int64_t row = 0;
        const bool ok = c < s1 && flat_among_row(my_ids, c, n, row, bad);   // before any load: a row not named is not read
        const unsigned long long have = __ballot(ok);              // bit 4 u: row u of the tile is offered
        if (have == 0) continue;                                   // no row to offer in the tile: nothing is loaded
        const unsigned row32 = (unsigned)row;                      // n <= 2^32 - 2
        const T* xr[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) {
            const unsigned ru = (unsigned)__builtin_amdgcn_readlane((int)row32, 4 * u);
            xr[u] = (have >> (4 * u)) & 1ull ? x + (int64_t)ru * x_rs : skip;
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
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_f), 0, part_k, part_i);
}

// Range search among given rows: grid (G, queries), one query per workgroup set, the producer above with the workgroup's
// slice of places cut into 16 contiguous wave sub-ranges (a multiple of 64 places each) as k_flat_range_lists cuts it, in
// front of its count / scan / fill.  part [queries][16 G].  hits [queries][bm_tiles]: tile i of unit u has slot
// u sub / 16 + i; the host sizes bm_tiles from n_ids (a shared list: every tile has a slot) resp. from a multiple of the
// mean range (lims given: it cannot see the ranges).  A tile whose slot lies beyond has no mask: the fill pass looks at
// all of its places again, under the same predicate.  out_i receives the id as named.
template <typename T, bool IP>
__global__ __launch_bounds__(1024) void k_flat_range_among(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                           int64_t n, int d, int64_t x_rs, const float* __restrict__ thr /* [queries] */,
                                                           const int64_t* __restrict__ lims, const int64_t* __restrict__ ids,
                                                           int64_t n_ids, int fill, int64_t* __restrict__ part,
                                                           uint16_t* __restrict__ hits, int64_t bm_tiles, int64_t capacity,
                                                           float* __restrict__ out_v, int64_t* __restrict__ out_i,
                                                           int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    const float* qrow = queries + (int64_t)blockIdx.y * q_rs;
    for (int j = threadIdx.x; j < d; j += 1024) lds_f[j] = qrow[j];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t slot_u = (int64_t)blockIdx.y * units + unit;
    uint16_t* hq = hits + (size_t)blockIdx.y * bm_tiles;
    const float t = thr[blockIdx.y];
    const AmongRange r = flat_among_range(lims, n_ids);
    bool bad = r.bad;
    const ListsSlice g = adc_lists_wg_slice(r.len);
    const int64_t sub = ((g.per + kRangeWaves - 1) / kRangeWaves + 63) / 64 * 64;
    const int64_t s0 = g.s0 + wave * sub < g.s1 ? g.s0 + wave * sub : g.s1;
    const int64_t s1 = s0 + sub < g.s1 ? s0 + sub : g.s1;
    const int64_t* my_ids = ids + r.begin;
    int64_t run = fill ? range_uniform(part[slot_u]) : 0;           // count: matches so far; fill: the next slot
    const T* skip = reinterpret_cast<const T*>(qrow);              // d elements of T are readable there
    const int u_mine = lane >> 2;
    int64_t tile = unit * (sub / kFlatTile);                        // the slot of the unit's first tile
    for (int64_t t0 = s0; t0 < s1; t0 += kFlatTile, ++tile) {       // wave-uniform: ascending tiles
        const bool has_mask = tile < bm_tiles;
        unsigned lm = 0xffffu;                                      // the places of the tile to look at
        if (fill && has_mask) {
            lm = (unsigned)__builtin_amdgcn_readfirstlane((int)hq[tile]);
            if (lm == 0) continue;                                  // no hit in the tile: no id or row is loaded
        }
        const int64_t c = t0 + u_mine;
        int64_t row = 0;
        const bool ok = c < s1 && ((lm >> u_mine) & 1u) && flat_among_row(my_ids, c, n, row, bad);
        const unsigned long long have = __ballot(ok);              // bit 4 u: row u of the tile is looked at
        if (have == 0) {
            if (!fill && has_mask && lane == 0) hq[tile] = 0;
            continue;
        }
        const unsigned row32 = (unsigned)row;                      // n <= 2^32 - 2
        const T* xr[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) {
            const unsigned ru = (unsigned)__builtin_amdgcn_readlane((int)row32, 4 * u);
            xr[u] = (have >> (4 * u)) & 1ull ? x + (int64_t)ru * x_rs : skip;
        }
        float p[1][kFlatTile];
        flat_range_tile<T, IP, 1>(xr, lds_f, d, lane, p);
        const float v = flat_reduce_tile(p[0]);
        const bool hit = ok && (lane & 3) == 0 && (IP ? v >= t : v <= t);
        if (!fill && has_mask) {
            const unsigned m = flat_range_mask16(__ballot(hit));
            if (lane == 0) hq[tile] = (uint16_t)m;
        }
        range_emit(hit, v, row, fill != 0, run, capacity, out_v, out_i);
    }
    if (!fill && lane == 0) part[slot_u] = run;
    if (bad) atomicOr(err, 1);
}

}  // namespace pqhip
