// kernels_flat_range.hip.h -- exact range search over resident vectors (include/pqhip.h: pqhip_flat_range_f32_dev,
// pqhip_flat_range_lists_f32_dev): EVERY row whose true squared distance is <= thr[q] resp. whose inner product is
// >= thr[q], exhaustive and over probed lists, as CSR.  A new pairing of what is there already: the producer of the exact
// searches (the query image in LDS, tiles of kFlatTile = 16 rows, the 16 row loads of a 64-element step issued before the
// first use, rerank_elem / rerank_step, flat_reduce_tile: kernels_flat_search.hip.h; the plan, slices and segment walk
// of the list searches: kernels_adc.hip.h) with the consumer of the ADC range searches (range_emit, range_uniform,
// k_adc_range_scan and the count / scan / fill sequence of kernels_adc_range.hip.h).
// (Instantiated by pqhip_flat_range.hip; kernels_flat_among.hip.h takes flat_range_tile and flat_range_mask16 from here.)
//
// Units and order.  The producer unit is a WAVE with a contiguous sub-range of its workgroup's rows (a multiple of 64, so
// mask words and tiles never straddle units) -- not the interleaved tiles of the top-k kernels.  Units ascend with rows
// (exhaustive) resp. with places of the concatenation of the probed lists, tiles ascend inside a unit, and after
// flat_reduce_tile the lanes with (lane & 3) == 0 hold the rows lane >> 2 of the tile in ascending order: the ballot of
// `hit` over them plus range_emit's rank is ascending row order as it stands.  No workgroup barrier sits in the row loop.
//
// The fill pass does not stream the matrix again.  A row is hundreds of bytes where a code row is 15, so the count pass
// leaves, per (query, tile), the tile's 16-bit hit mask in a scratch bitmap: one lane stores it with a plain vector store
// (a tile belongs to exactly one wave; no atomics), n / 8 bytes per query of the pass resp. T_q / 8 per query of a list
// chunk.  The fill pass loads only the rows of a tile that hit for some query of the pass -- a tile without a hit is
// skipped whole, a row without one is redirected to the query's own row like a masked row -- recomputes their values
// (the same arithmetic on the same bytes: the same bits), applies the same predicate and stores.  A selective radius costs
// one stream of the matrix plus its hits; a radius that admits every row costs two.
#pragma once
#include "kernels_adc_range.hip.h"
#include "kernels_flat_search_lists.hip.h"

namespace pqhip {

// bit u of the result = bit 4 u of b: the ballot of the offering lanes as the tile's mask
__device__ __forceinline__ unsigned flat_range_mask16(unsigned long long b)
{
    b &= 0x1111111111111111ull;
    b = (b | (b >> 3)) & 0x0303030303030303ull;
    b = (b | (b >> 6)) & 0x000f000f000f000full;
    b = (b | (b >> 12)) & 0x000000ff000000ffull;
    return (unsigned)((b | (b >> 24)) & 0xffffull);
}

// The partials of one tile: xr[u] the 16 row pointers (wave-uniform), q the query image [NQ][d] in LDS.
template <typename T, bool IP, int NQ>
__device__ __forceinline__ void flat_range_tile(const T* const (&xr)[kFlatTile], const float* q, int d, int lane,
                                                float (&p)[NQ][kFlatTile])
{
    const int n_full = d >> 6, tail = d & 63;
#pragma unroll
    for (int iq = 0; iq < NQ; ++iq)
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) p[iq][u] = 0.f;
    for (int i = 0; i < n_full; ++i) {
        float xv[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + i * 64 + lane);
#pragma unroll
        for (int iq = 0; iq < NQ; ++iq) {
            const float qv = q[iq * d + i * 64 + lane];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) p[iq][u] = rerank_step<IP>(p[iq][u], qv, xv[u]);
        }
    }
    if (lane < tail) {
        float xv[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) xv[u] = rerank_elem(xr[u] + n_full * 64 + lane);
#pragma unroll
        for (int iq = 0; iq < NQ; ++iq) {
            const float qv = q[iq * d + n_full * 64 + lane];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) p[iq][u] = rerank_step<IP>(p[iq][u], qv, xv[u]);
        }
    }
}

// Exhaustive range search, NQ queries per pass.  Workgroup b owns rows [b rows_per_wg, (b + 1) rows_per_wg) (rows_per_wg a
// multiple of 1,024), its wave w the sub-range [w rows_per_wg / 16, (w + 1) rows_per_wg / 16) of it: unit u = 16 b + w.
// part [NQ][units]: counts out (fill == 0), first slots in (fill == 1).  hits [NQ][ceil(n / 16)]: the tile masks, out
// (fill == 0: every tile of the unit's range, zero for a tile that is skipped) resp. in (fill == 1).  A wave looks at 64
// tiles at once -- lane l holds the masks of tile l of the group -- and visits those it has to: all of them in the count
// pass, those with a hit in the fill pass.  allow == null: no mask; the fill pass does not read it (a hit row is allowed).
template <typename T, bool IP, int NQ>
__global__ __launch_bounds__(1024) void k_flat_range(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                     int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow,
                                                     const float* __restrict__ thr /* [NQ] */, int64_t rows_per_wg, int fill,
                                                     int64_t* __restrict__ part, uint16_t* __restrict__ hits, int64_t capacity,
                                                     float* __restrict__ out_v, int64_t* __restrict__ out_i)
{
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        for (int j = threadIdx.x; j < d; j += 1024) lds_f[q * d + j] = queries[(int64_t)q * q_rs + j];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t sub = rows_per_wg / kRangeWaves;                  // a multiple of 64
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    const int64_t tiles = (n + kFlatTile - 1) / kFlatTile;
    float t[NQ];
    int64_t run[NQ];                                                // count: matches so far; fill: the next slot
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        t[q] = thr[q];
        run[q] = fill ? range_uniform(part[q * units + unit]) : 0;
    }
    const T* skip = reinterpret_cast<const T*>(queries);           // d elements of T are readable there
    const int u_mine = lane >> 2;
    for (int64_t g0 = row_begin; g0 < row_end; g0 += 64 * kFlatTile) {      // wave-uniform: groups of 64 tiles
        const int64_t my_row0 = g0 + (int64_t)lane * kFlatTile;
        unsigned hm[NQ];
        unsigned any = my_row0 < row_end ? 1u : 0u;
#pragma unroll
        for (int q = 0; q < NQ; ++q) hm[q] = 0xffffu;
        if (fill) {
            any = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                hm[q] = my_row0 < row_end ? (unsigned)hits[q * tiles + (my_row0 >> 4)] : 0u;
                any |= hm[q];
            }
        }
        unsigned long long todo = __ballot(any != 0);
        while (todo) {                                              // ascending tiles
            const int ti = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t row0 = g0 + (int64_t)ti * kFlatTile;
            const int64_t left = row_end - row0;
            unsigned bits = left >= kFlatTile ? 0xffffu : (1u << (int)left) - 1u;
            unsigned lm[NQ];                                        // the rows of the tile a query may return
            if (fill) {
                unsigned some = 0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    lm[q] = (unsigned)__builtin_amdgcn_readlane((int)hm[q], ti) & bits;
                    some |= lm[q];
                }
                bits = some;
            } else {
                if (allow) bits &= allow[row0 >> 5] >> ((unsigned)row0 & 31u);
                bits = (unsigned)__builtin_amdgcn_readfirstlane((int)bits);
#pragma unroll
                for (int q = 0; q < NQ; ++q) lm[q] = bits;
            }
            if (bits == 0) {                                        // no row to look at in the tile: nothing is loaded
                if (!fill && lane == 0) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) hits[q * tiles + (row0 >> 4)] = 0;
                }
                continue;
            }
            const T* xr[kFlatTile];
#pragma unroll
            for (int u = 0; u < kFlatTile; ++u) xr[u] = (bits >> u) & 1u ? x + (row0 + u) * x_rs : skip;
            float p[NQ][kFlatTile];
            flat_range_tile<T, IP, NQ>(xr, lds_f, d, lane, p);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float v = flat_reduce_tile(p[q]);
                const bool hit = (lane & 3) == 0 && ((lm[q] >> u_mine) & 1u) && (IP ? v >= t[q] : v <= t[q]);
                if (!fill) {
                    const unsigned m = flat_range_mask16(__ballot(hit));
                    if (lane == 0) hits[q * tiles + (row0 >> 4)] = (uint16_t)m;
                }
                range_emit(hit, v, row0 + u_mine, fill != 0, run[q], capacity, out_v, out_i);
            }
        }
    }
    if (!fill && lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) part[q * units + unit] = run[q];
    }
}

// Range search over probed lists: grid (G, queries), one query per workgroup, the walk of k_flat_search_lists -- the
// segment plan of k_adc_lists_plan, the workgroup's slice of the T_q concatenated probed rows (adc_lists_wg_slice), tiles
// of 16 consecutive PLACES, the rows of a tile sought once (the four lanes of group u seek place t0 + u, the row numbers
// read back as wave-uniform values) -- with the slice cut into 16 contiguous wave sub-ranges (a multiple of 64 places
// each) as k_adc_range_lists_u8 cuts it.  part [queries][16 G].  hits [queries][bm_tiles]: tile i of unit u has slot
// u sub / 16 + i; the host sizes bm_tiles for T_q <= n_rows (every row probed once).  A tile whose slot lies beyond --
// lists named more than once -- has no mask: the fill pass looks at all of its rows again, under the same predicate.
template <typename T, bool IP>
__global__ __launch_bounds__(1024) void k_flat_range_lists(const float* __restrict__ queries, int64_t q_rs, const T* __restrict__ x,
                                                           int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow,
                                                           const float* __restrict__ thr /* [queries] */,
                                                           const int64_t* __restrict__ seg_begin,
                                                           const int64_t* __restrict__ seg_cum, int n_probe, int fill,
                                                           int64_t* __restrict__ part, uint16_t* __restrict__ hits,
                                                           int64_t bm_tiles, int64_t capacity, float* __restrict__ out_v,
                                                           int64_t* __restrict__ out_i)
{
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    const float* qrow = queries + (int64_t)blockIdx.y * q_rs;
    for (int j = threadIdx.x; j < d; j += 1024) lds_f[j] = qrow[j];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t slot_u = (int64_t)blockIdx.y * units + unit;
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    uint16_t* hq = hits + (size_t)blockIdx.y * bm_tiles;
    const float t = thr[blockIdx.y];
    const ListsSlice g = adc_lists_wg_slice(sc[n_probe]);
    const int64_t sub = ((g.per + kRangeWaves - 1) / kRangeWaves + 63) / 64 * 64;
    const int64_t s0 = g.s0 + wave * sub < g.s1 ? g.s0 + wave * sub : g.s1;
    const int64_t s1 = s0 + sub < g.s1 ? s0 + sub : g.s1;
    SegmentPos pos = adc_segment_start(sb, sc, nullptr, n_probe, s0, s1);
    int64_t run = fill ? range_uniform(part[slot_u]) : 0;           // count: matches so far; fill: the next slot
    const T* skip = reinterpret_cast<const T*>(qrow);              // d elements of T are readable there
    const int u_mine = lane >> 2;
    int64_t tile = unit * (sub / kFlatTile);                        // the slot of the unit's first tile
    for (int64_t t0 = s0; t0 < s1; t0 += kFlatTile, ++tile) {       // wave-uniform: ascending tiles
        const bool has_mask = tile < bm_tiles;
        unsigned lm = 0xffffu;                                      // the places of the tile to look at
        if (fill && has_mask) {
            lm = (unsigned)__builtin_amdgcn_readfirstlane((int)hq[tile]);
            if (lm == 0) continue;                                  // no hit in the tile: nothing is sought or loaded
        }
        const int64_t c = t0 + u_mine;
        bool ok = c < s1 && ((lm >> u_mine) & 1u);
        int64_t row = 0;
        if (ok) {
            pos = adc_segment_seek<true>(pos, c, sb, sc, nullptr, n_probe);
            row = c + pos.delta;
            ok = (uint64_t)row < (uint64_t)n;                      // holds by construction of the plan
        }
        if (allow && ok) ok = adc_mask_bit(allow, row);            // before any load: a disallowed row is not read
        const unsigned long long have = __ballot(ok);              // bit 4 u: row u of the tile is looked at
        if (have == 0) {
            if (!fill && has_mask && lane == 0) hq[tile] = 0;
            continue;
        }
        const unsigned row32 = (unsigned)row;                      // n <= 2^32 - 2
        const T* xr[kFlatTile];
#pragma unroll
        for (int u = 0; u < kFlatTile; ++u) {
            const unsigned r = (unsigned)__builtin_amdgcn_readlane((int)row32, 4 * u);
            xr[u] = (have >> (4 * u)) & 1ull ? x + (int64_t)r * x_rs : skip;
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
}

}  // namespace pqhip
