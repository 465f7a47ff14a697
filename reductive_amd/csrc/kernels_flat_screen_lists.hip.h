// kernels_flat_screen_lists.hip.h -- the matrix-core range screen of kernels_flat_screen.hip.h over PROBED LISTS
// (include/pqhip.h: pqhip_flat_screen_lists_f32_dev).  Per query it returns a superset of what
// pqhip_flat_range_lists_f32_dev returns at the same thresholds, as positions in that call's order: probe slot first,
// then ascending position.  The work is list-major: a list that 64 queries probe is streamed once for all of them.
// (Instantiated by pqhip_flat_screen_lists.hip.)
//
// Screening value.  Exactly that of k_flat_screen: the f16 image row and the (s_q, tau_q) pair of a query come from
// k_flat_screen_prep, a(q, r) is one chain of v_mfma_f32_32x32x16_f16 through one accumulator in ascending trips of 32
// elements (fsl_tile_chain below is that loop), xx is accumulated from the elements as loaded, and the epilogue is
// w = fma(-s_q, a, c xx) against tau_q.  An output element of the matrix instruction depends on its own row of A and
// its own column of B only, so a(q, r) does not depend on which other queries share the group or which other rows share
// the tile: the bound of §5c holds as it stands.
//
// Inversion.  A chunk of queries has the probe table [nq][n_probe]; entry e = q n_probe + slot is a PAIR when its list
// id is valid and the (clamped) list is not empty.
//     k_fsl_pairs    one thread per entry: validates id and offsets (range flag), tiles[e] = tiles of 32 rows of the
//                    list, counts the pairs of every list (integer atomics), clears cnt[e].
//     k_fsl_units    one workgroup: exclusive prefixes over the lists of their pairs and of their UNITS.
//     k_fsl_scatter  one thread per entry: the pair takes a place among its list's pairs from an integer cursor.
// The place of a pair inside its list decides which group of <= 64 (32 while d > 1,024) pairs it is screened with and
// nothing else: its hit words, its count and its output are functions of (query, list) alone, see above.
//
// Units.  A list with p pairs and r rows has ceil(p / QG) groups x ceil(r / unit_rows) row chunks; unit_off is their
// prefix over the lists.  A fixed grid strides over unit numbers and finds the list of a unit by binary search in
// unit_off: no unit table exists, the host reads no count, lists nobody probes and empty lists have no unit.
//
// Count pass k_flat_screen_lists: per unit the workgroup gathers the group's image rows and pairs into LDS BY QUERY
// NUMBER (the padded pitch of k_flat_screen; padding slots zeros with tau = NaN, their hits masked out) and its 8 waves
// take the unit's tiles.  A tile is 32 consecutive rows counted from the LIST'S first row, so its mask word is
// assembled from two words of d_allow; a disallowed row and a row past the list's end are never loaded.  One 32-bit
// hit word per (pair, tile) goes to hits[hoff[e] + tile] -- hoff is the exclusive prefix of tiles[] in (query, slot)
// order -- and the unit's counts are added to cnt[e] with integer atomics.  The hit words of a chunk have a budget the
// host derives from n_rows, n_probe and n_lists; a pair whose words would not fit (lists far longer than the mean,
// lists named again and again) is counted all the same and its words are computed again by the fill pass.
//
// Fill pass k_flat_screen_lists_fill: cnt, scanned in (query, slot) order by k_adc_range_scan, is the first output slot
// of every pair.  One wave per entry walks the pair's hit words in ascending tile order, 64 words per step, with a wave
// prefix of their popcounts, and stores positions below `capacity`.  It reads the matrix only for a pair without stored
// words: then it forms each tile's word itself, the same chain with the pair's query alone in the A operand.
#pragma once
#include "kernels_flat_screen.hip.h"

namespace pqhip {

constexpr int kFslPlanThreads = 256;
constexpr int64_t kFslMaxEntries = 1 << 20;     // (query, slot) entries of a chunk: what one scan launch sums

// Hit words of one query of a chunk (host): twice what a query probes when the lists are equally long -- n_rows
// min(n_probe, n_lists) / n_lists rows in tiles of 32, one partial tile per slot -- and never more than n_probe whole
// matrices.  The budget of a chunk is the sum over its queries: what a query leaves, another may take.
inline int64_t fsl_words_per_query(int64_t n_rows, int64_t n_lists, int64_t n_probe)
{
    const double frac = (double)(n_probe < n_lists ? n_probe : n_lists) / (double)n_lists;
    const int64_t expected = (int64_t)((double)n_rows * frac / kFsTile) + 1 + n_probe;
    const int64_t most = n_probe * (n_rows / kFsTile + 1);
    return 2 * expected < most ? 2 * expected : most;
}

// list l as the list calls read it: clamped to [0, n], an inverted range empty; bad: the flag is due
struct FslRange {
    int64_t lo, hi;
    bool bad;
};
__device__ __forceinline__ FslRange fsl_list_range(const int64_t* __restrict__ list_off, int64_t l, int64_t n)
{
    const int64_t lo = list_off[l], hi = list_off[l + 1];
    const int64_t cl = lo < 0 ? 0 : lo > n ? n : lo;
    const int64_t ch = hi < 0 ? 0 : hi > n ? n : hi;
    return {cl, ch > cl ? ch : cl, cl != lo || ch != hi || hi < lo};
}

inline __global__ __launch_bounds__(kFslPlanThreads) void k_fsl_pairs(const int64_t* __restrict__ list_off, int64_t n_lists,
                                                               const int64_t* __restrict__ probes, int n_probe, int64_t p_rs,
                                                               int64_t n, int64_t nq, unsigned* __restrict__ lcnt,
                                                               int64_t* __restrict__ tiles, int64_t* __restrict__ cnt,
                                                               int64_t* __restrict__ scan0, int* __restrict__ err)
{
    const int64_t e = (int64_t)blockIdx.x * kFslPlanThreads + threadIdx.x;
    if (e == 0) scan0[0] = 0;                                       // the tile scan starts from zero
    if (e >= nq * n_probe) return;
    const int64_t q = e / n_probe;
    const int64_t l = probes[q * p_rs + (e - q * n_probe)];
    int64_t t = 0;
    bool bad = false;
    if (l >= 0 && l < n_lists) {
        const FslRange r = fsl_list_range(list_off, l, n);
        bad = r.bad;
        if (r.hi > r.lo) {
            t = (r.hi - r.lo + kFsTile - 1) / kFsTile;
            atomicAdd(&lcnt[l], 1u);
        }
    } else if (l != -1) {
        bad = true;
    }
    tiles[e] = t;
    cnt[e] = 0;
    if (bad) atomicOr(err, 1);
}

// pair_off [n_lists + 1], unit_off [n_lists + 1]: exclusive prefixes of the lists' pairs and units, 1,024 lists per trip
// with a carry (the scan of k_adc_range_scan, two sums at once).  A list has pairs only if it has rows.
inline __global__ __launch_bounds__(1024) void k_fsl_units(const int64_t* __restrict__ list_off, int64_t n_lists, int64_t n,
                                                    const unsigned* __restrict__ lcnt, int qg, int64_t unit_rows,
                                                    unsigned* __restrict__ pair_off, int64_t* __restrict__ unit_off)
{
    __shared__ long long wsum_p[16], wsum_u[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long carry_p = 0, carry_u = 0;
    for (int64_t l0 = 0; l0 < n_lists; l0 += 1024) {
        const int64_t l = l0 + threadIdx.x;
        long long p = 0, u = 0;
        if (l < n_lists) {
            p = (long long)lcnt[l];
            if (p > 0) {
                const FslRange r = fsl_list_range(list_off, l, n);
                u = ((p + qg - 1) / qg) * ((r.hi - r.lo + unit_rows - 1) / unit_rows);
            }
        }
        long long vp = p, vu = u;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const long long op = __shfl_up(vp, s), ou = __shfl_up(vu, s);
            if (lane >= s) { vp += op; vu += ou; }
        }
        if (lane == 63) { wsum_p[wave] = vp; wsum_u[wave] = vu; }
        __syncthreads();
        long long before_p = 0, before_u = 0, total_p = 0, total_u = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) { before_p += wsum_p[w]; before_u += wsum_u[w]; }
            total_p += wsum_p[w];
            total_u += wsum_u[w];
        }
        if (l < n_lists) {
            pair_off[l] = (unsigned)(carry_p + before_p + vp - p);
            unit_off[l] = carry_u + before_u + vu - u;
        }
        carry_p += total_p;
        carry_u += total_u;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pair_off[n_lists] = (unsigned)carry_p;
        unit_off[n_lists] = carry_u;
    }
}

// tiles[e] > 0 marks the pairs (k_fsl_pairs; the tile scan runs after this kernel)
inline __global__ __launch_bounds__(kFslPlanThreads) void k_fsl_scatter(const int64_t* __restrict__ probes, int n_probe, int64_t p_rs,
                                                                 int64_t nq, const int64_t* __restrict__ tiles,
                                                                 const unsigned* __restrict__ pair_off,
                                                                 unsigned* __restrict__ cursor, unsigned* __restrict__ pairs)
{
    const int64_t e = (int64_t)blockIdx.x * kFslPlanThreads + threadIdx.x;
    if (e >= nq * n_probe || tiles[e] <= 0) return;
    const int64_t q = e / n_probe;
    const int64_t l = probes[q * p_rs + (e - q * n_probe)];
    pairs[pair_off[l] + atomicAdd(&cursor[l], 1u)] = (unsigned)e;
}

// The mask word of the tile of 32 rows from position row0 (any alignment) of a list that ends at `end` <= n: the rows
// that exist and are allowed.  No word of d_allow beyond ceil(n / 32) is read.
__device__ __forceinline__ unsigned fsl_tile_bits(const uint32_t* __restrict__ allow, int64_t row0, int64_t end, int64_t n)
{
    const int64_t left = end - row0;
    unsigned bits = left >= kFsTile ? 0xffffffffu : (1u << (int)left) - 1u;
    if (allow) {
        const int64_t wi = row0 >> 5;
        const int sh = (int)(row0 & 31);
        unsigned m = allow[wi] >> sh;
        if (sh != 0 && (wi + 1) * 32 < n) m |= allow[wi + 1] << (32 - sh);
        bits &= m;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)bits);
}

// The k loop of k_flat_screen for one tile: rp = the lane's row + 16 h (dereferenced only when ok), arow = the image row
// of the lane's query of block 0 + 16 h, blocks 32 ldq apart; nba <= NB blocks are computed (wave-uniform).  SINGLE:
// the image is one query's row and only the lanes with a_live supply it, the others zeros (query 0 of the block).
// Returns xx of the lane's row.
template <typename T, int NB, bool SINGLE>
__device__ __forceinline__ float fsl_tile_chain(const T* rp, bool ok, int d, int dp, int al, float cx,
                                                const unsigned short* arow, int ldq, int nba, bool a_live, f32x16 (&acc)[NB])
{
    const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    float xx = 0.f;
    for (int k0 = 0; k0 < dp; k0 += kFsKStep) {
        float v[16];
        flat_screen_load16(rp + k0, ok ? d - k0 - 16 * h : 0, al, v);
        unsigned w[8];
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
            xx = __builtin_fmaf(v[e], v[e], xx);
            xx = __builtin_fmaf(v[e + 1], v[e + 1], xx);
            w[e >> 1] = flat_screen_pk(v[e] * cx, v[e + 1] * cx);
        }
        const fs_u32x4 b0 = (fs_u32x4){w[0], w[1], w[2], w[3]}, b1 = (fs_u32x4){w[4], w[5], w[6], w[7]};
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b < nba) {
                fs_u32x4 a0 = (fs_u32x4){0u, 0u, 0u, 0u}, a1 = (fs_u32x4){0u, 0u, 0u, 0u};
                if (!SINGLE || a_live) {
                    a0 = *reinterpret_cast<const fs_u32x4*>(arow + b * 32 * ldq + k0);
                    a1 = *reinterpret_cast<const fs_u32x4*>(arow + b * 32 * ldq + k0 + 8);
                }
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(fs_f16x8, a0), __builtin_bit_cast(fs_f16x8, b0),
                                                                acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(fs_f16x8, a1), __builtin_bit_cast(fs_f16x8, b1),
                                                                acc[b], 0, 0, 0);
            }
        }
    }
    return xx + __shfl_xor(xx, 32);                                 // the row's two halves: the same sum in both lanes
}

// dynamic LDS of the count pass: image rows, (s, tau) pairs, hit bases and entries of a group of qg pairs
constexpr size_t flat_screen_lists_lds(int qg, int d) { return flat_screen_image_bytes(qg, d) + (size_t)qg * 12; }

// The count pass (see the head of the file).  img / prm_g: the chunk's image [queries][ldq] and pairs [queries];
// cx, cxx, al as in k_flat_screen.  hoff [entries]: first hit word of a pair; hits [budget]; cnt [entries].
template <typename T, int NB>
__global__ __launch_bounds__(64 * kFsWaves) void k_flat_screen_lists(
    const T* __restrict__ x, int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow, const int64_t* __restrict__ list_off,
    int64_t n_lists, const unsigned* __restrict__ lcnt, const unsigned* __restrict__ pair_off, const int64_t* __restrict__ unit_off,
    const unsigned* __restrict__ pairs, int n_probe, const unsigned short* __restrict__ img, const float2* __restrict__ prm_g, int ldq,
    float cx, float cxx, int al, int64_t unit_rows, const int64_t* __restrict__ hoff, int64_t budget, uint32_t* __restrict__ hits,
    unsigned long long* __restrict__ cnt)
{
    constexpr int QG = 32 * NB;
    extern __shared__ __attribute__((aligned(16))) unsigned short lds_img[];
    __shared__ int64_t s_list;
    float2* prm = reinterpret_cast<float2*>(lds_img + QG * ldq);
    int64_t* s_hb = reinterpret_cast<int64_t*>(prm + QG);
    int* s_e = reinterpret_cast<int*>(s_hb + QG);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n32 = lane & 31, h = lane >> 5;
    const int dp = flat_screen_dp(d);
    const int row_chunks = ldq / 8;                                 // 16-byte pieces of an image row
    const float inf = __builtin_inff();
    const int64_t total = unit_off[n_lists];
    for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
        __syncthreads();                                            // the previous unit's LDS is free
        if (threadIdx.x == 0) {                                     // the largest l with unit_off[l] <= u
            int64_t lo = 0, hi = n_lists;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (unit_off[mid] <= u) lo = mid; else hi = mid;
            }
            s_list = lo;
        }
        __syncthreads();
        const int64_t l = range_uniform(s_list);
        const FslRange r = fsl_list_range(list_off, l, n);
        const int64_t chunks = (r.hi - r.lo + unit_rows - 1) / unit_rows;
        const int64_t local = u - unit_off[l];
        const int64_t g = local / chunks, ci = local - g * chunks;
        const int np = __builtin_amdgcn_readfirstlane((int)((int64_t)lcnt[l] - g * QG < QG ? (int64_t)lcnt[l] - g * QG : QG));
        const int64_t list_tiles = (r.hi - r.lo + kFsTile - 1) / kFsTile;
        const unsigned* pl = pairs + pair_off[l] + g * QG;
        for (int c = threadIdx.x; c < QG * row_chunks; c += 64 * kFsWaves) {
            const int j = c / row_chunks, k = c - j * row_chunks;
            fs_u32x4 v = (fs_u32x4){0u, 0u, 0u, 0u};
            if (j < np) v = reinterpret_cast<const fs_u32x4*>(img + (size_t)(pl[j] / (unsigned)n_probe) * ldq)[k];
            reinterpret_cast<fs_u32x4*>(lds_img)[c] = v;
        }
        if (threadIdx.x < QG) {
            const int j = threadIdx.x;
            if (j < np) {
                const unsigned e = pl[j];
                prm[j] = prm_g[e / (unsigned)n_probe];
                s_hb[j] = hoff[e];
                s_e[j] = (int)e;
            } else {
                prm[j] = make_float2(0.f, __builtin_nanf(""));
                s_hb[j] = budget;
                s_e[j] = -1;
            }
        }
        __syncthreads();
        const int nba = NB > 1 && np > 32 ? 2 : 1;
        const int64_t rb = r.lo + ci * unit_rows;
        const int64_t re = rb + unit_rows < r.hi ? rb + unit_rows : r.hi;
        unsigned long long cn[NB];                                  // lane l < 32: the unit's hits of pair 32 b + l
#pragma unroll
        for (int b = 0; b < NB; ++b) cn[b] = 0ull;
        for (int64_t row0 = rb + wave * kFsTile; row0 < re; row0 += kFsWaves * kFsTile) {   // wave-uniform
            const unsigned bits = fsl_tile_bits(allow, row0, re, n);
            unsigned mine[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) mine[b] = 0u;
            if (bits != 0u) {                                       // a tile without an allowed row loads nothing
                const bool ok = (bits >> n32) & 1u;
                f32x16 acc[NB];
                const float xx = fsl_tile_chain<T, NB, false>(x + (row0 + n32) * x_rs + 16 * h, ok, d, dp, al, cx,
                                                              lds_img + n32 * ldq + 16 * h, ldq, nba, true, acc);
                const float xk = cxx * xx;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < nba) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int q0 = 8 * (i >> 2) + (i & 3);  // the pair of half 0 in register i; half 1: q0 + 4
                            const float2 p = prm[b * 32 + q0 + 4 * h];
                            const float wv = __builtin_fmaf(-p.x, acc[b][i], xk);
                            const bool outside = wv > p.y && wv < inf;      // NaN and +-Inf: not proved, returned
                            const unsigned long long bl = __ballot(ok && !outside);
                            if (lane == q0) mine[b] = (unsigned)bl;
                            if (lane == q0 + 4) mine[b] = (unsigned)(bl >> 32);
                        }
                    }
                }
            }
            if (lane < 32) {
                const int64_t tile = (row0 - r.lo) >> 5;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int j = b * 32 + lane;
                    if (j < np) {                                   // a padding slot has no hits
                        const int64_t hb = s_hb[j];
                        if (hb + list_tiles <= budget) hits[hb + tile] = mine[b];
                        cn[b] += (unsigned long long)__popc(mine[b]);
                    }
                }
            }
        }
        if (lane < 32) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int j = b * 32 + lane;
                if (j < np && cn[b] != 0ull) atomicAdd(&cnt[s_e[j]], cn[b]);
            }
        }
    }
}

// The fill pass: one wave per entry e, entries taken grid-stride.  first [entries]: the scanned counts.
template <typename T>
__global__ __launch_bounds__(64 * kFsWaves) void k_flat_screen_lists_fill(
    const T* __restrict__ x, int64_t n, int d, int64_t x_rs, const uint32_t* __restrict__ allow, const int64_t* __restrict__ list_off,
    int64_t n_lists, const int64_t* __restrict__ probes, int n_probe, int64_t p_rs, int64_t nq, const unsigned short* __restrict__ img,
    const float2* __restrict__ prm_g, int ldq, float cx, float cxx, int al, const int64_t* __restrict__ hoff, int64_t budget,
    const uint32_t* __restrict__ hits, const int64_t* __restrict__ first, int64_t capacity, int64_t* __restrict__ out_i)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n32 = lane & 31, h = lane >> 5;
    const int dp = flat_screen_dp(d);
    const float inf = __builtin_inff();
    for (int64_t e = (int64_t)blockIdx.x * kFsWaves + wave; e < nq * n_probe; e += (int64_t)gridDim.x * kFsWaves) {   // wave-uniform
        const int64_t q = e / n_probe;
        const int64_t l = probes[q * p_rs + (e - q * n_probe)];
        if (l < 0 || l >= n_lists) continue;
        const FslRange r = fsl_list_range(list_off, l, n);
        if (r.hi <= r.lo) continue;
        const int64_t list_tiles = (r.hi - r.lo + kFsTile - 1) / kFsTile;
        const int64_t hb = hoff[e];
        int64_t run = first[e];
        if (hb + list_tiles <= budget) {
            for (int64_t t0 = 0; t0 < list_tiles; t0 += 64) {
                const int64_t t = t0 + lane;
                unsigned w = t < list_tiles ? hits[hb + t] : 0u;
                const int pc = __popc(w);
                int incl = pc;
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const int o = __shfl_up(incl, s);
                    if (lane >= s) incl += o;
                }
                int64_t slot = run + (int64_t)(incl - pc);
                const int64_t base = r.lo + t * kFsTile;
                while (w) {
                    const int b = __builtin_ctz(w);
                    w &= w - 1;
                    if (slot < capacity) out_i[slot] = base + b;
                    ++slot;
                }
                run += (int64_t)__shfl(incl, 63);
            }
        } else {                                                    // no stored words: form them again, this query alone
            const float2 p = prm_g[q];
            for (int64_t t = 0; t < list_tiles; ++t) {
                const int64_t row0 = r.lo + t * kFsTile;
                const unsigned bits = fsl_tile_bits(allow, row0, r.hi, n);
                if (bits == 0u) continue;
                const bool ok = (bits >> n32) & 1u;
                f32x16 acc[1];
                const float xx = fsl_tile_chain<T, 1, true>(x + (row0 + n32) * x_rs + 16 * h, ok, d, dp, al, cx,
                                                            img + (size_t)q * ldq + 16 * h, ldq, 1, n32 == 0, acc);
                const float wv = __builtin_fmaf(-p.x, acc[0][0], cxx * xx);   // register 0 of half 0: query 0 of the block
                const bool outside = wv > p.y && wv < inf;
                const unsigned w = (unsigned)__ballot(h == 0 && ok && !outside);
                if (lane < 32 && ((w >> lane) & 1u)) {
                    const int64_t slot = run + (int64_t)__popc(w & ((1u << lane) - 1u));
                    if (slot < capacity) out_i[slot] = row0 + lane;
                }
                run += (int64_t)__popc(w);
            }
        }
    }
}

}  // namespace pqhip
