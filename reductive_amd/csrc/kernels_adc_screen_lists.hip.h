// kernels_adc_screen_lists.hip.h -- the u8 table screen of kernels_adc_screen.hip.h over PROBED LISTS (include/pqhip.h:
// pqhip_adc_screen_lists_f32_dev).  Per query it returns a superset of what pqhip_adc_range_lists_f32_dev
// resp. pqhip_adc_ip_range_lists_f32_dev returns at the same thresholds, as positions in that call's order: probe slot
// first, then ascending position.  The work is list-major: a list that 32 queries probe is streamed once for all of them.
// (Instantiated by pqhip_adc_screen_lists.hip.)
//
// Screening value.  Exactly that of k_adc_screen_u8.  The image u[m][k] and the parameters (ulim, b, s, thr) of a query
// come from adc_screen_prep_slot, the body of k_adc_screen_prep: they depend on the query's tables and threshold and on
// the call-wide largest scale, on nothing else.  U of a (row, query) is an exact integer sum over the row's codes and the
// query's image.  So neither depends on which queries share a group, which rows share a unit or where a unit starts, and
// the bound of §5e holds as it stands.
//
// Inversion and units are those of kernels_flat_screen_lists.hip.h, kernel for kernel (k_fsl_pairs, k_fsl_units,
// k_fsl_scatter, k_adc_range_scan over tiles and counts): a PAIR is a (query, slot) entry with a valid, non-empty list, a
// list with p pairs and r rows has ceil(p / NQ) groups x ceil(r / unit_rows) row chunks, and a fixed grid strides over
// unit numbers and finds a unit's list by binary search in unit_off.  Hit words stay per tile of 32 rows (kFsTile): a wave
// step of 64 rows is two tiles, the halves of its ballot their words.
//
// Preparation k_adc_screen_lists_prep: one workgroup per query of the chunk; the images go to the scratch QUERY-MAJOR,
// [q][pitch] bytes with entry m K + k at byte m K + k -- a group is assembled per unit, so the interleaved layout of a
// pass cannot be precomputed.
//
// Count pass k_adc_screen_lists: per unit the workgroup stages the group's images into LDS in the interleaved
// [M][K][NQ] layout that adc_screen_entry reads (adc_screen_lists_stage: a byte transpose, see there), with the
// parameters, hit bases and entries of the pairs behind it; padding slots are zeros with ulim = -1.  A workgroup whose
// next unit has the same (list, group) keeps the image.  The 16 waves take the unit's rows, 64 per step, one row per
// lane, counted from the LIST'S first row: the allow bits of a step are assembled from d_allow at any bit offset
// (fsl_tile_bits); a disallowed row and a row past the list's end are never loaded.  The sums are adc_screen_row_sums,
// the predicate adc_screen_keep.  One 32-bit hit word per (pair, tile) goes to hits[hoff[e] + tile], the unit's counts to
// cnt[e] by integer atomics.  A pair whose words would not fit the budget is counted all the same.
//
// Fill pass k_adc_screen_lists_fill: one wave per (query, slot) entry walks the pair's hit words 64 at a time with a
// wave prefix of popcounts and stores positions below `capacity`; it does not read the codes.  For a pair without stored
// words it forms them again, for this query alone, from the query's image in the scratch: the same integers, so the
// same bits.
#pragma once
#include "kernels_adc_screen.hip.h"
#include "kernels_flat_screen_lists.hip.h"

namespace pqhip {

// bytes of a query's image in the scratch: entry m K + k at byte m K + k, rows 16 bytes apart at least
constexpr int64_t adc_screen_lists_pitch(int M, int K) { return ((int64_t)M * K + 15) / 16 * 16; }

// dynamic LDS of the count pass: the image and parameters of a pass, then per slot the first hit word (8), the entry (4)
// and the query (4), then the unit's list (8, padded)
constexpr size_t adc_screen_lists_lds_bytes(int M, int K, int nq) { return adc_screen_lds_bytes(M, K, nq) + (size_t)nq * 16 + 16; }

inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_lists_prep(const float* __restrict__ tables, int M, int K,
                                                                          const float* __restrict__ thr, int ip, int scaled,
                                                                          const unsigned* __restrict__ cmax_bits,
                                                                          uint8_t* __restrict__ imgq, int64_t pitch,
                                                                          AdcScreenPrm* __restrict__ prm)
{
    const int64_t q = blockIdx.x;
    adc_screen_prep_slot(tables + (size_t)q * M * K, true, M, K, thr + q, ip, scaled, cmax_bits, kAdcScreenSteps + 1,
                         imgq + q * pitch, (size_t)1, prm + q);
}

// rows a, b, c, d of 4 bytes each -> their columns: o[i] = (a_i, b_i, c_i, d_i), 8 v_perm_b32
__device__ __forceinline__ void adc_screen_transpose4(unsigned a, unsigned b, unsigned c, unsigned d, unsigned (&o)[4])
{
    const unsigned t0 = __builtin_amdgcn_perm(b, a, 0x05010400u), t1 = __builtin_amdgcn_perm(b, a, 0x07030602u);   // a0 b0 a1 b1 / a2 b2 a3 b3
    const unsigned u0 = __builtin_amdgcn_perm(d, c, 0x05010400u), u1 = __builtin_amdgcn_perm(d, c, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

// The images of a group, query-major in the scratch, into the interleaved LDS image [M K][NQ]: a byte transpose.  An
// item is (four consecutive entries, QT = min(NQ, 16) consecutive slots): QT dword loads -- one per query, 4 entries
// each --, QT / 4 transposes of 4 x 4 bytes, and four stores of QT bytes, each the QT slots of one entry (16 bytes for
// NQ >= 16).  Consecutive threads take the slot groups of one cell, then the next cell.  s_qn [NQ]: the query of every
// slot, -1 for padding (zeros).  The entries past the last whole cell (M K not a multiple of 4) go byte by byte.
template <int NQ>
__device__ __forceinline__ void adc_screen_lists_stage(uint8_t* lds_u, const uint8_t* __restrict__ imgq, int64_t pitch, int MK, const int* s_qn)
{
    constexpr int QT = NQ >= 16 ? 16 : NQ, QI = NQ / QT, G4 = QT / 4;
    const int cells = MK / 4;
    for (int it = threadIdx.x; it < cells * QI; it += 1024) {
        const int cell = it / QI, j0 = (it - cell * QI) * QT;
        unsigned o[4][G4];
#pragma unroll
        for (int g = 0; g < G4; ++g) {
            unsigned a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qn = s_qn[j0 + 4 * g + i];
                a[i] = qn >= 0 ? *reinterpret_cast<const unsigned*>(imgq + (int64_t)qn * pitch + 4 * cell) : 0u;
            }
            unsigned t[4];
            adc_screen_transpose4(a[0], a[1], a[2], a[3], t);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i][g] = t[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint8_t* dst = lds_u + (size_t)(4 * cell + i) * NQ + j0;
            if constexpr (G4 == 4) *reinterpret_cast<as_u32x4*>(dst) = (as_u32x4){o[i][0], o[i][1], o[i][2], o[i][3]};
            else if constexpr (G4 == 2) *reinterpret_cast<as_u32x2*>(dst) = (as_u32x2){o[i][0], o[i][1]};
            else *reinterpret_cast<unsigned*>(dst) = o[i][0];
        }
    }
    for (int it = threadIdx.x; it < (MK - 4 * cells) * NQ; it += 1024) {
        const int e = 4 * cells + it / NQ, j = it % NQ;
        const int qn = s_qn[j];
        lds_u[(size_t)e * NQ + j] = qn >= 0 ? imgq[(int64_t)qn * pitch + e] : (uint8_t)0;
    }
}

// the allowed, existing rows of the wave step of 64 rows from position row0 < end: the mask words of its two tiles
__device__ __forceinline__ unsigned long long adc_screen_lists_step_bits(const uint32_t* __restrict__ allow, int64_t row0, int64_t end, int64_t n)
{
    const unsigned b0 = fsl_tile_bits(allow, row0, end, n);
    const unsigned b1 = row0 + kFsTile < end ? fsl_tile_bits(allow, row0 + kFsTile, end, n) : 0u;
    return ((unsigned long long)b1 << 32) | b0;
}

// The count pass (see the head of the file).  imgq / prm_g: the chunk's images [queries][pitch] and parameters
// [queries].  hoff [entries]: first hit word of a pair; hits [budget]; cnt [entries].
template <int NV, int NQ>
__global__ __launch_bounds__(1024) void k_adc_screen_lists(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow /* or null */,
    const float* __restrict__ scales /* [n] or null */, const int64_t* __restrict__ list_off, int64_t n_lists,
    const unsigned* __restrict__ lcnt, const unsigned* __restrict__ pair_off, const int64_t* __restrict__ unit_off,
    const unsigned* __restrict__ pairs, int n_probe, const uint8_t* __restrict__ imgq, int64_t pitch,
    const AdcScreenPrm* __restrict__ prm_g, int M, int K, int64_t unit_rows, const int64_t* __restrict__ hoff, int64_t budget,
    uint32_t* __restrict__ hits, unsigned long long* __restrict__ cnt, int* __restrict__ err)
{
    static_assert(NQ == 4 || NQ == 8 || NQ == 16 || NQ == 32, "query slots per group");
    constexpr int NW = NV + 1, ND = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_u[];
    const int MK = M * K, KQ = K * NQ;
    AdcScreenPrm* prm = reinterpret_cast<AdcScreenPrm*>(lds_u + adc_screen_image_bytes(M, K, NQ));
    int64_t* s_hb = reinterpret_cast<int64_t*>(prm + NQ);
    int* s_e = reinterpret_cast<int*>(s_hb + NQ);
    int* s_qn = s_e + NQ;
    int64_t* s_list = reinterpret_cast<int64_t*>(s_qn + NQ);
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
                    prm[j] = prm_g[qn];
                    s_hb[j] = hoff[e];
                    s_e[j] = (int)e;
                    s_qn[j] = qn;
                } else {
                    prm[j] = AdcScreenPrm{-1, 0.f, 0.f, 0.f};
                    s_hb[j] = budget;
                    s_e[j] = -1;
                    s_qn[j] = -1;
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
            float sc = 1.f;
            if (valid) {                                            // a disallowed row and a row past the end load nothing
                const int64_t row = row0 + lane;
                if (scales) sc = scales[row];                       // issued with the row's code words
                const uintptr_t a = lo + (uintptr_t)(row * c_rs);
                unsigned w[NW];
                adc_fetch_row<NW>(a, lo, hi, M, w);
                adc_screen_row_sums<NV, ND>(w, (unsigned)(a & 3), lds_u, M, K, KQ, bad, even, odd);
            }
            unsigned long long mine = 0ull;                         // lane q: the hit word of pair q
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const bool keep = adc_screen_keep(adc_screen_sum_of<ND>(even, odd, q), prm[q], sc);
                const unsigned long long bl = __ballot(valid && keep && q < np);
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

// The stored hit words of one pair into positions, by one wave: 64 words per trip, a wave prefix of their popcounts.
// run: the pair's first slot.  Both list screens' fill passes walk their words with it.
__device__ __forceinline__ void adc_screen_lists_emit_words(const uint32_t* __restrict__ hits, int64_t hb, int64_t list_tiles, int64_t lo,
                                                            int64_t run, int64_t capacity, int64_t* __restrict__ out_i, int lane)
{
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
        const int64_t base = lo + t * kFsTile;
        while (w) {
            const int b = __builtin_ctz(w);
            w &= w - 1;
            if (slot < capacity) out_i[slot] = base + b;
            ++slot;
        }
        run += (int64_t)__shfl(incl, 63);
    }
}

// The fill pass: one wave per entry e, entries taken grid-stride.  first [entries]: the scanned counts.
inline __global__ __launch_bounds__(64 * kRangeWaves) void k_adc_screen_lists_fill(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow, const float* __restrict__ scales,
    const int64_t* __restrict__ list_off, int64_t n_lists, const int64_t* __restrict__ probes, int n_probe, int64_t p_rs, int64_t nq,
    const uint8_t* __restrict__ imgq, int64_t pitch, const AdcScreenPrm* __restrict__ prm_g, int M, int K,
    const int64_t* __restrict__ hoff, int64_t budget, const uint32_t* __restrict__ hits, const int64_t* __restrict__ first,
    int64_t capacity, int64_t* __restrict__ out_i)
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
            const uint8_t* iq = imgq + q * pitch;
            for (int64_t row0 = r.lo; row0 < r.hi; row0 += 64) {
                const unsigned long long bits = adc_screen_lists_step_bits(allow, row0, r.hi, n);
                const bool valid = (bits >> lane) & 1ull;
                const int64_t row = row0 + lane;
                int U = 0;
                float sc = 1.f;
                if (valid) {
                    if (scales) sc = scales[row];
                    const uint8_t* cr = codes + row * c_rs;         // row < n: bytes 0 .. M - 1 lie inside the matrix
                    for (int m = 0; m < M; ++m) {
                        unsigned c = cr[m];
                        if (c >= (unsigned)K) c = 0;                // the count pass raised the flag
                        U += (int)iq[m * K + c];
                    }
                }
                const bool hit = valid && adc_screen_keep(U, p, sc);
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
