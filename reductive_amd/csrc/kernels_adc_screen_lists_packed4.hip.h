// kernels_adc_screen_lists_packed4.hip.h -- the one-hot i8 screen of kernels_adc_screen_packed4.hip.h over PROBED LISTS of
// 4-BIT PACKED rows (include/pqhip.h: pqhip_adc_screen_lists_packed4_f32_dev).  lims and idx are, bit for
// bit, what pqhip_adc_screen_lists_f32_dev returns on the unpacked codes.  (Instantiated by
// pqhip_adc_screen_lists_packed4.hip.)
//
// Screening value.  That of k_adc_screen_p4: U[row][q] = onehot(row) . IMG[q] on v_mfma_i32_32x32x32_i8, the image of a
// query stored as u - 128 with u and the parameters from adc_screen_prep_slot<uint8_t>, accumulators from 128 M, exact in
// int32.  The predicate is adc_screen_keep.  Neither depends on which queries share a group, which rows share a unit or
// where a unit starts, so the bound of §5e holds as it stands and the bits are those of the u8 list screen.
//
// Inversion and units are those of kernels_adc_screen_lists.hip.h, kernel for kernel (k_fsl_pairs, k_fsl_units,
// k_fsl_scatter, k_adc_range_scan over tiles and counts), with groups of 64 slots (32 for M > 64: kP4ScreenMaxBlocks).
//
// Preparation k_adc_screen_lists_p4_prep: one workgroup per query of the chunk; the image goes to the scratch QUERY-MAJOR
// and already in B-operand order: per k-step j < PB = ceil(M / 2) 32 bytes, the 16 entries of subquantizer 2 j, then the
// 16 of 2 j + 1; entries k >= K are -128 (u = 0), the pad subquantizer of an odd M is 0.  The pitch is 32 PB bytes.
//
// Count pass k_adc_screen_lists_p4: per unit the workgroup assembles the group's image in LDS as
//     [block of 32 slots][k-step j][lane][16 bytes],
// the layout k_adc_screen_p4 reads; a (slot, j, half) is one 16-byte copy from the scratch, so there is no byte transpose.
// The parameters, hit bases, entries and queries of the pairs sit behind the image; padding slots are zeros with
// ulim = -1 and never set a bit.  A workgroup whose next unit has the same (list, group) keeps the image.  The 16 waves
// take the unit's rows in tiles of 32 counted from the LIST'S first row (kFsTile): one tile is one hit word of a pair.
// The allow bits of a tile come from fsl_tile_bits at any bit offset; a disallowed row and a row past the list's end are
// never loaded.  The one-hot of a k-step is built once per tile and used for both query blocks; the second block is
// skipped while the group holds at most 32 pairs.  The epilogue is k_adc_screen_p4's: lanes l and l + 32 join their 16
// bits, lane l < 32 stores the word at hits[hoff[e] + tile] and adds its popcount to the unit's count, which goes to
// cnt[e] by one integer atomic per unit.  A pair whose words would not fit the budget is counted all the same.
//
// Fill pass k_adc_screen_lists_p4_fill: k_adc_screen_lists_fill with the packed row walk: stored words are turned into
// positions without reading codes (adc_screen_lists_emit_words); a pair without stored words has them formed again, for
// this query alone, from the packed rows and the query's image in the scratch -- the same integers, so the same bits.
#pragma once
#include "kernels_adc_screen_lists.hip.h"
#include "kernels_adc_screen_packed4.hip.h"

namespace pqhip {

// bytes of a query's image in the scratch: k-step j at byte 32 j
constexpr int64_t adc_screen_lists_p4_pitch(int M) { return (int64_t)32 * ((M + 1) / 2); }

// dynamic LDS of the count pass: the group's image, then per slot the parameters (16), the first hit word (8), the entry
// (4) and the query (4), then the unit's list (8, padded)
constexpr size_t adc_screen_lists_p4_lds_bytes(int M, int blocks) { return p4_screen_image_bytes(M, blocks) + (size_t)blocks * 32 * 32 + 16; }

inline __global__ __launch_bounds__(kAsPrepThreads) void k_adc_screen_lists_p4_prep(const float* __restrict__ tables, int M, int K,
                                                                             const float* __restrict__ thr, int ip, int scaled,
                                                                             const unsigned* __restrict__ cmax_bits,
                                                                             int8_t* __restrict__ imgq, int64_t pitch,
                                                                             AdcScreenPrm* __restrict__ prm)
{
    __shared__ uint8_t s_u[kAdcScreenMaxM * 16];
    const int64_t q = blockIdx.x;
    adc_screen_prep_slot<uint8_t>(tables + (size_t)q * M * K, true, M, K, thr + q, ip, scaled, cmax_bits, kAdcScreenSteps + 1, s_u,
                                  (size_t)1, prm + q);
    __syncthreads();
    const int PB = (M + 1) >> 1;
    int8_t* dst = imgq + q * pitch;
    for (int i = threadIdx.x; i < PB * 32; i += kAsPrepThreads) {   // byte i: subquantizer i / 16 (k-step m / 2, half m % 2), entry i % 16
        const int m = i >> 4, k = i & 15;
        dst[i] = (int8_t)(m < M ? (k < K ? (int)s_u[m * K + k] : 0) - 128 : 0);
    }
}

// The count pass (see the head of the file).  NV packed dwords per row (>= ceil(PB / 4)), QB blocks of 32 slots per
// group.  imgq / prm_g: the chunk's images [queries][pitch] and parameters [queries].  hoff [entries]: first hit word of
// a pair; hits [budget]; cnt [entries].
template <int NV, int QB>
__global__ __launch_bounds__(1024) void k_adc_screen_lists_p4(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow /* or null */,
    const float* __restrict__ scales /* [n] or null */, const int64_t* __restrict__ list_off, int64_t n_lists,
    const unsigned* __restrict__ lcnt, const unsigned* __restrict__ pair_off, const int64_t* __restrict__ unit_off,
    const unsigned* __restrict__ pairs, int n_probe, const uint8_t* __restrict__ imgq, int64_t pitch,
    const AdcScreenPrm* __restrict__ prm_g, int M, int K, int64_t unit_rows, const int64_t* __restrict__ hoff, int64_t budget,
    uint32_t* __restrict__ hits, unsigned long long* __restrict__ cnt, int* __restrict__ err)
{
    static_assert(QB >= 1 && QB <= kP4ScreenMaxBlocks, "blocks of 32 slots per group");
    constexpr int NW = NV + 1, NQ = 32 * QB;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_p[];
    const int PB = (M + 1) >> 1;
    const int step_bytes = PB * 1024;                               // one block's image
    AdcScreenPrm* prm = reinterpret_cast<AdcScreenPrm*>(lds_p + QB * step_bytes);
    int64_t* s_hb = reinterpret_cast<int64_t*>(prm + NQ);
    int* s_e = reinterpret_cast<int*>(s_hb + NQ);
    int* s_qn = s_e + NQ;
    int64_t* s_list = reinterpret_cast<int64_t*>(s_qn + NQ);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int half = lane >> 5, l32 = lane & 31;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + PB);     // one past the last code byte
    const bool full = K == 16;
    const int64_t total = unit_off[n_lists];
    int64_t held = -1;                                              // the first unit of the (list, group) whose image the LDS holds
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
        // a 64-bit quotient is formed by vector instructions: back to scalar registers, the accumulators need the others
        const int64_t chunks = range_uniform((r.hi - r.lo + unit_rows - 1) / unit_rows);
        const int64_t local = u - unit_off[l];
        const int64_t g = range_uniform(local / chunks), ci = local - g * chunks;
        const int np = __builtin_amdgcn_readfirstlane((int)((int64_t)lcnt[l] - g * NQ < NQ ? (int64_t)lcnt[l] - g * NQ : NQ));
        if (u - ci != held) {                                       // workgroup-uniform; the units of a (list, group) are consecutive
            const int64_t list_tiles = (r.hi - r.lo + kFsTile - 1) / kFsTile;
            if (threadIdx.x < NQ) {
                const int j = threadIdx.x;
                if (j < np) {
                    const unsigned e = pairs[pair_off[l] + g * NQ + j];
                    const int qn = (int)(e / (unsigned)n_probe);
                    prm[j] = prm_g[qn];
                    s_hb[j] = hoff[e] + list_tiles <= budget ? hoff[e] : -1;   // -1: the pair's words do not fit, it is counted only
                    s_e[j] = (int)e;
                    s_qn[j] = qn;
                } else {
                    prm[j] = AdcScreenPrm{-1, 0.f, 0.f, 0.f};
                    s_hb[j] = -1;
                    s_e[j] = -1;
                    s_qn[j] = -1;
                }
            }
            __syncthreads();
            // 16-byte item it of the image: slot 32 b + it % 32, half (it / 32) % 2, k-step j, block b = it / (64 PB)
            as_u32x4* dst = reinterpret_cast<as_u32x4*>(lds_p);
            for (int it = threadIdx.x; it < QB * PB * 64; it += 1024) {
                const int bj = it >> 6, b = bj / PB, j = bj - b * PB;
                const int qn = s_qn[32 * b + (it & 31)];
                as_u32x4 v = {0u, 0u, 0u, 0u};
                if (qn >= 0) v = *reinterpret_cast<const as_u32x4*>(imgq + (int64_t)qn * pitch + 32 * j + 16 * ((it >> 5) & 1));
                dst[it] = v;
            }
            __syncthreads();
            held = u - ci;
        }
        const bool two = QB > 1 && np > 32;                         // workgroup-uniform: the second block holds a pair
        const int64_t rb = r.lo + ci * unit_rows;                   // rb - r.lo is a multiple of 64: tiles are the list's
        const int64_t re = rb + unit_rows < r.hi ? rb + unit_rows : r.hi;
        unsigned cn[QB];                                            // lane l < 32: the unit's hits of slot 32 qb + l
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) cn[qb] = 0u;
        const int tile_end = (int)((re - r.lo + kFsTile - 1) >> 5);  // at most 2^27 tiles in a list
        for (int tile = (int)((rb - r.lo) >> 5) + wave; tile < tile_end; tile += kRangeWaves) {   // wave-uniform
            const int64_t row0 = r.lo + (int64_t)tile * kFsTile;
            const unsigned vmask = fsl_tile_bits(allow, row0, re, n);
            const bool valid = (vmask >> l32) & 1u;                 // both lane halves hold row row0 + l32
            unsigned w[NW];
#pragma unroll
            for (int k = 0; k < NW; ++k) w[k] = 0u;
            unsigned sh = 0u;
            float scm = 1.f;
            if (valid) {                                            // a disallowed row and a row past the end load nothing
                const int64_t row = row0 + l32;
                if (scales) scm = scales[row];                      // issued with the row's code words
                const uintptr_t a = lo + (uintptr_t)(row * c_rs);
                adc_fetch_row<NW>(a, lo, hi, PB, w);
                sh = (unsigned)(a & 3);
            }
            int lbo = lane * 16;                                    // this lane's B operand of k-step 0, block 0
            asm volatile("" : "+v"(lbo));                           // formed per tile: no operand address of a k-step is kept over the loop
            const uint8_t* lb = lds_p + lbo;
            int start = 128 * M;
            asm volatile("" : "+v"(start));                         // set per tile: a start held over the loop takes 16 registers per block
            p4s_i32x16 acc[QB];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[qb][i] = start;
            if (vmask != 0u) {                                      // no row to screen: the words are still written
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);   // bytes 4k .. 4k+3 of the row: k-steps 4k .. 4k+3
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = 4 * k + e;
                        if (j < PB) {
                            const unsigned c = (v >> (8 * e + 4 * half)) & 0xfu;
                            if (!full) {
                                if (valid && c >= (unsigned)K && 2 * j + half < M) bad = true;   // the pad nibble is nobody's code
                            }
                            const unsigned bit = 1u << (8u * (c & 3u)), d = c >> 2;
                            const p4s_i32x4 onehot = {d == 0u ? (int)bit : 0, d == 1u ? (int)bit : 0, d == 2u ? (int)bit : 0, d == 3u ? (int)bit : 0};
#pragma unroll
                            for (int qb = 0; qb < QB; ++qb) {
                                if (qb == 0 || two) {
                                    const p4s_i32x4 b = *reinterpret_cast<const p4s_i32x4*>(lb + qb * step_bytes + j * 1024);
                                    acc[qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(onehot, b, acc[qb], 0, 0, 0);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);      // no operand of a later k-step is fetched ahead: the registers are the accumulators'
                        }
                    }
                }
            }
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                const int slot = qb * 32 + l32;
                unsigned bits = 0u;
                if (vmask != 0u && (qb == 0 || two)) {
                    int po = slot * (int)sizeof(AdcScreenPrm);
                    asm volatile("" : "+v"(po));                    // read per tile: four registers, not four per block kept over the loop
                    const AdcScreenPrm p = *reinterpret_cast<const AdcScreenPrm*>(reinterpret_cast<const uint8_t*>(prm) + po);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int ri = 8 * (i >> 2) + (i & 3) + 4 * half;   // the accumulator's row of the tile
                        const float sc = scales ? __shfl(scm, ri) : 1.f;    // lane ri < 32 holds row ri; 1 for a row not loaded
                        if (adc_screen_keep(acc[qb][i], p, sc)) bits |= 1u << ri;
                        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four rows in flight: the other accumulators keep their registers
                    }
                    bits |= (unsigned)__shfl_xor((int)bits, 32);    // the complementary rows of the same query
                    bits &= vmask;
                }
                if (lane < 32 && slot < np) {                       // a padding slot has no hits and no words
                    const int64_t hb = s_hb[slot];
                    if (hb >= 0) hits[hb + tile] = bits;
                    cn[qb] += (unsigned)__popc(bits);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (lane < 32) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
                if (qb * 32 + l32 < np && cn[qb] != 0u) atomicAdd(&cnt[s_e[qb * 32 + l32]], (unsigned long long)cn[qb]);
        }
    }
    if (bad) atomicOr(err, 1);
}

// The fill pass: one wave per entry e, entries taken grid-stride; k_adc_screen_lists_fill over packed rows.  first
// [entries]: the scanned counts.  imgq: the chunk's images as the prep kernel wrote them.
inline __global__ __launch_bounds__(64 * kRangeWaves) void k_adc_screen_lists_p4_fill(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow, const float* __restrict__ scales,
    const int64_t* __restrict__ list_off, int64_t n_lists, const int64_t* __restrict__ probes, int n_probe, int64_t p_rs, int64_t nq,
    const int8_t* __restrict__ imgq, int64_t pitch, const AdcScreenPrm* __restrict__ prm_g, int M,
    const int64_t* __restrict__ hoff, int64_t budget, const uint32_t* __restrict__ hits, const int64_t* __restrict__ first,
    int64_t capacity, int64_t* __restrict__ out_i)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int PB = (M + 1) >> 1;
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
            const int8_t* iq = imgq + q * pitch;
            for (int64_t row0 = r.lo; row0 < r.hi; row0 += 64) {
                const unsigned long long bits = adc_screen_lists_step_bits(allow, row0, r.hi, n);
                const bool valid = (bits >> lane) & 1ull;
                const int64_t row = row0 + lane;
                int U = 128 * M;
                float sc = 1.f;
                if (valid) {
                    if (scales) sc = scales[row];
                    const uint8_t* cr = codes + row * c_rs;         // row < n: bytes 0 .. PB - 1 lie inside the matrix
                    for (int j = 0; j < PB; ++j) {                  // entries >= K are -128 (u = 0), the pad subquantizer's are 0
                        const unsigned c = cr[j];
                        U += (int)iq[32 * j + (c & 15u)] + (int)iq[32 * j + 16 + (c >> 4)];
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
