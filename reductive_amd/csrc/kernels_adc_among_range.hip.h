// kernels_adc_among_range.hip.h -- ADC range search among given rows: of the rows that a list of candidate ids names per
// query, those within a radius (value <= thr) resp. at or above a similarity (value >= thr), as CSR in the order in which
// they were named (include/pqhip.h: pqhip_adc_among_range_f32_dev, pqhip_adc_ip_among_range_f32_dev; instantiated by
// pqhip_adc_among_range.hip).
//
// The producer is k_adc_among_u8's (kernels_adc_among.hip.h): the query's [M][K] table in LDS, the two lims words of the
// query clamped in the kernel, the workgroup's slice of the places (adc_lists_wg_slice) walked 1,024 places per trip,
// lane t of the workgroup at place base + t; the id is checked before any address is formed (-1 is padding, any other id
// outside [0, n) is skipped and flagged), then adc_fetch_row / adc_row_sum and the four value forms.  The consumer is the
// count / scan / fill of the range searches (kernels_adc_range.hip.h) with the hit bitmap of k_flat_range_among:
//   count  k_adc_among_range_u8<.., FILL = false>: a wave ballots its hits of a trip, keeps the ballot as the bitmap word
//          of (trip, wave) and adds its popcount; the workgroup leaves ONE count                  -> part[query][workgroup]
//   scan   k_adc_range_scan over part in (query, workgroup) order: lims and every workgroup's first slot, 64-bit
//   fill   <.., FILL = true>: a wave reads the 16 words of its trip -- its own word names the lanes that hit, the
//          popcounts of the words of the waves below it are the hits before them -- so a place that missed costs one
//          bit: no id, no row, no table lookup, and a trip without a hit is skipped after one 128-byte load.  The value
//          of a hit place is computed again (the same operations: the same bits) and stored at
//          base of the workgroup + hits of earlier trips + hits of lower waves + hits of lower lanes, iff below capacity.
// Places ascend over lanes, waves, trips and workgroups, so the entries of a query leave in the order named, whatever G.
//
// Bitmap slots.  Every workgroup of a query owns 16 ceil(per / 1,024) consecutive words (per = its slice length, the same
// for all): word 16 trip + wave.  The host sizes a query's bitmap from n_ids (a shared list: every trip has its words)
// resp. from a multiple of the mean range (lims given: it cannot see the ranges, and a longer range is legal).  A trip
// whose 16 words do not all lie inside has no mask -- a condition on the trip, so uniform over the workgroup: the fill
// pass looks at all of its places again under the same predicate and the 16 waves exchange their counts through LDS (one
// barrier per such trip, two alternating buffers).
#pragma once
#include "kernels_adc_range.hip.h"

namespace pqhip {

// The value of a named row, k_adc_among_u8's operation for operation but for the sign of a score (s the row sum over the
// query's table, x = extra[row] or 1, b = pb[row_list[row]]):
//   plain:     IP = false: s                              IP = true: fl(s * x)
//   RESIDUAL:  IP = false: fl(fl(b + x) - fl(s + s))      IP = true: fl(fl(b + s) * x)
// false: the row's list id lies outside [0, n_lists) -- the row is skipped and `bad` set.  row is in [0, n).
template <bool IP, bool RESIDUAL, int NV>
__device__ __forceinline__ bool adc_among_range_value(int64_t row, uintptr_t lo, uintptr_t hi, int64_t c_rs,
                                                      const float* __restrict__ extra, const int64_t* __restrict__ row_list,
                                                      int64_t n_lists, const float* __restrict__ pb, const float* lds_s, int M,
                                                      int K, bool& bad, float& v)
{
    float x = 1.f;
    int64_t l = 0;
    if constexpr (RESIDUAL) l = row_list[row];                      // issued with the row's code words, as x is
    if constexpr (IP) x = extra ? extra[row] : 1.f;
    else if constexpr (RESIDUAL) x = extra[row];
    const uintptr_t a = lo + (uintptr_t)(row * c_rs);
    unsigned w[NV + 1];
    adc_fetch_row<NV + 1>(a, lo, hi, M, w);
    float b = 0.f;
    if constexpr (RESIDUAL) {
        if ((uint64_t)l >= (uint64_t)n_lists) { bad = true; return false; }
        b = pb[l];
    }
    const float s = adc_row_sum<NV>(w, (unsigned)(a & 3), lds_s, M, K, bad);
    if constexpr (RESIDUAL) v = IP ? fmul(fadd(b, s), x) : fsub(fadd(b, x), fadd(s, s));
    else v = IP ? fmul(s, x) : s;
    return true;
}

// Grid (G, queries of the launch), 1,024 threads; dynamic LDS: the [M][K] table.  lut [queries][M][K]; thr [queries];
// lims [queries + 1] or null; bias [queries][b_rs] (RESIDUAL); part [queries][G]: counts out (count pass), first slots in
// (fill pass); hits [queries][bm_words].  out_i receives the id as named.
template <bool IP, bool RESIDUAL, int NV, bool FILL>
__global__ __launch_bounds__(1024) void k_adc_among_range_u8(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const float* __restrict__ lut,
    const float* __restrict__ extra /* [n]: scales (IP) or row terms (RESIDUAL, !IP), or null */, int M, int K,
    const float* __restrict__ thr, const int64_t* __restrict__ lims, const int64_t* __restrict__ ids, int64_t n_ids,
    const int64_t* __restrict__ row_list /* RESIDUAL: [n] */, int64_t n_lists, const float* __restrict__ bias /* RESIDUAL */,
    int64_t b_rs, int64_t* __restrict__ part, unsigned long long* __restrict__ hits, int64_t bm_words, int64_t capacity,
    float* __restrict__ out_v, int64_t* __restrict__ out_i, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    __shared__ int wcnt[2][kRangeWaves];                            // fill: the waves' hits of a trip without a mask
    __shared__ long long wsum[kRangeWaves];                         // count: the waves' totals
    const int MK = M * K;
    adc_stage_tables<1>(lds_s, lut + (size_t)blockIdx.y * MK, MK);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
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
    const float t = thr[blockIdx.y];
    const ListsSlice g = adc_lists_wg_slice(len);
    const int64_t* my_ids = ids + begin;
    unsigned long long* hq = hits + (size_t)blockIdx.y * bm_words;
    int64_t tw = (int64_t)blockIdx.x * ((g.per + 1023) / 1024) * kRangeWaves;   // the word of (trip 0, wave 0)
    const int64_t slot_wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    int64_t run = FILL ? range_uniform(part[slot_wg]) : 0;          // count: the wave's hits so far; fill: the trip's first slot
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    int par = 0;
    for (int64_t base = g.s0; base < g.s1; base += 1024, tw += kRangeWaves) {   // uniform over the workgroup
        const bool has_mask = tw + kRangeWaves <= bm_words;
        const int64_t c = base + threadIdx.x;
        bool look = c < g.s1;
        unsigned long long mine = 0;
        int before = 0, total = 0;
        if (FILL && has_mask) {
            const int cnt = lane < kRangeWaves ? __popcll(hq[tw + lane]) : 0;
            mine = hq[tw + wave];
#pragma unroll
            for (int u = 0; u < kRangeWaves; ++u) {
                const int x = __builtin_amdgcn_readlane(cnt, u);
                total += x;
                if (u < wave) before += x;
            }
            if (total == 0) continue;                               // no hit in the trip: no id or row is loaded
            look = look && ((mine >> lane) & 1ull);                 // a bit is only ever set for a place of the slice
        }
        float v = 0.f;
        int64_t row = 0;
        bool valid = false;
        if (look) {
            row = my_ids[c];                                        // begin + c < begin + len <= n_ids
            valid = (uint64_t)row < (uint64_t)n;
            if (!valid && row != -1) bad = true;
        }
        if (valid)                                                  // only now is an address formed: a row not named is not read
            valid = adc_among_range_value<IP, RESIDUAL, NV>(row, lo, hi, c_rs, extra, row_list, n_lists, pb, lds_s, M, K, bad, v);
        // a place with a mask bit passed this predicate in the count pass, on the same bits
        const bool hit = valid && ((FILL && has_mask) || (IP ? v >= t : v <= t));
        if constexpr (!FILL) {
            const unsigned long long b = __ballot(hit);
            if (has_mask && lane == 0) hq[tw + wave] = b;
            run += (int64_t)__popcll(b);
        } else {
            unsigned long long b = mine;
            if (!has_mask) {
                b = __ballot(hit);
                if (lane == 0) wcnt[par][wave] = __popcll(b);
                __syncthreads();
#pragma unroll
                for (int u = 0; u < kRangeWaves; ++u) {
                    const int x = wcnt[par][u];
                    total += x;
                    if (u < wave) before += x;
                }
                par ^= 1;
            }
            if (hit) {
                const int64_t slot = run + before + (int64_t)range_rank(b);
                if (slot < capacity) { out_v[slot] = v; out_i[slot] = row; }
            }
            run += total;
        }
    }
    if constexpr (!FILL) {
        if (lane == 0) wsum[wave] = run;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long sum = 0;
#pragma unroll
            for (int u = 0; u < kRangeWaves; ++u) sum += wsum[u];
            part[slot_wg] = sum;
        }
    }
    if (bad) atomicOr(err, 1);
}

}  // namespace pqhip
