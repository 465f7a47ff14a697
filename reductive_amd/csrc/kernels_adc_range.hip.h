// kernels_adc_range.hip.h -- ADC range search: every row within a radius (dist <= thr) resp. at or above a similarity
// (score >= thr), exhaustive and over probed lists, as CSR (include/pqhip.h: pqhip_adc_*range*_f32_dev).
// (Launched from exactly one translation unit, pqhip_adc_range.hip.)
//
// A range call is the searches' producer with another consumer: the same table image in LDS, the same row fetch and row
// sums (adc_stage_tables, adc_fetch_row, adc_row_sum / adc_row_sum_mq + adc_spread_mq), the same mask bit, slices and
// segment walk (adc_mask_bit, adc_lists_wg_slice, adc_segment_start / adc_segment_seek: all of kernels_adc.hip.h), the
// same value formulas -- and in the place of the register lists, the LDS queues and the merge tree one compare per
// (row, query).  Nothing is ordered by value, so there is no key: the predicate is the IEEE comparison itself (a NaN
// never qualifies) and a value is stored bit for bit.
//
// Two passes over the codes with a scan between them, all three on the caller's stream:
//   count  every producer unit counts its qualifying rows per query            -> part[query][unit]
//   scan   one flat exclusive prefix over part in row-major order (k_adc_range_scan), in place: part becomes the first
//          output slot of every (query, unit), lims[q] the prefix at the first unit of query q
//   fill   the same walk over the same rows with the same predicate; a qualifying lane's slot is its unit's offset plus
//          the unit's matches in earlier trips plus the number of qualifying lanes below it (mbcnt of the ballot), and
//          it stores value and index iff slot < capacity.
// The producer unit is a WAVE with a contiguous sub-range of its workgroup's rows (a multiple of 64): units in ascending
// order cover ascending rows (exhaustive) resp. ascending places of the concatenation of the probed lists, and inside a
// unit trips ascend and lanes ascend, so the output order is ascending row index resp. the order of the concatenation
// whatever the grid -- and the row loop needs no workgroup barrier.  A wave still reads 64 consecutive rows per trip.
// Count and fill are one kernel; `fill` is a wave-uniform argument.  The mask is a wave-uniform branch too
// (allow == null: no filter): the bit is tested before the fetch, so a disallowed row loads no code, scale, row term or
// bias and cannot raise the range flag.
#pragma once
#include "kernels_adc.hip.h"

namespace pqhip {

constexpr int kRangeWaves = 16;   // waves (producer units) per 1,024-thread workgroup

enum : int { kRangeL2 = 0, kRangeIP = 1, kRangeResL2 = 2, kRangeResIP = 3 };

// lanes of `ballot` below this lane
__device__ __forceinline__ unsigned range_rank(unsigned long long ballot)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// a value every lane holds alike, moved to scalar registers (the offsets and counters of a wave are wave-uniform)
__device__ __forceinline__ int64_t range_uniform(int64_t v)
{
    const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(uint64_t)v);
    const unsigned h = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)h << 32) | l);
}

// One (wave, query) step of either pass: `hit` lanes are counted, and in the fill pass stored at run + rank -- iff that
// slot lies below capacity.  run is wave-uniform: the unit's matches so far, in the fill pass on top of its first slot
// (one counter serves both passes).
__device__ __forceinline__ void range_emit(bool hit, float v, int64_t id, bool fill, int64_t& run, int64_t capacity,
                                           float* __restrict__ out_v, int64_t* __restrict__ out_i)
{
    const unsigned long long b = __ballot(hit);
    if (fill && hit) {
        const int64_t slot = run + (int64_t)range_rank(b);
        if (slot < capacity) { out_v[slot] = v; out_i[slot] = id; }
    }
    run += (int64_t)__popcll(b);
}

// Exhaustive range search, NQ queries per pass.  IP = false: v = the scan's row sum, hit = v <= thr; IP = true:
// v = fl(s * scale[row]) (s without scales), hit = v >= thr.  Workgroup b owns rows [b rows_per_wg, (b + 1) rows_per_wg)
// (rows_per_wg a multiple of 1,024), its wave w the sub-range [w rows_per_wg / 16, (w + 1) rows_per_wg / 16) of it:
// unit u = 16 b + w.  part [NQ][units]: counts out (fill == 0), first slots in (fill == 1).
template <bool IP, int NV, int NQ>
__global__ __launch_bounds__(1024) void k_adc_range_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                       const uint32_t* __restrict__ allow /* or null */,
                                                       const float* __restrict__ lut /* [NQ][M][K] */,
                                                       const float* __restrict__ scales /* IP: [n] or null */,
                                                       const float* __restrict__ thr /* [NQ] */, int M, int K,
                                                       int64_t rows_per_wg, int fill, int64_t* __restrict__ part,
                                                       int64_t capacity, float* __restrict__ out_v,
                                                       int64_t* __restrict__ out_i, int* __restrict__ err)
{
    static_assert(NQ == 1 || NQ == 4 || NQ == 8, "queries per pass");
    constexpr int NW = NV + 1, NH = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    adc_stage_tables<NQ>(lds_s, lut, MK);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t unit = (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t sub = rows_per_wg / kRangeWaves;                  // a multiple of 64
    int64_t wg_end = ((int64_t)blockIdx.x + 1) * rows_per_wg;
    if (wg_end > n) wg_end = n;
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg + wave * sub;
    int64_t row_end = row_begin + sub;
    if (row_end > wg_end) row_end = wg_end;
    float t[NQ];
    int64_t run[NQ];                                                // count: matches so far; fill: the next slot
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        t[q] = thr[q];
        run[q] = fill ? part[q * units + unit] : 0;
    }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t b0 = row_begin; b0 < row_end; b0 += 64) {          // wave-uniform: the ballots are wave-wide
        const int64_t row = b0 + lane;
        bool valid = row < row_end;
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        float v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = 0.f;
        if (valid) {
            float sc = 1.f;
            if constexpr (IP) sc = scales ? scales[row] : 1.f;      // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            if constexpr (NQ == 1) {
                v[0] = adc_row_sum<NV>(w, sh, lds_s, M, K, bad);
            } else {
                f32x2 s[NH][2];
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) { s[hq][0] = (f32x2){0.f, 0.f}; s[hq][1] = (f32x2){0.f, 0.f}; }
                adc_row_sum_mq<NV, NH>(w, sh, lds_s, M, K, MK, bad, s);
                adc_spread_mq<NH>(s, v);
            }
            if constexpr (IP) {
                if (scales) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) v[q] = fmul(v[q], sc);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bool hit = valid && (IP ? v[q] >= t[q] : v[q] <= t[q]);
            range_emit(hit, v[q], row, fill != 0, run[q], capacity, out_v, out_i);
        }
    }
    if (!fill && lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) part[q * units + unit] = run[q];
    }
    if (bad) atomicOr(err, 1);
}

// Range search over probed lists: grid (G, queries), the walk of k_adc_search_lists_u8 -- the segment plan of
// k_adc_lists_plan, the workgroup's slice of the T concatenated probed rows (adc_lists_wg_slice) -- cut once more into
// 16 contiguous wave sub-ranges (a multiple of 64 places each).  Every lane maps its place to a row by stepping
// through the segments.  POL: kRangeL2 / kRangeIP the values of the flat list searches, kRangeResL2 / kRangeResIP
// those of the residual ones (bias [queries][b_rs], extra = row terms resp. scales); the bias is read per segment for a
// place that exists, so the bias of a skipped probe enters nothing.  part [queries][16 G].
template <int POL, int NV>
__global__ __launch_bounds__(1024) void k_adc_range_lists_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                             const uint32_t* __restrict__ allow /* or null */,
                                                             const float* __restrict__ lut,
                                                             const float* __restrict__ bias, int64_t b_rs,
                                                             const float* __restrict__ extra /* [n] or null */,
                                                             const float* __restrict__ thr /* [queries] */, int M, int K,
                                                             const int64_t* __restrict__ seg_begin,
                                                             const int64_t* __restrict__ seg_cum, int n_probe, int fill,
                                                             int64_t* __restrict__ part, int64_t capacity,
                                                             float* __restrict__ out_v, int64_t* __restrict__ out_i,
                                                             int* __restrict__ err)
{
    constexpr int NW = NV + 1;
    constexpr bool IP = POL == kRangeIP || POL == kRangeResIP, RES = POL == kRangeResL2 || POL == kRangeResIP;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    adc_stage_tables<1>(lds_s, lut + (size_t)blockIdx.y * MK, MK);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t units = (int64_t)gridDim.x * kRangeWaves;
    const int64_t slot_u = (int64_t)blockIdx.y * units + (int64_t)blockIdx.x * kRangeWaves + wave;
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const float* pb = RES ? bias + (int64_t)blockIdx.y * b_rs : nullptr;
    const float t = thr[blockIdx.y];
    const ListsSlice g = adc_lists_wg_slice(sc[n_probe]);
    const int64_t sub = ((g.per + kRangeWaves - 1) / kRangeWaves + 63) / 64 * 64;
    const int64_t s0 = g.s0 + wave * sub < g.s1 ? g.s0 + wave * sub : g.s1;
    const int64_t s1 = s0 + sub < g.s1 ? s0 + sub : g.s1;
    SegmentPos pos = adc_segment_start<RES>(sb, sc, pb, n_probe, s0, s1);
    int64_t run = fill ? range_uniform(part[slot_u]) : 0;           // count: matches so far; fill: the next slot
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t b0 = s0; b0 < s1; b0 += 64) {                      // wave-uniform: the ballot is wave-wide
        const int64_t c = b0 + lane;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            pos = adc_segment_seek<false, RES>(pos, c, sb, sc, pb, n_probe);
            row = c + pos.delta;
            valid = (uint64_t)row < (uint64_t)n;                    // holds by construction of the plan
        }
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        if (valid) {
            float x = 1.f;
            if constexpr (POL == kRangeResL2) x = extra[row];       // issued with the row's code words
            else if constexpr (IP) x = extra ? extra[row] : 1.f;
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const float s = adc_row_sum<NV>(w, (unsigned)(a & 3), lds_s, M, K, bad);
            if constexpr (POL == kRangeL2) v = s;
            else if constexpr (POL == kRangeIP) v = extra ? fmul(s, x) : s;
            else if constexpr (POL == kRangeResL2) v = fsub(fadd(pos.bias, x), fadd(s, s));
            else v = extra ? fmul(fadd(pos.bias, s), x) : fadd(pos.bias, s);
        }
        const bool hit = valid && (IP ? v >= t : v <= t);
        range_emit(hit, v, row, fill != 0, run, capacity, out_v, out_i);
    }
    if (!fill && lane == 0) part[slot_u] = run;
    if (bad) atomicOr(err, 1);
}

// In place, one workgroup: part[0 .. len) counts -> their exclusive prefix in flat order, started at lims[0] (the total
// of the queries before this launch; the host zeroes lims[0] of a call).  len = nq units: lims[q] receives the prefix at
// the first unit of query q and lims[nq] the running total -- the lims[0] of the next launch.  1,024 counts per trip
// with a carry, as k_adc_lists_plan sums its segments.
inline __global__ __launch_bounds__(1024) void k_adc_range_scan(int64_t* __restrict__ part, int64_t units, int64_t nq,
                                                         int64_t* __restrict__ lims)
{
    __shared__ long long wsum[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t len = units * nq;
    long long carry = lims[0];
    for (int64_t p0 = 0; p0 < len; p0 += 1024) {
        const int64_t p = p0 + threadIdx.x;
        const long long cnt = p < len ? part[p] : 0;
        long long v = cnt;                                      // inclusive scan over the wave, then over the 16 waves
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
        if (p < len) {
            const long long excl = carry + before + v - cnt;
            part[p] = excl;
            if (p % units == 0) lims[p / units] = excl;
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) lims[nq] = carry;
}

}  // namespace pqhip
