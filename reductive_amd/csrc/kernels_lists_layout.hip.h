// kernels_lists_layout.hip.h -- building a partitioned index on the device (include/pqhip.h: pqhip_lists_layout_dev,
// pqhip_residuals_f32_dev, pqhip_residual_terms_f32_dev).  (Launched from exactly one translation unit,
// pqhip_lists_layout.hip.)
//
// LAYOUT: a counting sort of n list ids on a key of at most 14 bits, stable by construction.  Workgroup g of G owns the
// contiguous rows [g per, (g + 1) per), per <= 2^31.
//     k_layout_count    counts the slice into LDS (atomics: a count has no order) and writes counts[g][l]; it is the pass
//                       that validates the ids: bad[g] = 1 and the stream's range flag if one lies outside [0, n_lists).
//     k_layout_columns  one thread per list: counts[g][l] becomes the number of rows of list l in the slices before g,
//                       totals[l] the size of the list.
//     k_layout_offsets  one workgroup: the validity word (no slice bad AND the totals sum to n), list_off = exclusive
//                       scan of the totals.
//     k_layout_place    returns at once unless the validity word is 1.  Each workgroup walks its slice again IN ROW ORDER,
//                       256 rows at a time.  A lane's rank among the lanes of its wave that hold the same id comes from
//                       a match over the id's bits with 64-bit ballots; the ranks across the four waves come from the
//                       waves adding their group sizes to the cursor table cur[l] in LDS (rows of list l placed so far by
//                       this workgroup) ONE WAVE AFTER THE OTHER, a barrier between two waves.  No atomics: their order
//                       is not the row order.  position = list_off[l] + counts[g][l] + cur[l] + rank.
// The position of a row is a function of the ids alone (the number of rows with a smaller id, plus the number of earlier
// rows with the same id), so the result does not depend on G.
//
// RESIDUALS: out[i][j] = x[i][j] - centroids[assign[i]][j], one IEEE subtraction per element.  An item is four
// consecutive columns of one row: a 16-byte load of x and of the centroid and a 16-byte store where all three addresses
// are multiples of 16, element by element otherwise (unaligned rows, the tail of d % 4 columns).
//
// TERMS: t_i = (float) sum_m p_im, p_im = sum_e (r r + 2 c r) in f64, sequential in e and then in m, no fused
// multiply-add.  One lane per (row, subquantizer) computes p_im into LDS -- the lanes of a row read adjacent bytes of
// the code row and adjacent sub-vectors of the centroid row --, then one lane per row folds the M partial sums in order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pqhip {

constexpr int kLayoutThreads = 256;
constexpr int kLayoutWaves = kLayoutThreads / 64;
constexpr int kLayoutUnroll = 4;          // tiles of 256 rows whose ids a workgroup loads before it places them
constexpr int kResidualThreads = 256;
constexpr int kResidualRows = 16;         // rows per block of k_residuals
constexpr int kTermsThreads = 256;

template <typename T>
__global__ __launch_bounds__(kLayoutThreads) void k_layout_count(const T* __restrict__ assign, int64_t n, int64_t per,
                                                                 int n_lists, int64_t* __restrict__ counts,
                                                                 int64_t* __restrict__ bad, int* __restrict__ err)
{
    extern __shared__ unsigned lds_cnt[];
    for (int l = threadIdx.x; l < n_lists; l += kLayoutThreads) lds_cnt[l] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * per < n ? (int64_t)blockIdx.x * per : n;
    const int64_t r1 = r0 + per < n ? r0 + per : n;
    bool wrong = false;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kLayoutThreads) {
        const int64_t key = (int64_t)assign[r];
        if (key < 0 || key >= n_lists) wrong = true;
        else atomicAdd(&lds_cnt[key], 1u);
    }
    const int any = __syncthreads_or(wrong ? 1 : 0);
    int64_t* mine = counts + (int64_t)blockIdx.x * n_lists;
    for (int l = threadIdx.x; l < n_lists; l += kLayoutThreads) mine[l] = (int64_t)lds_cnt[l];
    if (threadIdx.x == 0) {
        bad[blockIdx.x] = any ? 1 : 0;
        if (any) atomicOr(err, 1);
    }
}

__global__ __launch_bounds__(256) void k_layout_columns(int64_t* __restrict__ counts, int G, int n_lists,
                                                        int64_t* __restrict__ totals)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_lists) return;
    int64_t run = 0;
    int64_t* p = counts + l;
#pragma unroll 4
    for (int g = 0; g < G; ++g) {
        const int64_t c = p[(int64_t)g * n_lists];
        p[(int64_t)g * n_lists] = run;
        run += c;
    }
    totals[l] = run;
}

// one workgroup of 1,024 threads; n_lists <= 16,384 = 16 lists per thread
__global__ __launch_bounds__(1024) void k_layout_offsets(const int64_t* __restrict__ totals, const int64_t* __restrict__ bad,
                                                         int G, int n_lists, int64_t n, int64_t* __restrict__ valid,
                                                         int64_t* __restrict__ list_off, int* __restrict__ err)
{
    __shared__ int64_t part[1024];
    bool wrong = false;
    for (int g = threadIdx.x; g < G; g += 1024)
        if (bad[g] != 0) wrong = true;
    const int each = (n_lists + 1023) / 1024;
    const int l0 = threadIdx.x * each < n_lists ? threadIdx.x * each : n_lists;
    const int l1 = l0 + each < n_lists ? l0 + each : n_lists;
    int64_t sum = 0;
    for (int l = l0; l < l1; ++l) sum += totals[l];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int step = 1; step < 1024; step <<= 1) {           // inclusive scan of the partial sums
        const int64_t add = threadIdx.x >= step ? part[threadIdx.x - step] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - sum;
    for (int l = l0; l < l1; ++l) {
        list_off[l] = run;
        run += totals[l];
    }
    const int64_t all = part[1023];
    const int any = __syncthreads_or(wrong ? 1 : 0);
    if (threadIdx.x == 0) {
        list_off[n_lists] = all;
        const bool ok = !any && all == n;
        valid[0] = ok ? 1 : 0;
        if (!ok) atomicOr(err, 1);
    }
}

template <typename T>
__global__ __launch_bounds__(kLayoutThreads) void k_layout_place(const T* __restrict__ assign, int64_t n, int64_t per,
                                                                 int n_lists, int key_bits, const int64_t* __restrict__ valid,
                                                                 const int64_t* __restrict__ counts,
                                                                 const int64_t* __restrict__ list_off,
                                                                 int64_t* __restrict__ ids, int64_t* __restrict__ positions,
                                                                 int64_t* __restrict__ lists)
{
    extern __shared__ unsigned cur[];
    if (valid[0] != 1) return;
    for (int l = threadIdx.x; l < n_lists; l += kLayoutThreads) cur[l] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * per < n ? (int64_t)blockIdx.x * per : n;
    const int64_t r1 = r0 + per < n ? r0 + per : n;
    const int64_t* before = counts + (int64_t)blockIdx.x * n_lists;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int64_t base = r0; base < r1; base += kLayoutThreads * kLayoutUnroll) {
        int key[kLayoutUnroll];
        int64_t first[kLayoutUnroll];       // position of the first row of this list that this workgroup places
#pragma unroll
        for (int u = 0; u < kLayoutUnroll; ++u) {
            const int64_t r = base + u * kLayoutThreads + threadIdx.x;
            key[u] = -1;
            first[u] = 0;
            if (r < r1) {
                const int64_t a = (int64_t)assign[r];
                if (a >= 0 && a < n_lists) {               // (holds behind a valid count unless the ids changed since)
                    key[u] = (int)a;
                    first[u] = list_off[a] + before[a];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLayoutUnroll; ++u) {
            const bool live = key[u] >= 0;
            // the lanes of this wave with the same id
            unsigned long long same = __ballot(live);
            for (int b = 0; b < key_bits; ++b) {
                const unsigned long long set = __ballot(live && ((key[u] >> b) & 1));
                same &= ((key[u] >> b) & 1) ? set : ~set;
            }
            const unsigned rank = (unsigned)__popcll(same & below);
            const unsigned size = (unsigned)__popcll(same);
            const bool last = live && (same >> lane) <= 1ull;             // the highest lane of its group
            unsigned seen = 0;
            for (int w = 0; w < kLayoutWaves; ++w) {
                if (wave == w && live) {
                    seen = cur[key[u]];                                   // every lane of the group reads, then one adds
                    if (last) cur[key[u]] = seen + size;
                }
                __syncthreads();
            }
            if (live) {
                const int64_t r = base + u * kLayoutThreads + threadIdx.x;
                const int64_t p = first[u] + seen + rank;
                if (p >= 0 && p < n) {
                    positions[r] = p;
                    ids[p] = r;
                    if (lists) lists[p] = key[u];
                }
            }
        }
    }
}

__global__ __launch_bounds__(kResidualThreads) void k_residuals(const float* __restrict__ x, int64_t x_rs,
                                                                const int64_t* __restrict__ assign,
                                                                const float* __restrict__ centroids, int64_t n_lists,
                                                                int64_t n, int d, float* __restrict__ out, int64_t o_rs,
                                                                int* __restrict__ err)
{
    const int per_row = (d + 3) >> 2;                   // items of a row
    const int64_t n_blocks = (n + kResidualRows - 1) / kResidualRows;
    bool wrong = false;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t row0 = blk * kResidualRows;
        const int rows = n - row0 < kResidualRows ? (int)(n - row0) : kResidualRows;
        for (int it = threadIdx.x; it < rows * per_row; it += kResidualThreads) {
            const int rl = it / per_row, j0 = (it - rl * per_row) << 2;
            const int64_t i = row0 + rl;
            const int64_t a = assign[i];
            const float* xp = x + i * x_rs + j0;
            float* op = out + i * o_rs + j0;
            const int w = d - j0 < 4 ? d - j0 : 4;
            if (a < 0 || a >= n_lists) {
                wrong = true;
                for (int e = 0; e < w; ++e) op[e] = 0.0f;
                continue;
            }
            const float* cp = centroids + a * (int64_t)d + j0;
            const uintptr_t bits = reinterpret_cast<uintptr_t>(xp) | reinterpret_cast<uintptr_t>(op) | reinterpret_cast<uintptr_t>(cp);
            if (w == 4 && (bits & 15) == 0) {
                const float4 xv = *reinterpret_cast<const float4*>(xp);
                const float4 cv = *reinterpret_cast<const float4*>(cp);
                *reinterpret_cast<float4*>(op) = make_float4(xv.x - cv.x, xv.y - cv.y, xv.z - cv.z, xv.w - cv.w);
            } else {
                for (int e = 0; e < w; ++e) op[e] = xp[e] - cp[e];
            }
        }
    }
    if (wrong) atomicOr(err, 1);
}

// rows_per_wg rows per pass; dynamic LDS: rows_per_wg * M doubles
__global__ __launch_bounds__(kTermsThreads) void k_residual_terms(const float* __restrict__ cb, int M, int K, int ds,
                                                                  const uint8_t* __restrict__ codes, int64_t c_rs,
                                                                  const int64_t* __restrict__ assign,
                                                                  const float* __restrict__ centroids, int64_t n_lists,
                                                                  int64_t n, int rows_per_wg, float* __restrict__ out,
                                                                  int* __restrict__ err)
{
    extern __shared__ double part[];
    const int64_t d = (int64_t)M * ds;
    const int64_t n_blocks = (n + rows_per_wg - 1) / rows_per_wg;
    bool wrong = false;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t row0 = blk * rows_per_wg;
        const int rows = n - row0 < rows_per_wg ? (int)(n - row0) : rows_per_wg;
        for (int it = threadIdx.x; it < rows * M; it += kTermsThreads) {
            const int rl = it / M, m = it - rl * M;
            const int64_t i = row0 + rl;
            const int64_t a = assign[i];
            double p = 0.0;
            if (a >= 0 && a < n_lists) {
                int code = codes[i * c_rs + m];
                if (code >= K) { wrong = true; code = 0; }
                const float* rp = cb + ((int64_t)m * K + code) * ds;
                const float* cp = centroids + a * d + (int64_t)m * ds;
                for (int e = 0; e < ds; ++e) {
                    const double r = (double)rp[e], c = (double)cp[e];
                    p = __dadd_rn(p, __dadd_rn(__dmul_rn(r, r), __dmul_rn(__dmul_rn(2.0, c), r)));
                }
            } else {
                wrong = true;
            }
            part[it] = p;
        }
        __syncthreads();
        for (int rl = threadIdx.x; rl < rows; rl += kTermsThreads) {
            const int64_t a = assign[row0 + rl];
            double t = 0.0;
            if (a >= 0 && a < n_lists)
                for (int m = 0; m < M; ++m) t = __dadd_rn(t, part[rl * M + m]);
            out[row0 + rl] = (float)t;
        }
        __syncthreads();
    }
    if (wrong) atomicOr(err, 1);
}

}  // namespace pqhip
