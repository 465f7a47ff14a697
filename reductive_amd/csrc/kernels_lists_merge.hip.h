// kernels_lists_merge.hip.h -- merge of two list-ordered row arrays (include/pqhip.h: pqhip_lists_merge_dev): list l of the
// output is list l of `a` followed by list l of `b`, rows copied byte for byte.  (Launched from exactly one translation
// unit, pqhip_lists_merge.hip.)
//
// Two kernels.  k_lists_merge_plan (one workgroup) is the only reader of the two offset arrays.  It checks them --
// off[0] == 0, non-decreasing, off[n_lists] == n, which together keep every entry inside [0, n] -- and writes the table of
// the 2 n_lists output segments: segment 2 l is list l of a, segment 2 l + 1 list l of b.
//     table[0]                          1 = both arrays valid, 0 = not (the stream's range flag is raised as well)
//     seg_out [2 n_lists + 1]           first output row of the segment; the last entry is n_a + n_b
//     seg_src [2 n_lists]               (first source row << 1) | source array (0 = a, 1 = b)
// k_lists_merge_move returns at once unless table[0] == 1, so after a bad array no input byte is read and no output byte
// written.  It is destination-major: the output bytes are cut into 16-byte chunks on the 16-byte grid of the
// DESTINATION ADDRESS (chunk c covers output bytes [16 c - pre, 16 c - pre + 16), pre = address of out mod 16), workgroup
// g takes the chunks [ceil(C / G) g, ceil(C / G) (g + 1)), and lane t of a pass the chunk base + 256 u + t, u < 4.  A
// chunk that lies inside one segment -- all but at most two per segment -- is one 16-byte load at whatever byte
// address the source has (the device is in unaligned access mode; no byte outside the 16 is touched) and one aligned
// 16-byte store.  A chunk across a segment boundary is gathered byte by byte and still stored as one 16-byte store;
// only the chunks that hang over the first or the last output byte are stored as bytes.  The value of an output byte
// is a function of its position alone, so the result does not depend on the grid.  Lanes own chunks, not lists: a
// list shorter than a wave, an empty list (a segment no position falls into) and a list longer than a slice all cost
// the same per byte.  The workgroup finds the segment of its first byte by one binary search over seg_out; a lane then
// steps forward from segment to segment as its chunks advance (monotone), and searches again only when eight steps
// did not reach the position (many short lists between two chunks of a lane).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pqhip {

constexpr int kMergeThreads = 256;
constexpr int kMergeUnroll = 4;        // chunks in flight per lane: loads of a pass are issued before its stores

__global__ __launch_bounds__(1024) void k_lists_merge_plan(const int64_t* __restrict__ off_a, int64_t n_a,
                                                           const int64_t* __restrict__ off_b, int64_t n_b, int64_t n_lists,
                                                           int64_t* __restrict__ table, int64_t* __restrict__ off_out,
                                                           int* __restrict__ err)
{
    int64_t* seg_out = table + 1;
    int64_t* seg_src = seg_out + 2 * n_lists + 1;
    bool bad = false;
    for (int64_t l = threadIdx.x; l <= n_lists; l += 1024) {
        const int64_t a0 = off_a[l], b0 = off_b[l];
        if (l == 0 && (a0 != 0 || b0 != 0)) bad = true;
        const int64_t o0 = (int64_t)((uint64_t)a0 + (uint64_t)b0);        // (wraps only for an invalid array)
        if (off_out) off_out[l] = o0;
        seg_out[2 * l] = o0;
        if (l < n_lists) {
            const int64_t a1 = off_a[l + 1], b1 = off_b[l + 1];
            if (a1 < a0 || b1 < b0) bad = true;
            seg_src[2 * l] = (int64_t)((uint64_t)a0 << 1);
            seg_out[2 * l + 1] = (int64_t)((uint64_t)a1 + (uint64_t)b0);
            seg_src[2 * l + 1] = (int64_t)(((uint64_t)b0 << 1) | 1u);
        } else if (a0 != n_a || b0 != n_b) {
            bad = true;
        }
    }
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) {
        table[0] = any ? 0 : 1;
        if (any) atomicOr(err, 1);
    }
}

// a lane's place in the segment table: segment j holds the output bytes [.., end_b), and an output byte o of it is the
// byte o + delta of source array `which`
struct MergeCursor {
    const int64_t* seg_out;
    const int64_t* seg_src;
    int n_seg, j, which;
    int64_t rb, end_b, delta;

    __device__ void load_seg()
    {
        end_b = seg_out[j + 1] * rb;
        const int64_t s = seg_src[j];
        which = (int)(s & 1);
        delta = ((s >> 1) - seg_out[j]) * rb;
    }
    // the first segment >= lo that ends behind byte p (it exists for every p < total bytes)
    __device__ void find(int64_t p, int lo)
    {
        int hi = n_seg - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (seg_out[mid + 1] * rb > p) hi = mid; else lo = mid + 1;
        }
        j = lo;
        load_seg();
    }
    __device__ void seek(int64_t p)
    {
        if (p < end_b) return;
        for (int step = 0; step < 8 && j + 1 < n_seg; ++step) {
            ++j;
            if (seg_out[j + 1] * rb > p) { load_seg(); return; }
        }
        find(p, j + 1 < n_seg ? j + 1 : n_seg - 1);
    }
};

__global__ __launch_bounds__(kMergeThreads) void k_lists_merge_move(const int64_t* __restrict__ table, int n_seg, int64_t rb,
                                                                    const uint8_t* __restrict__ a, int64_t a_bytes,
                                                                    const uint8_t* __restrict__ b, int64_t b_bytes,
                                                                    uint8_t* __restrict__ out, int64_t total)
{
    if (table[0] != 1) return;
    const int pre = (int)(reinterpret_cast<uintptr_t>(out) & 15);
    const int64_t n_chunks = (total + pre + 15) >> 4;
    const int64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
    const int64_t c0 = (int64_t)blockIdx.x * per < n_chunks ? (int64_t)blockIdx.x * per : n_chunks;
    const int64_t c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
    if (c0 >= c1) return;
    MergeCursor cur;
    cur.seg_out = table + 1;
    cur.seg_src = cur.seg_out + n_seg + 1;
    cur.n_seg = n_seg;
    cur.rb = rb;
    cur.find(c0 * 16 - pre < 0 ? 0 : c0 * 16 - pre, 0);
    for (int64_t base = c0; base < c1; base += kMergeThreads * kMergeUnroll) {
        uint64_t lo[kMergeUnroll], hi[kMergeUnroll];
        int64_t at[kMergeUnroll];
        int first[kMergeUnroll], last[kMergeUnroll];          // the chunk's bytes [first, last) are output bytes
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u) {
            const int64_t c = base + u * kMergeThreads + threadIdx.x;
            lo[u] = hi[u] = 0;
            at[u] = c * 16 - pre;
            first[u] = last[u] = 0;
            if (c >= c1) continue;
            first[u] = at[u] < 0 ? (int)-at[u] : 0;
            last[u] = total - at[u] < 16 ? (int)(total - at[u]) : 16;
            cur.seek(at[u] + first[u]);
            const int64_t s = at[u] + cur.delta;
            if (first[u] == 0 && at[u] + 16 <= cur.end_b) {            // inside one segment: one load
                const int64_t lim = cur.which ? b_bytes : a_bytes;
                if (s >= 0 && s + 16 <= lim) {                          // holds by construction of the plan
                    uint64_t t[2];
                    __builtin_memcpy(t, (cur.which ? b : a) + s, 16);
                    lo[u] = t[0];
                    hi[u] = t[1];
                }
            } else {
#pragma unroll 1
                for (int i = first[u]; i < last[u]; ++i) {
                    const int64_t o = at[u] + i;
                    cur.seek(o);
                    const int64_t sb = o + cur.delta;
                    const int64_t lim = cur.which ? b_bytes : a_bytes;
                    uint64_t x = 0;
                    if (sb >= 0 && sb < lim) x = (cur.which ? b : a)[sb];
                    if (i < 8) lo[u] |= x << (8 * i); else hi[u] |= x << (8 * (i - 8));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u) {
            if (last[u] - first[u] == 16) {
                *reinterpret_cast<uint4*>(out + at[u]) =
                    make_uint4((unsigned)lo[u], (unsigned)(lo[u] >> 32), (unsigned)hi[u], (unsigned)(hi[u] >> 32));
            } else {
                for (int i = first[u]; i < last[u]; ++i)
                    out[at[u] + i] = (uint8_t)((i < 8 ? lo[u] >> (8 * i) : hi[u] >> (8 * (i - 8))) & 0xff);
            }
        }
    }
}

}  // namespace pqhip
