// kernels_rows_compact.hip.h -- stable compaction of a row array under a row mask (include/pqhip.h:
// pqhip_rows_compact_dev): output row j is the j-th kept row of the input, rows copied byte for byte.  (Launched from
// exactly one translation unit, pqhip_rows_compact.hip.)
//
// Three kernels in stream order; no workgroup waits for another.  The source rows are cut into G slices of `per` rows,
// per a multiple of the tile (1,024 rows = 32 mask words), one slice per workgroup of the count and of the move kernel.
//     k_rows_compact_count   the kept rows of every tile (tile_cnt, 32 bits each) and of every slice (ctl[1 + g])
//     k_rows_compact_scan    one workgroup: slice counts -> first output row of each slice (in place) and the total;
//                            d_count; the check of d_off_in (off[0] == 0, non-decreasing, off[n_lists] == n) and
//                            d_off_out[l] = kept rows below off[l] (slice prefix + tile counts + a popcount over at most
//                            32 words); ctl[0] = 1 iff the offsets are valid and the total fits the capacity
//     k_rows_compact_move    returns at once unless ctl[0] == 1, so after a bad offset array or with too small a
//                            capacity no row is read and no output byte written
// The mover is source-major.  A workgroup walks its slice tile by tile; per tile one wave turns the 32 words into an
// exclusive popcount prefix, every thread ranks its four rows and writes the rows it keeps into the tile's list in LDS
// (rank -> row of the tile; 2 KB, whatever the row width) and, if asked, their numbers to d_src_rows.  The tile's output
// bytes are one contiguous range; it is cut into 16-byte chunks on the 16-byte grid of the DESTINATION ADDRESS, a chunk
// per lane and pass.  A chunk is assembled in registers from the rows it covers: every piece is one 16-byte load at the
// byte address that puts the piece's bytes where the chunk wants them (the device is in unaligned access mode; the
// bytes around the piece belong to neighbouring rows of the input and are masked off), or, within 16 bytes of either
// end of the input, single byte loads -- no byte outside the n row_bytes input bytes is read.  Rows that follow each
// other in the source are one piece.  A whole chunk goes out as one aligned 16-byte store; the ragged first and last
// chunk of a tile as bytes.  With rows and addresses on multiples of 16 bytes this is one load and one store per chunk,
// straight from global to global.  The value of an output byte is a function of its position alone, so the result does
// not depend on the grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pqhip {

constexpr int kCompactThreads = 256;
constexpr int kCompactTile = 1024;        // rows of a tile: 32 mask words, four rows per thread of the mover

// the mask word that starts at row `first`, bits at or beyond row `end` cleared (0 if it starts there or later)
__device__ inline uint32_t compact_word(const uint32_t* __restrict__ keep, int64_t first, int64_t end)
{
    if (first >= end) return 0;
    uint32_t x = keep[first >> 5];
    const int64_t left = end - first;
    if (left < 32) x &= (1u << (int)left) - 1u;
    return x;
}

__global__ __launch_bounds__(kCompactThreads) void k_rows_compact_count(const uint32_t* __restrict__ keep, int64_t n, int64_t per,
                                                                        int64_t* __restrict__ slice_cnt,
                                                                        uint32_t* __restrict__ tile_cnt)
{
    __shared__ int64_t s_part[kCompactThreads / 32];
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < n ? r0 + per : n;
    const int64_t n_tiles = (r1 - r0 + kCompactTile - 1) / kCompactTile;
    const int group = threadIdx.x >> 5, gl = threadIdx.x & 31;      // 32 lanes share a tile, one word each
    int64_t acc = 0;
    for (int64_t base = 0; base < n_tiles; base += kCompactThreads / 32) {
        const int64_t t = base + group;
        int c = t < n_tiles ? __popc(compact_word(keep, r0 + t * kCompactTile + gl * 32, r1)) : 0;
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (gl == 0 && t < n_tiles) {
            tile_cnt[(r0 >> 10) + t] = (uint32_t)c;
            acc += c;
        }
    }
    if (gl == 0) s_part[group] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int i = 0; i < kCompactThreads / 32; ++i) s += s_part[i];
        slice_cnt[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(1024) void k_rows_compact_scan(int64_t* __restrict__ ctl, int64_t n_slices,
                                                            const uint32_t* __restrict__ tile_cnt,
                                                            const uint32_t* __restrict__ keep, int64_t n, int64_t per,
                                                            int64_t capacity, const int64_t* __restrict__ off_in, int64_t n_lists,
                                                            int64_t* __restrict__ off_out, int64_t* __restrict__ count,
                                                            int* __restrict__ err)
{
    __shared__ int64_t s_sum[1024];
    int64_t* base = ctl + 1;
    const int tid = threadIdx.x;
    const int64_t chunk = (n_slices + 1023) / 1024;
    const int64_t g0 = tid * chunk < n_slices ? tid * chunk : n_slices;
    const int64_t g1 = g0 + chunk < n_slices ? g0 + chunk : n_slices;
    int64_t mine = 0;
    for (int64_t g = g0; g < g1; ++g) mine += base[g];
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    const int64_t total = s_sum[1023];
    int64_t run = s_sum[tid] - mine;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t c = base[g];
        base[g] = run;
        run += c;
    }
    bool bad = false;
    if (off_in) {
        for (int64_t l = tid; l <= n_lists; l += 1024) {
            const int64_t o = off_in[l];
            if (l == 0 && o != 0) bad = true;
            if (l < n_lists) {
                if (off_in[l + 1] < o) bad = true;
            } else if (o != n) {
                bad = true;
            }
        }
    }
    const int any = __syncthreads_or(bad ? 1 : 0);        // (the slice bases are visible to the workgroup behind it)
    if (off_in && off_out && !any) {
        for (int64_t l = tid; l <= n_lists; l += 1024) {
            const int64_t x = off_in[l];                  // inside [0, n]: the array is valid
            int64_t r = total;
            if (x < n) {
                const int64_t g = x / per;
                r = base[g];
                const int64_t tx = x >> 10;
                for (int64_t t = (g * per) >> 10; t < tx; ++t) r += tile_cnt[t];
                const int64_t wx = x >> 5;
                for (int64_t w = tx << 5; w < wx; ++w) r += __popc(keep[w]);
                const int bits = (int)(x & 31);
                if (bits) r += __popc(keep[wx] & ((1u << bits) - 1u));
            }
            off_out[l] = r;
        }
    }
    if (tid == 0) {
        count[0] = total;
        ctl[0] = !any && total <= capacity ? 1 : 0;
        if (any) atomicOr(err, 1);
    }
}

// the bytes [lo, hi) of an 8-byte word as a mask; lo and hi may lie outside [0, 8]
__device__ inline uint64_t compact_below(int k) { return k <= 0 ? 0ull : k >= 8 ? ~0ull : (1ull << (8 * k)) - 1ull; }

// the bytes [off, off + len) of the chunk (v0 = bytes 0 .. 7, v1 = bytes 8 .. 15) from the input bytes src, src + 1, ..
__device__ inline void compact_piece(const uint8_t* __restrict__ in, int64_t in_bytes, int64_t src, int off, int len,
                                     uint64_t& v0, uint64_t& v1)
{
    const int64_t at = src - off;
    if (at >= 0 && at + 16 <= in_bytes) {
        uint64_t t[2];
        __builtin_memcpy(t, in + at, 16);
        v0 |= t[0] & (compact_below(off + len) & ~compact_below(off));
        v1 |= t[1] & (compact_below(off + len - 8) & ~compact_below(off - 8));
    } else {
#pragma unroll 1
        for (int i = 0; i < len; ++i) {
            const uint64_t x = in[src + i];
            const int p = off + i;
            if (p < 8) v0 |= x << (8 * p); else v1 |= x << (8 * (p - 8));
        }
    }
}

__global__ __launch_bounds__(kCompactThreads) void k_rows_compact_move(const int64_t* __restrict__ ctl,
                                                                       const uint32_t* __restrict__ keep, int64_t n, int64_t per,
                                                                       uint32_t rb, const uint8_t* __restrict__ in,
                                                                       uint8_t* __restrict__ out, int64_t* __restrict__ src_rows)
{
    if (ctl[0] != 1) return;
    __shared__ uint32_t s_word[32];
    __shared__ uint32_t s_pre[33];
    __shared__ uint16_t s_list[kCompactTile];
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < n ? r0 + per : n;
    const int64_t in_bytes = n * (int64_t)rb;
    const int tid = threadIdx.x;
    int64_t o_row = ctl[1 + blockIdx.x];        // first output row of the tile
    for (int64_t t0 = r0; t0 < r1; t0 += kCompactTile) {
        if (tid < 64) {                          // one wave: the words of the tile and their exclusive popcount prefix
            const uint32_t x = tid < 32 ? compact_word(keep, t0 + tid * 32, r1) : 0u;
            const int c = __popc(x);
            int inc = c;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int y = __shfl_up(inc, d);
                if (tid >= d) inc += y;
            }
            if (tid < 32) {
                s_word[tid] = x;
                s_pre[tid] = (uint32_t)(inc - c);
            }
            if (tid == 31) s_pre[32] = (uint32_t)inc;
        }
        __syncthreads();
        {
            const int w = tid >> 3, sh = (tid & 7) * 4;
            const uint32_t x = s_word[w];
            uint32_t k = s_pre[w] + __popc(x & ((1u << sh) - 1u));
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if ((x >> (sh + b)) & 1u) {
                    s_list[k] = (uint16_t)(tid * 4 + b);
                    if (src_rows) src_rows[o_row + k] = t0 + tid * 4 + b;
                    ++k;
                }
            }
        }
        __syncthreads();
        const uint32_t cnt = s_pre[32];
        if (in && cnt) {
            uint8_t* dst = out + o_row * (int64_t)rb;                   // the tile's output bytes: [dst, dst + bytes)
            const int pre = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
            const int32_t bytes = (int32_t)(cnt * rb);                  // at most 1,024 x 4,096
            const int32_t n_chunks = (bytes + pre + 15) >> 4;
            for (int32_t c = tid; c < n_chunks; c += kCompactThreads) {
                const int32_t cs = c * 16 - pre;                        // the chunk covers tile bytes [cs, cs + 16)
                const int first = cs < 0 ? -cs : 0;
                const int last = bytes - cs < 16 ? bytes - cs : 16;
                const uint32_t lo = (uint32_t)(cs + first), hi = (uint32_t)(cs + last);
                uint32_t j = lo / rb;
                uint32_t within = lo - j * rb;
                const uint32_t jl = (hi - 1) / rb;
                uint64_t v0 = 0, v1 = 0;
                if ((uint32_t)(s_list[jl] - s_list[j]) == jl - j) {     // rows that follow each other in the source
                    compact_piece(in, in_bytes, (t0 + s_list[j]) * (int64_t)rb + within, first, last - first, v0, v1);
                } else {
                    uint32_t pos = lo;
                    while (pos < hi) {
                        const uint32_t len = rb - within < hi - pos ? rb - within : hi - pos;
                        compact_piece(in, in_bytes, (t0 + s_list[j]) * (int64_t)rb + within, (int)(pos - (uint32_t)cs),
                                      (int)len, v0, v1);
                        pos += len;
                        within = 0;
                        ++j;
                    }
                }
                if (last - first == 16) {
                    *reinterpret_cast<uint4*>(dst + cs) =
                        make_uint4((unsigned)v0, (unsigned)(v0 >> 32), (unsigned)v1, (unsigned)(v1 >> 32));
                } else {
                    for (int i = first; i < last; ++i)
                        dst[cs + i] = (uint8_t)((i < 8 ? v0 >> (8 * i) : v1 >> (8 * (i - 8))) & 0xff);
                }
            }
        }
        o_row += cnt;
        __syncthreads();
    }
}

}  // namespace pqhip
