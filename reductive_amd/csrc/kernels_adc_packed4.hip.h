// kernels_adc_packed4.hip.h -- ADC search over 4-bit packed codes (include/pqhip.h: "4-bit packed codes"), and the
// kernels that pack and unpack them.  (The exhaustive producers are launched from pqhip_adc_packed4.hip, the list
// producers from pqhip_adc_packed4_lists.hip; both define PQHIP_ADC_TEMPLATES_ONLY.)
//
// Format.  A row of M codes, each < K <= 16, is PB = ceil(M / 2) bytes: code m is nibble m & 1 (0 = low) of byte m >> 1.
// The high nibble of the last byte of an odd M is written as 0 and never looked at.  Rows are `stride` >= PB bytes
// apart; nothing is assumed of the base address or of the stride.
//
// Definition.  Every producer here is a sibling of a u8 producer -- k_adc_search_u8 and k_adc_search_lists_u8 with
// their IP, RESIDUAL and MASKED flags -- and offers, for every row, the value that sibling offers for the unpacked row:
// the row sum is the same sequential f32 chain over m = 0 .. M-1 from +0 (one table entry per code, never a sum of two
// entries looked up by a whole byte), a nibble >= K raises the range flag and reads entry 0, and the score / residual
// arithmetic is the siblings' operation for operation.  Selection (SearchState, offer, search_finish), the mask bit,
// the slices and the segment walk (adc_mask_bit, adc_lists_wg_slice, adc_segment_start / adc_segment_seek of
// kernels_adc.hip.h) and the order are shared with them; the partial lists go to the same merge kernel.  So a packed
// search returns, bit for bit, what the u8 search returns on the unpacked codes.  The bodies stay apart from the u8
// ones because the code format differs: another table image, another row sum, and flags that are run-time null pointers
// here (below).
//
// What differs.  adc_fetch_row is called with PB in the place of M (it takes a byte count): NV counts packed dwords,
// eight codes each.  The table image in LDS has a stride of 16 entries per m whatever K is -- [M][16] f32 for one
// query, [NQ / 4][M][16][4] for 4 / 8 queries -- so lookup m is the base plus an immediate plus the nibble scaled:
// one shift and one mask per code.  Sixteen consecutive dwords are sixteen banks and equal addresses broadcast, so the
// gather has no bank conflict whatever the codes are.  Entries K .. 15 of a row are never staged and never read.
// When K == 16 no nibble can be out of range and the compare is skipped (a wave-uniform branch).  The row mask and the
// scales are wave-uniform branches on a null pointer as well, not template parameters, and the list producer takes the
// probe bias the same way: one body serves the plain and the residual searches.
#pragma once
#include "kernels_adc_search.hip.h"

namespace pqhip {

constexpr int kPacked4MaxValueWords = 13;   // M <= 100: 50 bytes per row

// [M][K] table of one query -> [M][16] image
__device__ __forceinline__ void p4_stage_table(float* lds, const float* __restrict__ lut, int M, int K)
{
    for (int i = threadIdx.x; i < M * K; i += 1024) {
        const int m = i / K, c = i - m * K;
        lds[m * 16 + c] = lut[i];
    }
}

// [NQ][M][K] tables -> [NQ / 4][M][16][4] image, the four queries of a group side by side
template <int NQ>
__device__ __forceinline__ void p4_stage_tables_mq(float* lds, const float* __restrict__ lut, int M, int K)
{
    const int MK = M * K;
    for (int i = threadIdx.x; i < NQ * MK; i += 1024) {
        const int q = i / MK, r = i - q * MK;
        const int m = r / K, c = r - m * K;
        lds[(((q >> 2) * M + m) * 16 + c) * 4 + (q & 3)] = lut[i];
    }
}

// sum over m = 0 .. M-1, in order, from +0, of the entry of code m, for the packed row fetched by adc_fetch_row (shift
// sh = a & 3); lm is the [M][16] image.  FULL (K == 16): no range check.  Else a nibble >= K sets `bad` and reads
// entry 0; K4 = 4 K.  The pad nibble of an odd M is code M and is not reached.
template <int NV, bool FULL>
__device__ __forceinline__ float adc_row_sum_p4(const unsigned (&w)[NV + 1], unsigned sh, const float* lm, int M, unsigned K4, bool& bad)
{
    const char* lb = reinterpret_cast<const char*>(lm);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);   // bytes 4k .. 4k+3 of the row: codes 8k .. 8k+7
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (8 * k + e < M) {
                unsigned o = ((v >> (4 * e)) & 0xfu) << 2;                 // 4 * nibble e: one shift and one mask
                if (!FULL) {
                    if (o >= K4) { bad = true; o = 0; }
                }
                s = fadd(s, *reinterpret_cast<const float*>(lb + (8 * k + e) * 64 + o));
            }
        }
    }
    return s;
}

// The same sum for 4 NH queries over the [NH][M][16][4] image, added onto s (the caller's +0); s as in adc_row_sum_mq:
// each query's sum is its own sequential f32 chain over m.  K16 = 16 K.
template <int NV, int NH, bool FULL>
__device__ __forceinline__ void adc_row_sum_p4_mq(const unsigned (&w)[NV + 1], unsigned sh, const float* lm, int M, unsigned K16,
                                                  bool& bad, f32x2 (&s)[NH][2])
{
    const char* lb = reinterpret_cast<const char*>(lm);
    const int group = M * 256;                                              // bytes of one group's image
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const unsigned v = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (8 * k + e < M) {
                unsigned o = ((v >> (4 * e)) & 0xfu) << 4;                 // 16 * nibble e
                if (!FULL) {
                    if (o >= K16) { bad = true; o = 0; }
                }
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(lb + hq * group + (8 * k + e) * 256 + o);
                    s[hq][0] = pk_add(s[hq][0], (f32x2){t[0], t[1]});
                    s[hq][1] = pk_add(s[hq][1], (f32x2){t[2], t[3]});
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Exhaustive producers: k_adc_search_u8 over packed rows, with its row mask when allow != null.  NV = packed dwords
// per row (>= ceil(PB / 4)); LDS: the table image (NQ M 64 bytes), then the queues [16][NQ][kSearchQueue] keys and
// indices; later the combine lists.
// ---------------------------------------------------------------------------------------------
template <bool IP, int NV, int NQ, int L>
__global__ __launch_bounds__(1024) void k_adc_search_p4(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                        const uint32_t* __restrict__ allow /* or null */,
                                                        const float* __restrict__ lut /* [NQ][M][K] */,
                                                        const float* __restrict__ scales /* IP: [n] or null */, int M, int K,
                                                        int kk, int64_t rows_per_wg, unsigned* __restrict__ part_k,
                                                        uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    static_assert(NQ == 1 || NQ == 4 || NQ == 8, "queries per pass");
    constexpr int NW = NV + 1, NH = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    if (NQ == 1) p4_stage_table(lds_s, lut, M, K);
    else p4_stage_tables_mq<NQ>(lds_s, lut, M, K);
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + NQ * M * 16);   // [16][NQ][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * NQ * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    const int PB = (M + 1) >> 1;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + PB);     // one past the last code byte
    const bool full = K == 16;
    const unsigned KS = (unsigned)K * (NQ == 1 ? 4u : 16u);
    bool bad = false;
    for (int64_t base = row_begin; base < row_end; base += 1024) {  // wave-uniform trip count: the selection is wave-wide
        const int64_t row = base + threadIdx.x;
        bool valid = row < row_end;
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        float val[NQ];                                              // distance, or -score
#pragma unroll
        for (int q = 0; q < NQ; ++q) val[q] = 0.f;
        if (valid) {
            float sc = 1.f;
            if constexpr (IP) sc = scales ? scales[row] : 1.f;
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, PB, w);
            const unsigned sh = (unsigned)(a & 3);
            if constexpr (NQ == 1) {
                val[0] = full ? adc_row_sum_p4<NV, true>(w, sh, lds_s, M, KS, bad)
                              : adc_row_sum_p4<NV, false>(w, sh, lds_s, M, KS, bad);
            } else {
                f32x2 s[NH][2];
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) { s[hq][0] = (f32x2){0.f, 0.f}; s[hq][1] = (f32x2){0.f, 0.f}; }
                if (full) adc_row_sum_p4_mq<NV, NH, true>(w, sh, lds_s, M, KS, bad, s);
                else adc_row_sum_p4_mq<NV, NH, false>(w, sh, lds_s, M, KS, bad, s);
                adc_spread_mq<NH>(s, val);
            }
            if constexpr (IP) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) val[q] = -fmul(val[q], sc);
            }
        }
        const unsigned off = (unsigned)(row - row_begin);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            st[q].offer(val[q], off, valid, qk + (wave * NQ + q) * kSearchQueue, qi + (wave * NQ + q) * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<NQ, L>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), row_begin, part_k, part_i);
}

// ---------------------------------------------------------------------------------------------
// List producer: k_adc_search_lists_u8 without (bias == null) and with RESIDUAL (bias != null) over packed rows, behind
// the same plan (seg_begin, seg_cum of k_adc_lists_plan); allow != null: its MASKED form, the mask in position order.
// With s the row sum, b the bias of the probe slot through which the row is reached, x = extra[row]:
//   bias == null:  IP = false: s                            IP = true: -fl(s * x)            (x = 1 when extra == null)
//   bias != null:  IP = false: fl(fl(b + x) - fl(s + s))    IP = true: -fl(fl(b + s) * x)    (IP: x = 1 when extra == null)
// lut [queries of the launch][M][K]; bias [queries of the launch][b_rs]; part_* [queries][G][64 L].
// ---------------------------------------------------------------------------------------------
template <bool IP, int NV, int L>
__global__ __launch_bounds__(1024) void k_adc_search_lists_p4(
    const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs, const uint32_t* __restrict__ allow /* or null */,
    const float* __restrict__ lut, const float* __restrict__ bias /* or null */, int64_t b_rs,
    const float* __restrict__ extra /* [n]: scales (IP) or row terms (bias, !IP), or null */, int M, int K, int kk,
    const int64_t* __restrict__ seg_begin, const int64_t* __restrict__ seg_cum, int n_probe, unsigned* __restrict__ part_k,
    uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    constexpr int NW = NV + 1;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    p4_stage_table(lds_s, lut + (size_t)blockIdx.y * M * K, M, K);
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + M * 16);    // [16][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[1];
    st[0].init();
    const int64_t* sb = seg_begin + (size_t)blockIdx.y * n_probe;
    const int64_t* sc = seg_cum + (size_t)blockIdx.y * ((size_t)n_probe + 1);
    const float* pb = bias ? bias + (int64_t)blockIdx.y * b_rs : nullptr;
    const ListsSlice slice = adc_lists_wg_slice(sc[n_probe]);
    const int64_t s0 = slice.s0, s1 = slice.s1;
    SegmentPos pos = adc_segment_start(sb, sc, pb, n_probe, s0, s1);
    const int PB = (M + 1) >> 1;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + PB);     // one past the last code byte
    const bool full = K == 16;
    const unsigned K4 = (unsigned)K * 4u;
    bool bad = false;
    for (int64_t base = s0; base < s1; base += 1024) {              // wave-uniform trip count: the selection is wave-wide
        const int64_t c = base + threadIdx.x;
        bool valid = c < s1;
        float v = 0.f;
        int64_t row = 0;
        if (valid) {
            pos = adc_segment_seek<false>(pos, c, sb, sc, pb, n_probe);
            row = c + pos.delta;
            valid = (uint64_t)row < (uint64_t)n;                    // holds by construction of the plan
        }
        if (allow && valid) valid = adc_mask_bit(allow, row);       // before the fetch: a disallowed row is not read
        if (valid) {
            float x = 1.f;
            if (IP ? extra != nullptr : pb != nullptr) x = extra[row];   // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, PB, w);
            const unsigned sh = (unsigned)(a & 3);
            const float s = full ? adc_row_sum_p4<NV, true>(w, sh, lds_s, M, K4, bad)
                                 : adc_row_sum_p4<NV, false>(w, sh, lds_s, M, K4, bad);
            if (pb) v = IP ? -fmul(fadd(pos.bias, s), x) : fsub(fadd(pos.bias, x), fadd(s, s));
            else v = IP ? -fmul(s, x) : s;
        }
        st[0].offer(v, (unsigned)row, valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L, true>(st, qk, qi, reinterpret_cast<unsigned*>(lds_s), 0, part_k, part_i);
}

// ---------------------------------------------------------------------------------------------
// Pack / unpack.  Both walk the aligned dwords that cover the output's byte span [out, out + (rows - 1) stride + len),
// one lane per dword, consecutive lanes consecutive dwords: a dword whose four bytes all belong to rows is one store,
// any other -- the span's two ends, and the dwords that touch the gap between rows when stride > len -- stores its row
// bytes singly and leaves the rest alone.
// ---------------------------------------------------------------------------------------------

// packed[i][j] = code(i, 2j) | code(i, 2j + 1) << 4 (0 past M); a code >= K packs as 0 and raises the flag
template <typename IdxT>
__global__ __launch_bounds__(256) void k_pack_codes4(const IdxT* __restrict__ codes, int64_t n, int64_t c_rs, int M, int K,
                                                     uint8_t* __restrict__ out, int64_t o_rs, int* __restrict__ err)
{
    const int PB = (M + 1) >> 1;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(out);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * o_rs + PB);
    const uintptr_t a0 = (lo & ~(uintptr_t)3) + 4 * ((uintptr_t)blockIdx.x * 256 + threadIdx.x);
    if (a0 >= hi) return;
    const uintptr_t first = a0 < lo ? lo : a0;
    int64_t row = (int64_t)((first - lo) / (uintptr_t)o_rs);
    int64_t j = (int64_t)(first - lo) - row * o_rs;
    unsigned v = 0, have = 0;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uintptr_t p = a0 + e;
        if (p < first || p >= hi) continue;
        if (j < PB) {
            const IdxT* cr = codes + row * c_rs + 2 * j;
            uint64_t c0 = (uint64_t)cr[0], c1 = 2 * j + 1 < M ? (uint64_t)cr[1] : 0;
            if (c0 >= (uint64_t)K) { bad = true; c0 = 0; }
            if (c1 >= (uint64_t)K) { bad = true; c1 = 0; }
            v |= (unsigned)(c0 | c1 << 4) << (8 * e);
            have |= 1u << e;
        }
        if (++j == o_rs) { j = 0; ++row; }
    }
    if (have == 0xfu) {
        *reinterpret_cast<unsigned*>(a0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (have >> e & 1u) *reinterpret_cast<uint8_t*>(a0 + e) = (uint8_t)(v >> (8 * e));
    }
    if (bad) atomicOr(err, 1);
}

// out[r][m] = nibble m of packed row (rows ? rows[r] : r), as it is; a row id outside [0, n) gives a zero row and raises
// the flag.  The pad nibble of an odd M is not emitted.  (Not a template: it belongs to one translation unit,
// pqhip_adc_packed4.hip; pqhip_adc_packed4_lists.hip defines PQHIP_PACKED4_PRODUCERS_ONLY.)
#ifndef PQHIP_PACKED4_PRODUCERS_ONLY
__global__ __launch_bounds__(256) void k_unpack_codes4(const uint8_t* __restrict__ packed, int64_t n, int64_t p_rs,
                                                       const int64_t* __restrict__ rows, int64_t n_out, int M,
                                                       uint8_t* __restrict__ out, int64_t o_rs, int* __restrict__ err)
{
    const uintptr_t lo = reinterpret_cast<uintptr_t>(out);
    const uintptr_t hi = lo + (uintptr_t)((n_out - 1) * o_rs + M);
    const uintptr_t a0 = (lo & ~(uintptr_t)3) + 4 * ((uintptr_t)blockIdx.x * 256 + threadIdx.x);
    if (a0 >= hi) return;
    const uintptr_t first = a0 < lo ? lo : a0;
    int64_t r = (int64_t)((first - lo) / (uintptr_t)o_rs);
    int64_t m = (int64_t)(first - lo) - r * o_rs;
    unsigned v = 0, have = 0;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uintptr_t p = a0 + e;
        if (p < first || p >= hi) continue;
        if (m < M) {
            const int64_t src = rows ? rows[r] : r;
            unsigned c = 0;
            if (src >= 0 && src < n) c = (packed[src * p_rs + (m >> 1)] >> (4 * (m & 1))) & 0xfu;
            else bad = true;
            v |= c << (8 * e);
            have |= 1u << e;
        }
        if (++m == o_rs) { m = 0; ++r; }
    }
    if (have == 0xfu) {
        *reinterpret_cast<unsigned*>(a0) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (have >> e & 1u) *reinterpret_cast<uint8_t*>(a0 + e) = (uint8_t)(v >> (8 * e));
    }
    if (bad) atomicOr(err, 1);
}
#endif  // PQHIP_PACKED4_PRODUCERS_ONLY

}  // namespace pqhip
