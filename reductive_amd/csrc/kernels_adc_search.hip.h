// kernels_adc_search.hip.h -- ADC search: the table-sum scan of kernels_adc.hip.h fused with an exact top-k selection,
// so that a search returns the k nearest rows of every query without writing the n_codes distances.
// (pqhip_adc.hip instantiates the kernels without a row mask and the merge, pqhip_adc_masked.hip those with one.)
//
// Order.  A row is the pair (key(dist), row index) and rows compare lexicographically: key() is the first-minimum order
// of cluster_assignments (kmeans.rs:133-159, oracle of_less) -- -0 == +0, every NaN equal to every other and above
// +Inf -- and a tie in distance goes to the smaller index.  The order is strict (indices differ), so the k smallest
// rows are one set whatever grid, row ranges or merge order produced them: the result does not depend on them.
//
// Producer (per wave, per query): the row's distance comes from the scan's own row sum (adc_fetch_row + adc_row_sum /
// adc_row_sum_mq, the same sequential f32 chain over m) and is compared with a wave-uniform threshold, the k-th entry of
// the wave's sorted list.  Rows below it are queued in LDS (kSearchQueue entries per wave and query); a full queue is
// merged into the list: the 64 candidates are sorted across the lanes (bitonic, __shfl_xor), reversed against the
// list's last 64 entries (pairwise min: the result is bitonic) and the list is bitonic-merged in registers -- entry
// e = r * 64 + lane lives in register r of lane `lane`, strides >= 64 are register pairs, smaller ones lane swaps.
// A list holds 64 L >= k entries; its first k are exact for the rows the wave has seen, the rest are real rows and do
// no harm.  After the row loop the 16 waves' lists are merged in a tree through LDS (the table image is dead by then)
// and the workgroup writes one sorted list per query to scratch.  k_adc_search_merge merges the workgroups' lists of
// one query and writes the first k entries (index -1 and +Inf past the last row).
// The similarity search (the IP flag of every kernel) offers the key of -score to the same selection.
#pragma once
#include "adc_key.hip.h"
#include "kernels_adc.hip.h"

namespace pqhip {

constexpr int kSearchMaxK = 1024;
constexpr int kSearchQueue = 32;             // queued candidates per (wave, query)
constexpr int kSearchWaves = 16;             // producer workgroups: 1,024 threads
constexpr int kSearchMergeWaves = 8;         // k_adc_search_merge: 512 threads
constexpr unsigned kSearchEmptyKey = 0xffffffffu;

// adc_order_key, adc_key_value and adc_ip_key_score: adc_key.hip.h (shared with the re-ranking kernels)

template <typename I>
__device__ __forceinline__ bool ent_less(unsigned ka, I ia, unsigned kb, I ib)
{
    return ka < kb || (ka == kb && ia < ib);
}

// compare-exchange with the lane at xor distance d: this lane keeps the smaller entry when keep_min, else the larger
template <typename I>
__device__ __forceinline__ void cmpx_lanes(unsigned& k, I& i, int d, bool keep_min)
{
    const unsigned ok = __shfl_xor(k, d);
    const I oi = __shfl_xor(i, d);
    const bool take = keep_min ? ent_less(ok, oi, k, i) : ent_less(k, i, ok, oi);
    if (take) { k = ok; i = oi; }
}

// bitonic sort of one entry per lane, ascending over the 64 lanes
template <typename I>
__device__ __forceinline__ void wave_sort64(unsigned& k, I& i)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int d = size >> 1; d > 0; d >>= 1) cmpx_lanes(k, i, d, ((lane & d) == 0) == ((lane & size) == 0));
    }
}

// A wave's sorted list of 64 L entries (row key, index); entry e = r * 64 + lane is k[r], i[r] of lane `lane`.
// Empty entries are (kSearchEmptyKey, all ones): above every row, NaN rows included.
template <int L, typename I>
struct WaveList {
    unsigned k[L];
    I i[L];

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int r = 0; r < L; ++r) { k[r] = kSearchEmptyKey; i[r] = ~(I)0; }
    }
    // sorts a bitonic sequence ascending
    __device__ __forceinline__ void bitonic_merge()
    {
#pragma unroll
        for (int dr = L / 2; dr >= 1; dr >>= 1) {
#pragma unroll
            for (int r = 0; r < L; ++r) {
                if (!(r & dr) && ent_less(k[r + dr], i[r + dr], k[r], i[r])) {
                    const unsigned tk = k[r]; k[r] = k[r + dr]; k[r + dr] = tk;
                    const I ti = i[r]; i[r] = i[r + dr]; i[r + dr] = ti;
                }
            }
        }
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
            for (int r = 0; r < L; ++r) cmpx_lanes(k[r], i[r], d, (lane & d) == 0);
        }
    }
    // keep the 64 L smallest of the list and 64 candidates, one per lane, in any order
    __device__ __forceinline__ void merge64(unsigned ck, I ci)
    {
        const int lane = threadIdx.x & 63;
        wave_sort64(ck, ci);
        const unsigned rk = __shfl(ck, 63 - lane);
        const I ri = __shfl(ci, 63 - lane);
        if (ent_less(rk, ri, k[L - 1], i[L - 1])) { k[L - 1] = rk; i[L - 1] = ri; }
        bitonic_merge();
    }
    // keep the 64 L smallest of the list and another sorted list of 64 L entries at bk / bi (LDS or global)
    __device__ __forceinline__ void merge_sorted(const unsigned* bk, const I* bi)
    {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int r = 0; r < L; ++r) {
            const int e = (L - 1 - r) * 64 + 63 - lane;
            const unsigned ok = bk[e];
            const I oi = bi[e];
            if (ent_less(ok, oi, k[r], i[r])) { k[r] = ok; i[r] = oi; }
        }
        bitonic_merge();
    }
    __device__ __forceinline__ void store(unsigned* bk, I* bi) const
    {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int r = 0; r < L; ++r) { bk[r * 64 + lane] = k[r]; bi[r * 64 + lane] = i[r]; }
    }
};

// Per (wave, query) producer state: the list, its k-th entry (the threshold, wave-uniform) and the LDS queue.
template <int L>
struct SearchState {
    WaveList<L, unsigned> lst;
    unsigned tk, ti;     // k-th entry of lst: a row enters only below it
    int cnt;             // queued entries

    __device__ __forceinline__ void init()
    {
        lst.clear();
        tk = kSearchEmptyKey;
        ti = kSearchEmptyKey;
        cnt = 0;
    }
    __device__ __forceinline__ void update_threshold(int kk)
    {
        const int rk = (kk - 1) >> 6, ln = (kk - 1) & 63;
#pragma unroll
        for (int r = 0; r < L; ++r) {
            if (r == rk) {
                tk = (unsigned)__builtin_amdgcn_readlane((int)lst.k[r], ln);
                ti = (unsigned)__builtin_amdgcn_readlane((int)lst.i[r], ln);
            }
        }
    }
    // merge the queue's entries into the list
    __device__ __forceinline__ void flush(const unsigned* qk, const unsigned* qi)
    {
        const int lane = threadIdx.x & 63;
        __builtin_amdgcn_wave_barrier();
        const unsigned ck = lane < cnt ? qk[lane] : kSearchEmptyKey;
        const unsigned ci = lane < cnt ? qi[lane] : kSearchEmptyKey;
        __builtin_amdgcn_wave_barrier();
        lst.merge64(ck, ci);
        cnt = 0;
    }
    // one row per lane (`valid` lanes only); `off` is the row's index within the workgroup's range
    __device__ __forceinline__ void offer(float dist, unsigned off, bool valid, unsigned* qk, unsigned* qi, int kk)
    {
        const unsigned key = adc_order_key(dist);
        const bool pass = valid && ent_less(key, off, tk, ti);
        const unsigned long long b = __ballot(pass);
        if (b == 0) return;
        const int pc = __popcll(b);
        if (cnt + pc > kSearchQueue) {
            if (cnt) flush(qk, qi);
            if (pc > kSearchQueue) lst.merge64(pass ? key : kSearchEmptyKey, pass ? off : kSearchEmptyKey);
            update_threshold(kk);
            if (pc > kSearchQueue) return;
        }
        const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        __builtin_amdgcn_wave_barrier();
        if (pass) { qk[pos] = key; qi[pos] = off; }
        __builtin_amdgcn_wave_barrier();
        cnt += pc;
    }
};

// After the row loop: flush the queues, merge the 16 waves' lists per query through LDS (`comb`: the whole dynamic LDS,
// at least 16 NQ 64 L 8 bytes; the caller has synchronised the workgroup away from the table image) and write the
// workgroup's list of query q to part_*[(q * gridDim.x + blockIdx.x) * 64 L ..] with indices made global.
// QUERY_Y (NQ = 1): the grid is (workgroups of a query, queries) and the query of the list slot is blockIdx.y
// (kernels_adc_search_lists.hip.h); the slot is formed where it is used, so the other producers compile as before.
template <int NQ, int L, bool QUERY_Y = false>
__device__ __forceinline__ void search_finish(SearchState<L> (&st)[NQ], unsigned* qk, unsigned* qi, unsigned* comb,
                                              int64_t row_begin, unsigned* __restrict__ part_k, uint64_t* __restrict__ part_i)
{
    static_assert(!QUERY_Y || NQ == 1, "one query per workgroup when the query comes from the grid");
    constexpr int LK = 64 * L;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (st[q].cnt) st[q].flush(qk + (wave * NQ + q) * kSearchQueue, qi + (wave * NQ + q) * kSearchQueue);
    __syncthreads();                                           // queues and table image are dead from here
    unsigned* ck = comb;                                       // [16][NQ][LK] keys
    unsigned* ci = comb + kSearchWaves * NQ * LK;              // [16][NQ][LK] indices
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].lst.store(ck + (wave * NQ + q) * LK, ci + (wave * NQ + q) * LK);
    __syncthreads();
    for (int h = kSearchWaves / 2; h >= 1; h >>= 1) {
        if (wave < h) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                st[q].lst.merge_sorted(ck + ((wave + h) * NQ + q) * LK, ci + ((wave + h) * NQ + q) * LK);
                st[q].lst.store(ck + (wave * NQ + q) * LK, ci + (wave * NQ + q) * LK);
            }
        }
        __syncthreads();
    }
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const size_t base = ((size_t)(QUERY_Y ? blockIdx.y : q) * gridDim.x + blockIdx.x) * LK;
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const unsigned off = st[q].lst.i[r];
                part_k[base + r * 64 + lane] = st[q].lst.k[r];
                part_i[base + r * 64 + lane] = off == kSearchEmptyKey ? ~0ull : (uint64_t)(row_begin + off);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// u8 codes, tables in LDS: NQ = 1 ([M][K] image, the single-query scan's row sum) or NQ = 4 / 8 (the multi-query
// scan's interleaved [NQ/4][M][K][4] image and row sum).  One 1,024-thread workgroup per CU over a contiguous row range
// of rows_per_wg < 2^31 rows; NV = the code dwords fetched per row (>= ceil(M / 4)).  LDS: the table image, then the
// queues [16][NQ][kSearchQueue] keys and indices; later the combine lists.
//
// One body serves the four exhaustive searches; a flag that is off leaves no instruction and no argument load behind.
// IP (pqhip_adc_ip_search_f32_dev): the value offered to the unchanged SearchState is -fl(s * scale), s the row sum over
// inner-product tables and scale = scales[i] (1 without scales: exact), loaded once per row for all NQ queries; negation
// is exact, so the smallest key is the largest score.  Without IP `scales` is not looked at.
// MASKED (pqhip_adc_masked.hip instantiates these): the row's bit of `allow` (adc_mask_bit) is one more term of the
// `valid` that offer() takes, formed before the fetch -- a row whose bit is clear loads no code and no scale and cannot
// raise the range flag.  Row ranges start on multiples of 1,024, so a wave reads two mask words per trip; the trip
// count does not depend on the mask (offer is wave-wide).  Without MASKED `allow` is not looked at.
// ---------------------------------------------------------------------------------------------
template <bool IP, bool MASKED, int NV, int NQ, int L>
__global__ __launch_bounds__(1024) void k_adc_search_u8(const uint8_t* __restrict__ codes, int64_t n, int64_t c_rs,
                                                        const uint32_t* __restrict__ allow /* MASKED */,
                                                        const float* __restrict__ lut /* [NQ][M][K] */,
                                                        const float* __restrict__ scales /* IP: [n] or null */, int M, int K,
                                                        int kk, int64_t rows_per_wg, unsigned* __restrict__ part_k,
                                                        uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    static_assert(NQ == 1 || NQ == 4 || NQ == 8, "queries per pass");
    constexpr int NW = NV + 1, NH = NQ / 4;
    extern __shared__ __attribute__((aligned(16))) float lds_s[];
    const int MK = M * K;
    adc_stage_tables<NQ>(lds_s, lut, MK);
    unsigned* qk = reinterpret_cast<unsigned*>(lds_s + NQ * MK);   // [16][NQ][kSearchQueue]
    unsigned* qi = qk + kSearchWaves * NQ * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) st[q].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(codes);
    const uintptr_t hi = lo + (uintptr_t)((n - 1) * c_rs + M);      // one past the last code byte
    bool bad = false;
    for (int64_t base = row_begin; base < row_end; base += 1024) {  // wave-uniform trip count: the selection is wave-wide
        const int64_t row = base + threadIdx.x;
        bool valid = row < row_end;
        if constexpr (MASKED) {
            if (valid) valid = adc_mask_bit(allow, row);            // before the fetch: a disallowed row is not read
        }
        float val[NQ];                                              // distance, or -score
#pragma unroll
        for (int q = 0; q < NQ; ++q) val[q] = 0.f;
        if (valid) {
            float sc = 1.f;
            if constexpr (IP) sc = scales ? scales[row] : 1.f;      // issued with the row's code words
            const uintptr_t a = lo + (uintptr_t)(row * c_rs);
            unsigned w[NW];
            adc_fetch_row<NW>(a, lo, hi, M, w);
            const unsigned sh = (unsigned)(a & 3);
            if constexpr (NQ == 1) {
                val[0] = adc_row_sum<NV>(w, sh, lds_s, M, K, bad);
            } else {
                f32x2 s[NH][2];
#pragma unroll
                for (int hq = 0; hq < NH; ++hq) { s[hq][0] = (f32x2){0.f, 0.f}; s[hq][1] = (f32x2){0.f, 0.f}; }
                adc_row_sum_mq<NV, NH>(w, sh, lds_s, M, K, MK, bad, s);
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

// Any code width, any table: one query, the table in LDS when TAB_LDS (k_adc_scan_wide's condition) else read through
// L2 as in k_adc_scan_any; the sum is theirs (sequential over m from +0).  Same selection, and IP as above.  No
// throughput claim.
template <bool IP, typename IdxT, int L, bool TAB_LDS>
__global__ __launch_bounds__(1024) void k_adc_search_any(const IdxT* __restrict__ codes, int64_t n, int64_t c_rs,
                                                         const float* __restrict__ lut,
                                                         const float* __restrict__ scales /* IP: [n] or null */, int M, int K,
                                                         int kk, int64_t rows_per_wg, unsigned* __restrict__ part_k,
                                                         uint64_t* __restrict__ part_i, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) float lds_a[];
    const int MK = M * K;
    const float* tab = lut;
    unsigned* qk = reinterpret_cast<unsigned*>(lds_a);
    if (TAB_LDS) {
        adc_stage_tables<1>(lds_a, lut, MK);
        tab = lds_a;
        qk = reinterpret_cast<unsigned*>(lds_a + MK);
    }
    unsigned* qi = qk + kSearchWaves * kSearchQueue;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SearchState<L> st[1];
    st[0].init();
    const int64_t row_begin = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row_end = row_begin + rows_per_wg;
    if (row_end > n) row_end = n;
    bool bad = false;
    for (int64_t base = row_begin; base < row_end; base += 1024) {
        const int64_t row = base + threadIdx.x;
        const bool valid = row < row_end;
        float s = 0.f;
        if (valid) {
            const IdxT* cr = codes + row * c_rs;
            for (int m = 0; m < M; ++m) {
                uint64_t c = (uint64_t)cr[m];
                if (c >= (uint64_t)K) { bad = true; c = 0; }
                s = fadd(s, tab[(int64_t)m * K + (int64_t)c]);
            }
            if constexpr (IP) s = -fmul(s, scales ? scales[row] : 1.f);
        }
        st[0].offer(s, (unsigned)(row - row_begin), valid, qk + wave * kSearchQueue, qi + wave * kSearchQueue, kk);
    }
    if (bad) atomicOr(err, 1);
    search_finish<1, L>(st, qk, qi, reinterpret_cast<unsigned*>(lds_a), row_begin, part_k, part_i);
}

// One workgroup per query: merges the n_lists workgroup lists of query blockIdx.x (sorted, 64 L entries each, global
// indices) and writes the first kk entries: distances, or (IP) the scores that the keys of -score stand for; past the
// last row, index -1 and +Inf resp. -Inf.  n_lists = 0 writes the padding only.
// LDS: 8 lists of 64 L keys + 64 L indices (12 KB L).
template <bool IP, int L>
__global__ __launch_bounds__(512) void k_adc_search_merge(const unsigned* __restrict__ part_k, const uint64_t* __restrict__ part_i,
                                                          int n_lists, int kk, float* __restrict__ val, int64_t v_rs,
                                                          int64_t* __restrict__ idx, int64_t i_rs)
{
    constexpr int LK = 64 * L;
    extern __shared__ __attribute__((aligned(16))) unsigned lds_m[];
    unsigned* ck = lds_m;                                                    // [8][LK]
    uint64_t* ci = reinterpret_cast<uint64_t*>(lds_m + kSearchMergeWaves * LK);   // [8][LK]
    const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    WaveList<L, uint64_t> lst;
    lst.clear();
    for (int g = wave; g < n_lists; g += kSearchMergeWaves) {
        const size_t base = ((size_t)q * n_lists + g) * LK;
        lst.merge_sorted(part_k + base, part_i + base);
    }
    lst.store(ck + wave * LK, ci + wave * LK);
    __syncthreads();
    for (int h = kSearchMergeWaves / 2; h >= 1; h >>= 1) {
        if (wave < h) {
            lst.merge_sorted(ck + (wave + h) * LK, ci + (wave + h) * LK);
            lst.store(ck + wave * LK, ci + wave * LK);
        }
        __syncthreads();
    }
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < L; ++r) {
            const int e = r * 64 + lane;
            if (e < kk) {
                const bool pad = lst.i[r] == ~0ull;
                const float v = IP ? adc_ip_key_score(lst.k[r]) : adc_key_value(lst.k[r]);
                val[(int64_t)q * v_rs + e] = pad ? __uint_as_float(IP ? 0xff800000u : 0x7f800000u) : v;
                idx[(int64_t)q * i_rs + e] = pad ? (int64_t)-1 : (int64_t)lst.i[r];
            }
        }
    }
}

}  // namespace pqhip
