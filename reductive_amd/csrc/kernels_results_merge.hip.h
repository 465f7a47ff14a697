// kernels_results_merge.hip.h -- exact merge of the top-k results of several searches (include/pqhip.h:
// pqhip_topk_merge_f32_dev): P parts, each one sorted result row [k_in] per query, become one row [k] per query.
//
// Order.  An entry is (key, part << 10 | rank): key = adc_order_key of the value (of -value for scores), rank the entry's
// position in its part's row.  The 32-bit composite makes the order strict and never looks at a row id, so the merge is
// stable by part and the WaveList order (key, I) of kernels_adc_search.hip.h is the definition itself.  An absent entry
// (index < 0) becomes the list's empty entry (kSearchEmptyKey, all ones), which is above every present entry: a NaN has
// the same key but a composite below 2^26.
//
// One workgroup per query, one wave per part (at most kSearchMergeWaves waves; further parts go round).  A wave reads
// its part's row reversed against its list -- lanes read consecutive addresses -- keeps the pairwise minimum and
// bitonic-merges in registers, as WaveList::merge_sorted does from a stored list.  Only the first 64 L >= k entries of
// a part can reach the output, so L follows k alone.  The waves' lists are merged in a tree through LDS: in each round
// the upper half of the live waves stores, the lower half merges, so LDS holds waves / 2 lists of 64 L (key, composite)
// pairs -- 32 KB at L = 16.  The row id of a winner is fetched once, from its part and rank, and its part's offset added.
#pragma once
#include "kernels_adc_search.hip.h"

namespace pqhip {

constexpr int kTopkMergeRankBits = 10;       // rank < 1,024 = PQHIP_TOPK_MERGE_MAX_K
constexpr int kTopkMergeMaxParts = 65536;    // part << 10 | rank stays below 2^26: never the empty entry

// val / idx [P][nq][k_in] with part strides v_ps / i_ps and row strides v_rs / i_rs (elements), offsets [P] or null.
// waves = blockDim.x / 64 is a power of two <= kSearchMergeWaves; dynamic LDS: max(waves / 2, 1) * 64 L * 8 bytes.
// Queries are taken grid-stride: the result does not depend on the grid.
template <bool LARGEST, int L>
__global__ __launch_bounds__(64 * kSearchMergeWaves) void k_topk_merge(const float* __restrict__ val, int64_t v_ps, int64_t v_rs,
                                                                       const int64_t* __restrict__ idx, int64_t i_ps, int64_t i_rs,
                                                                       const int64_t* __restrict__ offsets, int P, int64_t nq,
                                                                       int k_in, int kk, float* __restrict__ out_val, int64_t ov_rs,
                                                                       int64_t* __restrict__ out_idx, int64_t oi_rs,
                                                                       int* __restrict__ out_part, int64_t op_rs)
{
    constexpr int LK = 64 * L;
    extern __shared__ __attribute__((aligned(16))) unsigned lds_t[];
    const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slots = waves > 1 ? waves / 2 : 1;
    unsigned* ck = lds_t;                    // [slots][LK] keys
    unsigned* ci = lds_t + slots * LK;       // [slots][LK] composites
    for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        WaveList<L, unsigned> lst;
        lst.clear();
        for (int p = wave; p < P; p += waves) {
            const float* vr = val + (int64_t)p * v_ps + q * v_rs;
            const int64_t* ir = idx + (int64_t)p * i_ps + q * i_rs;
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int e = (L - 1 - r) * 64 + 63 - lane;            // reversed: the pairwise minimum is bitonic
                if (e < k_in && ir[e] >= 0) {
                    const float v = vr[e];
                    const unsigned ok = adc_order_key(LARGEST ? -v : v);
                    const unsigned oi = ((unsigned)p << kTopkMergeRankBits) | (unsigned)e;
                    if (ent_less(ok, oi, lst.k[r], lst.i[r])) { lst.k[r] = ok; lst.i[r] = oi; }
                }
            }
            lst.bitonic_merge();
        }
        for (int h = waves >> 1; h >= 1; h >>= 1) {
            if (wave >= h && wave < 2 * h) lst.store(ck + (wave - h) * LK, ci + (wave - h) * LK);
            __syncthreads();
            if (wave < h) lst.merge_sorted(ck + wave * LK, ci + wave * LK);
            __syncthreads();                                           // the slots are rewritten in the next round
        }
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int e = r * 64 + lane;
                if (e < kk) {
                    const unsigned c = lst.i[r];
                    const bool pad = c == ~0u;
                    const int p = (int)(c >> kTopkMergeRankBits), rank = (int)(c & ((1u << kTopkMergeRankBits) - 1));
                    float v = __uint_as_float(LARGEST ? 0xff800000u : 0x7f800000u);
                    int64_t id = -1;
                    if (!pad) {
                        v = LARGEST ? adc_ip_key_score(lst.k[r]) : adc_key_value(lst.k[r]);
                        id = idx[(int64_t)p * i_ps + q * i_rs + rank] + (offsets ? offsets[p] : 0);
                    }
                    out_val[q * ov_rs + e] = v;
                    out_idx[q * oi_rs + e] = id;
                    if (out_part) out_part[q * op_rs + e] = pad ? -1 : p;
                }
            }
        }
    }
}

}  // namespace pqhip
