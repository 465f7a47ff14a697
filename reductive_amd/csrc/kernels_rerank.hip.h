// kernels_rerank.hip.h -- exact re-ranking of search candidates against resident vectors (pqhip_rerank_f32_dev): the
// stage after an ADC search that replaces the quantizer's estimate by the distance (or inner product) to the stored
// vector itself.  Per query: a gather of n_cand rows of d elements, a fixed-order f32 reduction per row, an exact top-k.
// (The kernels are instantiated in one translation unit, pqhip_rerank.hip; kernels_flat_search.hip.h takes rerank_elem
// and rerank_step, the row value's element and chain step, so that both calls share one definition of the value.)
//
// Value of a row (include/pqhip.h has the definition): lane l of a wave owns the chain over j = l, l + 64, l + 128, ..
// -- one coalesced 256-byte load per 64 f32 elements (128 bytes for f16) -- and the 64 partials are reduced by the fixed
// tree p_l += p_(l+s), s = 32 .. 1.  Nothing in it depends on the grid: every candidate is reduced by one whole wave.
//
// k_rerank_dist: grid (G, queries), 4 waves per workgroup.  The query is staged in LDS once per workgroup; wave w of
// workgroup g takes the candidates (g * 4 + w) * 4 + {0 .. 3}, then strides by 16 G: four rows, two 64-element steps
// each, are loaded before the first is used, so eight loads per lane are in flight.  Lane 0 writes the 64-bit entry
// (key << 32 | row id) of the candidate to scratch [queries][n_cand]; a skipped candidate (-1, or out of range, which
// also raises the flag) writes all ones, which sorts after every row (row ids stay below 2^32 - 2).
// k_rerank_select: one 512-thread workgroup per query sorts the entries (bitonic, padded to a power of two <= 1,024,
// 8 KB of LDS) and writes the first k.  Entries are whole (key, row id) pairs under a strict order, so the result does
// not depend on G; an id named twice gives two equal entries.
#pragma once
#include "adc_key.hip.h"

namespace pqhip {

constexpr int kRerankMaxK = 1024;
constexpr int kRerankMaxCand = 1024;
constexpr int kRerankMaxD = 16384;           // the query image: 64 KB of LDS
constexpr int kRerankWaves = 4;              // k_rerank_dist: 256 threads
constexpr int kRerankGroup = 4;              // candidates a wave reduces side by side
constexpr int kRerankSelectThreads = 512;
constexpr uint64_t kRerankSkipped = ~0ull;

__device__ __forceinline__ float rerank_elem(const float* p) { return *p; }
__device__ __forceinline__ float rerank_elem(const _Float16* p) { return (float)*p; }   // exact

template <bool IP>
__device__ __forceinline__ float rerank_step(float p, float q, float x)
{
    if constexpr (IP) {
        return fadd(p, fmul(q, x));
    } else {
        const float t = fsub(q, x);
        return fadd(p, fmul(t, t));
    }
}

template <typename T, bool IP>
__global__ __launch_bounds__(64 * kRerankWaves) void k_rerank_dist(const float* __restrict__ queries, int64_t q_rs,
                                                                  const T* __restrict__ x, int64_t n_rows, int d, int64_t x_rs,
                                                                  const int64_t* __restrict__ cand, int n_cand, int64_t c_rs,
                                                                  uint64_t* __restrict__ pairs, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) float lds_q[];
    const int q = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* qrow = queries + (int64_t)q * q_rs;
    for (int j = threadIdx.x; j < d; j += 64 * kRerankWaves) lds_q[j] = qrow[j];
    __syncthreads();
    const int64_t* crow = cand + (int64_t)q * c_rs;
    uint64_t* prow = pairs + (size_t)q * n_cand;
    const int n_full = d >> 6, tail = d & 63;
    bool bad = false;
    for (int c0 = (blockIdx.x * kRerankWaves + wave) * kRerankGroup; c0 < n_cand; c0 += gridDim.x * kRerankWaves * kRerankGroup) {
        int64_t id[kRerankGroup];
        bool ok[kRerankGroup];
        const T* xr[kRerankGroup];
        float p[kRerankGroup];
#pragma unroll
        for (int u = 0; u < kRerankGroup; ++u) {
            id[u] = c0 + u < n_cand ? crow[c0 + u] : (int64_t)-1;
            ok[u] = id[u] >= 0 && id[u] < n_rows;
            if (!ok[u] && id[u] != -1) bad = true;
            // A skipped candidate reads the first d elements of the query's own row instead (always readable; the sum
            // is dropped): the loads below stay free of branches and no byte outside the vectors is touched for it.
            xr[u] = ok[u] ? x + id[u] * x_rs : reinterpret_cast<const T*>(qrow);
            p[u] = 0.f;
        }
        int i = 0;
        for (; i + 2 <= n_full; i += 2) {
            float xv[kRerankGroup][2];
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) {
                xv[u][0] = rerank_elem(xr[u] + i * 64 + lane);
                xv[u][1] = rerank_elem(xr[u] + i * 64 + 64 + lane);
            }
            const float q0 = lds_q[i * 64 + lane], q1 = lds_q[i * 64 + 64 + lane];
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) p[u] = rerank_step<IP>(rerank_step<IP>(p[u], q0, xv[u][0]), q1, xv[u][1]);
        }
        if (i < n_full) {
            const float q0 = lds_q[i * 64 + lane];
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) p[u] = rerank_step<IP>(p[u], q0, rerank_elem(xr[u] + i * 64 + lane));
        }
        if (lane < tail) {
            const float q0 = lds_q[n_full * 64 + lane];
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) p[u] = rerank_step<IP>(p[u], q0, rerank_elem(xr[u] + n_full * 64 + lane));
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) p[u] = fadd(p[u], __shfl_down(p[u], s));   // lanes < s: p_l + p_(l+s)
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < kRerankGroup; ++u) {
                if (c0 + u < n_cand) {
                    const unsigned key = adc_order_key(IP ? -p[u] : p[u]);
                    prow[c0 + u] = ok[u] ? ((uint64_t)key << 32 | (uint64_t)(uint32_t)id[u]) : kRerankSkipped;
                }
            }
        }
    }
    if (bad && lane == 0) atomicOr(err, 1);
}

// n_pow2: the power of two >= n_cand (<= 1,024); n_cand = 0 writes the padding only (pairs is not read)
template <bool IP>
__global__ __launch_bounds__(kRerankSelectThreads) void k_rerank_select(const uint64_t* __restrict__ pairs, int n_cand, int n_pow2,
                                                                        int kk, float* __restrict__ val, int64_t v_rs,
                                                                        int64_t* __restrict__ idx, int64_t i_rs)
{
    __shared__ uint64_t ent[kRerankMaxCand];
    const int q = blockIdx.x;
    for (int e = threadIdx.x; e < n_pow2; e += kRerankSelectThreads)
        ent[e] = e < n_cand ? pairs[(size_t)q * n_cand + e] : kRerankSkipped;
    __syncthreads();
    for (int size = 2; size <= n_pow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n_pow2 >> 1); t += kRerankSelectThreads) {
                const int a = 2 * t - (t & (stride - 1)), b = a + stride;
                const uint64_t ea = ent[a], eb = ent[b];
                if ((ea > eb) == ((a & size) == 0)) { ent[a] = eb; ent[b] = ea; }
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < kk; e += kRerankSelectThreads) {
        const uint64_t v = e < n_pow2 ? ent[e] : kRerankSkipped;
        const bool pad = v == kRerankSkipped;
        const unsigned key = (unsigned)(v >> 32);
        val[(int64_t)q * v_rs + e] = pad ? __uint_as_float(IP ? 0xff800000u : 0x7f800000u) : (IP ? adc_ip_key_score(key) : adc_key_value(key));
        idx[(int64_t)q * i_rs + e] = pad ? (int64_t)-1 : (int64_t)(v & 0xffffffffull);
    }
}

}  // namespace pqhip
