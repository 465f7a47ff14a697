// pqhip_rerank.hip -- exact re-ranking of search candidates against resident vectors (include/pqhip.h:
// pqhip_rerank_f32_dev): argument checks, the grid of the distance stage, the entries in the codebook's scratch.
#include "pqhip_internal.h"

#include "kernels_rerank.hip.h"

using namespace pqhip;

namespace pqh {

constexpr size_t kRerankScratchBytes = 64u << 20;   // entries of one chunk of queries

// Workgroups that share one query in the distance stage: enough that every wave has one group of candidates, and no
// more than eight workgroups per CU over all queries of the launch (the waves of a CU then cover its 32 wave slots).
inline int64_t rerank_wgs_per_query(int64_t n_cand, int64_t nq, int n_cus)
{
    const int64_t by_work = (n_cand + kRerankWaves * kRerankGroup - 1) / (kRerankWaves * kRerankGroup);
    const int64_t by_cus = std::max<int64_t>(1, (int64_t)n_cus * 8 / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min(by_work, by_cus));
}

template <typename T, bool IP>
void launch_rerank_dist(unsigned G, unsigned nq, const float* q, int64_t q_rs, const void* x, int64_t n_rows, int d, int64_t x_rs,
                        const int64_t* cand, int n_cand, int64_t c_rs, uint64_t* pairs, int* err, hipStream_t st)
{
    hipLaunchKernelGGL((k_rerank_dist<T, IP>), dim3(G, nq), dim3(64 * kRerankWaves), (size_t)d * sizeof(float), st, q, q_rs,
                       (const T*)x, n_rows, d, x_rs, cand, n_cand, c_rs, pairs, err);
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_rerank_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                             int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const int64_t* d_cand, int32_t n_cand,
                             int64_t c_rs, int32_t metric, int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs,
                             void* stream)
{
    if (!cb || nq < 0 || n_rows < 0 || k < 1 || n_cand < 1 || d < 1 || (metric != 0 && metric != 1)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (vec_bytes != 2 && vec_bytes != 4) return PQHIP_EUNSUPPORTED;
    if (k > kRerankMaxK || n_cand > kRerankMaxCand || d > kRerankMaxD) return PQHIP_EUNSUPPORTED;
    if (n_rows > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;      // an entry keeps the row id in 32 bits
    if (nq == 0) return PQHIP_OK;
    if (!d_q || !d_cand || !d_val || !d_idx || (n_rows > 0 && !d_x)) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d) || c_rs < n_cand || v_rs < k || i_rs < k) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const int64_t chunk = std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kRerankScratchBytes / ((size_t)n_cand * sizeof(uint64_t)))});
    const int64_t forced = cb->ctx->opt.rerank_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 1024) : rerank_wgs_per_query(n_cand, chunk, cb->ctx->devs[slot]->n_cus);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * n_cand * sizeof(uint64_t)));
    uint64_t* pairs = (uint64_t*)lease.ptr();
    int n_pow2 = 1;
    while (n_pow2 < n_cand) n_pow2 <<= 1;
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        const float* qp = d_q + q * q_rs;
        const int64_t* cp = d_cand + q * c_rs;
        if (vec_bytes == 4) {
            if (metric) launch_rerank_dist<float, true>((unsigned)G, nqc, qp, q_rs, d_x, n_rows, (int)d, x_rs, cp, n_cand, c_rs, pairs, ef.flag, st);
            else launch_rerank_dist<float, false>((unsigned)G, nqc, qp, q_rs, d_x, n_rows, (int)d, x_rs, cp, n_cand, c_rs, pairs, ef.flag, st);
        } else {
            if (metric) launch_rerank_dist<_Float16, true>((unsigned)G, nqc, qp, q_rs, d_x, n_rows, (int)d, x_rs, cp, n_cand, c_rs, pairs, ef.flag, st);
            else launch_rerank_dist<_Float16, false>((unsigned)G, nqc, qp, q_rs, d_x, n_rows, (int)d, x_rs, cp, n_cand, c_rs, pairs, ef.flag, st);
        }
        HIPCHK(hipGetLastError());
        note_kernel("k_rerank_dist");
        if (metric)
            hipLaunchKernelGGL((k_rerank_select<true>), dim3(nqc), dim3(kRerankSelectThreads), 0, st, pairs, (int)n_cand, n_pow2, (int)k,
                               d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs);
        else
            hipLaunchKernelGGL((k_rerank_select<false>), dim3(nqc), dim3(kRerankSelectThreads), 0, st, pairs, (int)n_cand, n_pow2, (int)k,
                               d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs);
        HIPCHK(hipGetLastError());
        note_kernel("k_rerank_select");
    }
    return PQHIP_OK;
}

}  // extern "C"
