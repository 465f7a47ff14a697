// pqhip_lists_layout.hip -- building a partitioned index on the device (include/pqhip.h: pqhip_lists_layout_dev,
// pqhip_residuals_f32_dev, pqhip_residual_terms_f32_dev): the entry points, their checks, the grid choices and the
// launches of kernels_lists_layout.hip.h.  The count table of the layout lives in the codebook's scratch for the
// duration of the call.  Nothing else refers to this unit.
#include "pqhip_internal.h"

#include "kernels_lists_layout.hip.h"

using namespace pqhip;
using namespace pqh;

namespace pqh {

constexpr int64_t kLayoutSliceMax = (int64_t)1 << 31;        // rows of one workgroup: its counts are 32-bit words in LDS

template <typename T>
int32_t launch_layout(pqhip_codebook* cb, int slot, const T* assign, int64_t n, int n_lists, int64_t* list_off, int64_t* ids,
                      int64_t* positions, int64_t* lists, hipStream_t st)
{
    // one tile set (1,024 rows) per workgroup at least; by default as many workgroups per CU as keep their cursor tables
    // (4 bytes per list) within 64 KB of LDS, at most four
    const int64_t tile = (int64_t)kLayoutThreads * kLayoutUnroll;
    const int64_t forced = cb->ctx->opt.lists_layout_wgs.load(std::memory_order_relaxed);
    const int per_cu = n_lists <= 4096 ? 4 : n_lists <= 8192 ? 2 : 1;
    int64_t G = forced > 0 ? std::min<int64_t>(forced, 65536) : (int64_t)cb->ctx->devs[slot]->n_cus * per_cu;
    G = std::max<int64_t>(1, std::min<int64_t>(G, (n + tile - 1) / tile));
    G = std::max<int64_t>(G, (n + kLayoutSliceMax - 1) / kLayoutSliceMax);
    const int64_t per = (n + G - 1) / G;
    // scratch: valid [1] | bad [G] | totals [n_lists] | counts [G][n_lists]
    const int64_t words = 1 + G + n_lists + G * n_lists;
    if (words > kScratchBytesMax / (int64_t)sizeof(int64_t)) return PQHIP_EUNSUPPORTED;
    ErrFlag ef(cb, slot, st);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)words * sizeof(int64_t)));
    int64_t* valid = (int64_t*)lease.ptr();
    int64_t* bad = valid + 1;
    int64_t* totals = bad + G;
    int64_t* counts = totals + n_lists;
    const size_t lds = (size_t)n_lists * sizeof(unsigned);
    // (64 KB at 16,384 lists; the count kernel has a few static words beside it, so the limit asked for leaves room)
    HIPCHK(hipFuncSetAttribute((const void*)k_layout_count<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPCHK(hipFuncSetAttribute((const void*)k_layout_place<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    hipLaunchKernelGGL((k_layout_count<T>), dim3((unsigned)G), dim3(kLayoutThreads), lds, st, assign, n, per, n_lists, counts, bad,
                       ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_layout_count");
    hipLaunchKernelGGL(k_layout_columns, dim3((unsigned)((n_lists + 255) / 256)), dim3(256), 0, st, counts, (int)G, n_lists, totals);
    HIPCHK(hipGetLastError());
    note_kernel("k_layout_columns");
    hipLaunchKernelGGL(k_layout_offsets, dim3(1), dim3(1024), 0, st, totals, bad, (int)G, n_lists, n, valid, list_off, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_layout_offsets");
    int key_bits = 0;
    while (((int64_t)1 << key_bits) < n_lists) ++key_bits;
    hipLaunchKernelGGL((k_layout_place<T>), dim3((unsigned)G), dim3(kLayoutThreads), lds, st, assign, n, per, n_lists, key_bits, valid,
                       counts, list_off, ids, positions, lists);
    HIPCHK(hipGetLastError());
    note_kernel("k_layout_place");
    return PQHIP_OK;
}

}  // namespace pqh

extern "C" {

int32_t pqhip_lists_layout_dev(pqhip_codebook* cb, int32_t slot, const void* d_assign, int32_t idx_bytes, int64_t n,
                               int64_t n_lists, int64_t* d_list_off, int64_t* d_ids, int64_t* d_positions, int64_t* d_lists,
                               void* stream)
{
    if (!cb || n < 0 || n_lists < 1 || (idx_bytes != 4 && idx_bytes != 8) || !d_list_off) return PQHIP_EINVAL;
    if (n > 0 && (!d_assign || !d_ids || !d_positions)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (n_lists > PQHIP_LISTS_LAYOUT_MAX_LISTS || n > ((int64_t)1 << 49)) return PQHIP_EUNSUPPORTED;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_list_off, 0, (size_t)(n_lists + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    if (idx_bytes == 4)
        return launch_layout<int32_t>(cb, slot, (const int32_t*)d_assign, n, (int)n_lists, d_list_off, d_ids, d_positions, d_lists, st);
    return launch_layout<int64_t>(cb, slot, (const int64_t*)d_assign, n, (int)n_lists, d_list_off, d_ids, d_positions, d_lists, st);
}

int32_t pqhip_residuals_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_x, int64_t n, int64_t d, int64_t x_rs,
                                const int64_t* d_assign, const float* d_centroids, int64_t n_lists, float* d_out, int64_t o_rs,
                                void* stream)
{
    if (!cb || n < 0 || d < 1 || n_lists < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (d > PQHIP_RESIDUALS_MAX_D) return PQHIP_EUNSUPPORTED;
    if (n == 0) return PQHIP_OK;
    if (!d_x || !d_assign || !d_centroids || !d_out) return PQHIP_EINVAL;
    if (x_rs < d || o_rs < d) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const int64_t blocks = (n + kResidualRows - 1) / kResidualRows;
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)cb->ctx->devs[slot]->n_cus * 32));
    hipLaunchKernelGGL(k_residuals, dim3((unsigned)wgs), dim3(kResidualThreads), 0, st, d_x, x_rs, d_assign, d_centroids, n_lists, n,
                       (int)d, d_out, o_rs, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_residuals");
    return PQHIP_OK;
}

int32_t pqhip_residual_terms_f32_dev(pqhip_codebook* cb, int32_t slot, const uint8_t* d_codes, int64_t n, int64_t c_rs,
                                     const int64_t* d_assign, const float* d_centroids, int64_t n_lists, float* d_out,
                                     void* stream)
{
    if (!cb || n < 0 || n_lists < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->has_proj || cb->K > 256 || cb->M > PQHIP_RESIDUAL_TERMS_MAX_M || cb->d > PQHIP_RESIDUALS_MAX_D) return PQHIP_EUNSUPPORTED;
    if (n == 0) return PQHIP_OK;
    if (!d_codes || !d_assign || !d_centroids || !d_out) return PQHIP_EINVAL;
    if (c_rs < cb->M) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const int M = (int)cb->M;
    const int rows_per_wg = std::max(1, std::min(kTermsThreads, 4096 / M));        // at most 32 KB of partial sums
    const int64_t blocks = (n + rows_per_wg - 1) / rows_per_wg;
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)cb->ctx->devs[slot]->n_cus * 16));
    HIPCHK(hipFuncSetAttribute((const void*)k_residual_terms, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    hipLaunchKernelGGL(k_residual_terms, dim3((unsigned)wgs), dim3(kTermsThreads), (size_t)rows_per_wg * M * sizeof(double), st,
                       cb->dev[slot].cb, M, (int)cb->K, (int)cb->dsub, d_codes, c_rs, d_assign, d_centroids, n_lists, n, rows_per_wg,
                       d_out, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_residual_terms");
    return PQHIP_OK;
}

}  // extern "C"
