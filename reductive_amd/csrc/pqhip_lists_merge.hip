// pqhip_lists_merge.hip -- merge of two list-ordered row arrays on the device (include/pqhip.h: pqhip_lists_merge_dev):
// the primitive under growing a partitioned matrix.  This unit holds the entry point, its checks, the grid choice and
// the two launches of kernels_lists_merge.hip.h; the segment table lives in the codebook's scratch for the duration of
// the call.  Nothing else refers to this unit.
#include "pqhip_internal.h"

#include "kernels_lists_merge.hip.h"

using namespace pqhip;
using namespace pqh;

extern "C" {

int32_t pqhip_lists_merge_dev(pqhip_codebook* cb, int32_t slot, const int64_t* d_off_a, int64_t n_a, const int64_t* d_off_b,
                              int64_t n_b, int64_t n_lists, int64_t row_bytes, const void* d_a, const void* d_b, void* d_out,
                              int64_t* d_off_out, void* stream)
{
    if (!cb || n_a < 0 || n_b < 0 || n_lists < 0 || row_bytes < 1) return PQHIP_EINVAL;
    const bool rows = n_a > 0 || n_b > 0;
    if (n_lists == 0 && rows) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (row_bytes > PQHIP_LISTS_MERGE_MAX_ROW_BYTES || n_lists > PQHIP_LISTS_MERGE_MAX_LISTS) return PQHIP_EUNSUPPORTED;
    constexpr int64_t kMaxRows = (int64_t)1 << 49;                  // (n_a + n_b) row_bytes stays below 2^62
    if (n_a > kMaxRows || n_b > kMaxRows) return PQHIP_EUNSUPPORTED;
    if (rows && (!d_off_a || !d_off_b || !d_out || (n_a > 0 && !d_a) || (n_b > 0 && !d_b))) return PQHIP_EINVAL;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (!rows) {
        if (d_off_out) HIPCHK(hipMemsetAsync(d_off_out, 0, (size_t)(n_lists + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    ErrFlag ef(cb, slot, st);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)(4 * n_lists + 2) * sizeof(int64_t)));
    int64_t* table = (int64_t*)lease.ptr();
    hipLaunchKernelGGL(k_lists_merge_plan, dim3(1), dim3(1024), 0, st, d_off_a, n_a, d_off_b, n_b, n_lists, table, d_off_out,
                       ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_lists_merge_plan");
    // 16-byte chunks of the destination (one more when the chunk grid cuts the first and the last byte off); by default
    // eight 256-thread workgroups per CU -- the 32 waves a CU holds -- and never fewer than one pass of chunks each
    const int64_t total = (n_a + n_b) * row_bytes;
    const int64_t n_chunks = (total + 15) / 16 + 1;
    const int64_t pass = (int64_t)kMergeThreads * kMergeUnroll;
    const int64_t forced = cb->ctx->opt.lists_merge_wgs.load(std::memory_order_relaxed);
    int64_t wgs = forced > 0 ? std::min<int64_t>(forced, (int64_t)1 << 20) : (int64_t)cb->ctx->devs[slot]->n_cus * 8;
    wgs = std::max<int64_t>(1, std::min<int64_t>(wgs, (n_chunks + pass - 1) / pass));
    hipLaunchKernelGGL(k_lists_merge_move, dim3((unsigned)wgs), dim3(kMergeThreads), 0, st, table, (int)(2 * n_lists), row_bytes,
                       (const uint8_t*)d_a, n_a * row_bytes, (const uint8_t*)d_b, n_b * row_bytes, (uint8_t*)d_out, total);
    HIPCHK(hipGetLastError());
    note_kernel("k_lists_merge_move");
    return PQHIP_OK;
}

}  // extern "C"
