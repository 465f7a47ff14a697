// pqhip_rows_compact.hip -- stable compaction of a row array under a row mask on the device (include/pqhip.h:
// pqhip_rows_compact_dev): the primitive under removing rows from a resident matrix.  This unit holds the entry point, its
// checks, the grid choice and the three launches of kernels_rows_compact.hip.h; the slice and tile counts live in the
// codebook's scratch for the duration of the call.  Nothing else refers to this unit.
#include "pqhip_internal.h"

#include "kernels_rows_compact.hip.h"

using namespace pqhip;
using namespace pqh;

extern "C" {

int32_t pqhip_rows_compact_dev(pqhip_codebook* cb, int32_t slot, const uint32_t* d_keep, int64_t n, int64_t row_bytes,
                               const void* d_in, void* d_out, int64_t out_capacity_rows, const int64_t* d_off_in, int64_t n_lists,
                               int64_t* d_off_out, int64_t* d_src_rows, int64_t* d_count, void* stream)
{
    if (!cb || n < 0 || row_bytes < 1 || out_capacity_rows < 0 || !d_count || n_lists < 0) return PQHIP_EINVAL;
    if ((d_in == nullptr) != (d_out == nullptr) || (d_off_out && !d_off_in) || (n > 0 && !d_keep)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (row_bytes > PQHIP_ROWS_COMPACT_MAX_ROW_BYTES || n_lists > PQHIP_LISTS_MERGE_MAX_LISTS || n > ((int64_t)1 << 49))
        return PQHIP_EUNSUPPORTED;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
        if (d_off_out) HIPCHK(hipMemsetAsync(d_off_out, 0, (size_t)(n_lists + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    // slices of whole tiles; by default eight 256-thread workgroups per CU -- the 32 waves a CU holds
    const int64_t n_tiles = (n + kCompactTile - 1) / kCompactTile;
    const int64_t forced = cb->ctx->opt.rows_compact_wgs.load(std::memory_order_relaxed);
    int64_t G = forced > 0 ? std::min<int64_t>(forced, (int64_t)1 << 20) : (int64_t)cb->ctx->devs[slot]->n_cus * 8;
    G = std::max<int64_t>(1, std::min<int64_t>(G, n_tiles));
    const int64_t per = (n_tiles + G - 1) / G * kCompactTile;
    G = (n + per - 1) / per;
    // scratch: go [1] | slice counts, then first output rows [G] | tile counts [n_tiles], 32 bits each
    const int64_t bytes = (1 + G) * (int64_t)sizeof(int64_t) + n_tiles * (int64_t)sizeof(uint32_t);
    if (bytes > kScratchBytesMax) return PQHIP_EUNSUPPORTED;
    ErrFlag ef(cb, slot, st);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)bytes));
    int64_t* ctl = (int64_t*)lease.ptr();
    uint32_t* tile_cnt = (uint32_t*)(ctl + 1 + G);
    hipLaunchKernelGGL(k_rows_compact_count, dim3((unsigned)G), dim3(kCompactThreads), 0, st, d_keep, n, per, ctl + 1, tile_cnt);
    HIPCHK(hipGetLastError());
    note_kernel("k_rows_compact_count");
    hipLaunchKernelGGL(k_rows_compact_scan, dim3(1), dim3(1024), 0, st, ctl, G, tile_cnt, d_keep, n, per, out_capacity_rows, d_off_in,
                       n_lists, d_off_out, d_count, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_rows_compact_scan");
    if (!d_out && !d_src_rows) return PQHIP_OK;
    hipLaunchKernelGGL(k_rows_compact_move, dim3((unsigned)G), dim3(kCompactThreads), 0, st, ctl, d_keep, n, per, (uint32_t)row_bytes,
                       (const uint8_t*)d_in, (uint8_t*)d_out, d_src_rows);
    HIPCHK(hipGetLastError());
    note_kernel("k_rows_compact_move");
    return PQHIP_OK;
}

}  // extern "C"
