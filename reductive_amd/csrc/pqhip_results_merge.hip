// pqhip_results_merge.hip -- exact merge of the top-k results of several searches on the device (include/pqhip.h:
// pqhip_topk_merge_f32_dev): the primitive under searching several resident matrices as one.  This unit holds the entry
// point, its checks, the choice of list registers and waves and the one launch of kernels_results_merge.hip.h.  The call
// takes no scratch.  Nothing else refers to this unit.
#include "pqhip_internal.h"

#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of kernels_adc.hip.h belong to pqhip_adc.hip
#include "kernels_results_merge.hip.h"
#include "launch_dispatch.h"

using namespace pqhip;
using namespace pqh;

static_assert(PQHIP_TOPK_MERGE_MAX_K == (1 << kTopkMergeRankBits) && PQHIP_TOPK_MERGE_MAX_K == kSearchMaxK, "rank bits");
static_assert(PQHIP_TOPK_MERGE_MAX_PARTS == kTopkMergeMaxParts, "part bits");

extern "C" {

int32_t pqhip_topk_merge_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_val, int64_t v_ps, int64_t v_rs,
                                 const int64_t* d_idx, int64_t i_ps, int64_t i_rs, int64_t n_parts, int64_t nq, int32_t k_in,
                                 const int64_t* d_offsets, int32_t largest, int32_t k, float* d_out_val, int64_t ov_rs,
                                 int64_t* d_out_idx, int64_t oi_rs, int32_t* d_out_part, int64_t op_rs, void* stream)
{
    if (!cb || nq < 0 || n_parts < 1 || k < 1 || k_in < 1 || (largest != 0 && largest != 1)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (k > PQHIP_TOPK_MERGE_MAX_K || k_in > PQHIP_TOPK_MERGE_MAX_K || n_parts > PQHIP_TOPK_MERGE_MAX_PARTS) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_val || !d_idx || !d_out_val || !d_out_idx) return PQHIP_EINVAL;
    if (v_rs < k_in || i_rs < k_in || ov_rs < k || oi_rs < k || (d_out_part && op_rs < k)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    int L = 1;                                     // 64 L >= k: entries of a part past rank k cannot reach the output
    while (64 * L < k) L <<= 1;
    int waves = 1;                                 // one wave per part, a power of two
    while (waves < kSearchMergeWaves && waves < n_parts) waves <<= 1;
    const int64_t forced = cb->ctx->opt.topk_merge_wgs.load(std::memory_order_relaxed);
    const int64_t G = std::min<int64_t>(nq, forced > 0 ? std::min<int64_t>(forced, (int64_t)1 << 20) : (int64_t)1 << 20);
    const size_t lds = waves > 1 ? (size_t)(waves / 2) * 64 * L * 2 * sizeof(unsigned) : 0;   // at most 32 KB
    const int32_t status = dispatch_int<0, 1>(largest, [&](auto lg_c) {
        return dispatch_int<1, 2, 4, 8, 16>(L, [&](auto l_c) -> int32_t {
            hipLaunchKernelGGL((k_topk_merge<decltype(lg_c)::value != 0, decltype(l_c)::value>), dim3((unsigned)G), dim3(64 * waves), lds,
                               st, d_val, v_ps, v_rs, d_idx, i_ps, i_rs, d_offsets, (int)n_parts, nq, (int)k_in, (int)k, d_out_val,
                               ov_rs, d_out_idx, oi_rs, d_out_part, op_rs);
            return PQHIP_OK;
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(largest ? "k_topk_merge_largest" : "k_topk_merge");
    return PQHIP_OK;
}

}  // extern "C"
