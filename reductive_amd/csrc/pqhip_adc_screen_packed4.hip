// pqhip_adc_screen_packed4.hip -- the u8 table screen over 4-bit packed rows on the i8 matrix cores (include/pqhip.h:
// pqhip_adc_screen_packed4_f32_dev): the entry point, its host policy and the instantiations of
// kernels_adc_screen_packed4.hip.h.  The policy is adc_screen_run's (adc_screen_launch.h) with two differences that its
// policy type cannot express -- a pass holds 32 or 64 query slots, and k_adc_screen_fill (lane = query) is launched
// per group of 32 of them; part and hits are query-major, so a group is a pointer offset -- hence a run function of its
// own beside the shared launch record, launcher, scan and fill.  A unit of its own; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of kernels_adc.hip.h belong to pqhip_adc.hip
#include "adc_screen_launch.h"
#include "kernels_adc_screen_packed4.hip.h"

namespace pqh {

// packed dwords per row: the buckets of the packed searches (a wider window is always correct)
static int p4_screen_nv_bucket(int nv)
{
    for (int b : {1, 2, 4, 8, 13})
        if (nv <= b) return b;
    return 0;
}

// the most query blocks of a pass whose image and parameters fit the LDS; 0 when one does not.  Rows of more than 32
// packed bytes (nvb 13, M > 64) take one block: with two the 14 row dwords beside 32 accumulators spill vector registers.
static int p4_screen_blocks(int M, int nvb)
{
    for (int b : {2, 1})
        if ((b == 1 || nvb < 13) && p4_screen_lds_bytes(M, b) <= kAdcScreenLds) return b;
    return 0;
}

static int32_t p4_screen_count(int nvb, int blocks, const AdcScreenLaunch& a)
{
    const int32_t status = dispatch_int<1, 2, 4, 8, 13>(nvb, [&](auto nv_c) {
        return dispatch_int<2, 1>(blocks, [&](auto qb_c) {
            constexpr int NV = decltype(nv_c)::value, QB = decltype(qb_c)::value;
            if constexpr (NV == 13 && QB == 2) return (int32_t)PQHIP_EUNSUPPORTED;   // not instantiated (p4_screen_blocks)
            else return launch_adc_screen_kernel(k_adc_screen_p4<NV, QB>, p4_screen_lds_bytes(a.M, QB), a);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(blocks == 2 ? "k_adc_screen_p4<64 queries>" : "k_adc_screen_p4<32 queries>");
    return PQHIP_OK;
}

// Grid, row ranges, scratch and the sequence of a pass are adc_screen_run's; passes of the most blocks that fit, the last
// pass the fewest blocks that hold what is left.  Scratch of a pass: n / 8 bytes per query slot, 8 n at most.
static int32_t adc_screen_packed4_run(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                      int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t ip,
                                      const float* d_scales, const float* d_thr, int64_t* d_lims, int64_t* d_idx, int64_t capacity,
                                      void* stream)
{
    if (!cb || nq < 0 || n < 0 || capacity < 0 || (ip != 0 && ip != 1) || (!ip && d_scales)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || cb->M > kAdcScreenMaxM || cb->K > 16) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, K = (int)cb->K, PB = (M + 1) / 2;
    const int nvb = p4_screen_nv_bucket((PB + 3) / 4);
    const int blocks_max = p4_screen_blocks(M, nvb);
    if (nvb == 0 || blocks_max == 0) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || (n > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if (n > 0 && c_rs < PB) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first pass starts from it
    ErrFlag ef(cb, slot, st);
    const int64_t forced = cb->ctx->opt.adc_screen_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, kAdcScreenWgsMax)
                                   : std::min<int64_t>((int64_t)cb->ctx->devs[slot]->n_cus, kAdcScreenWgsMax);
    const int64_t rows_per_wg = round_up((n + wgs - 1) / wgs, 64 * kRangeWaves);
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    const int64_t units = grid * kRangeWaves;
    const int64_t words = (n + 63) / 64;
    const auto pass_blocks = [&](int64_t left) {                    // the fewest blocks that hold what is left
        return blocks_max > 1 && left <= 32 ? 1 : blocks_max;
    };
    const int slots_call = 32 * pass_blocks(nq);                    // the first pass is the widest
    const size_t head_bytes = 256;                                  // the largest scale
    const size_t img_bytes = (size_t)round_up((int64_t)p4_screen_lds_bytes(M, slots_call / 32), 256);
    const size_t part_bytes = (size_t)slots_call * units * sizeof(int64_t);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire(head_bytes + img_bytes + part_bytes + (size_t)slots_call * words * sizeof(unsigned long long)));
    unsigned* cmax = (unsigned*)lease.ptr();
    uint8_t* img = (uint8_t*)lease.ptr() + head_bytes;
    int64_t* part = (int64_t*)((char*)lease.ptr() + head_bytes + img_bytes);
    unsigned long long* hits = (unsigned long long*)((char*)lease.ptr() + head_bytes + img_bytes + part_bytes);
    if (d_scales) {
        HIPCHK(hipMemsetAsync(cmax, 0, sizeof(unsigned), st));
        const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
        hipLaunchKernelGGL(k_adc_screen_scale_max, dim3(g), dim3(256), 0, st, d_scales, n, cmax);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_screen_scale_max");
    }
    AdcScreenLaunch a{(const uint8_t*)d_codes, n, c_rs, d_allow, d_scales, img, M, K, rows_per_wg, (unsigned)grid, 0, words, part, hits,
                      ef.flag, st};
    for (int64_t q = 0; q < nq;) {
        const int blocks = pass_blocks(nq - q);
        const int nqp = (int)std::min<int64_t>(nq - q, 32 * blocks);
        hipLaunchKernelGGL(k_adc_screen_p4_prep, dim3(32 * blocks), dim3(kAsPrepThreads), 0, st, d_tables + q * (int64_t)M * K, nqp, M, K,
                           d_thr + q, (int)ip, d_scales ? 1 : 0, cmax, (int8_t*)img, (AdcScreenPrm*)(img + p4_screen_image_bytes(M, blocks)));
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_screen_p4_prep");
        a.nq_pass = nqp;
        PQCHK(p4_screen_count(nvb, blocks, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, (int64_t)nqp, d_lims + q);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        for (int g = 0; capacity > 0 && g < nqp; g += 32) {         // capacity == 0: a pure count call
            hipLaunchKernelGGL(k_adc_screen_fill, dim3((unsigned)grid), dim3(1024), 0, st, hits + (int64_t)g * words, words,
                               std::min(nqp - g, 32), n, rows_per_wg, part + (int64_t)g * units, capacity, d_idx);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_fill");
        }
        q += nqp;
    }
    return PQHIP_OK;
}

}  // namespace pqh

extern "C" {

int32_t pqhip_adc_screen_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                         int32_t code_bytes, int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t ip,
                                         const float* d_scales, const float* d_thr, int64_t* d_lims, int64_t* d_idx, int64_t capacity,
                                         void* stream)
{
    return pqh::adc_screen_packed4_run(cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_allow, ip, d_scales, d_thr, d_lims, d_idx,
                                       capacity, stream);
}

}  // extern "C"
