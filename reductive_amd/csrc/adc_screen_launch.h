// adc_screen_launch.h -- the host policy that the two table screens over resident u8 codes share (pqhip_adc_screen.hip:
// u8 image; pqhip_adc_screen16.hip: 16-bit image): checks, query slots per pass, grid, scratch, the prep / count / scan /
// fill sequence.  A unit names its image through a policy type P:
//     P::kSlots                       the slot counts of a pass, widest first
//     P::lds_bytes(M, K, slots)       image and parameters of a pass; P::image_bytes(M, K, slots) the image alone
//     P::prep(...)                    launches the preparation kernel of a pass
//     P::count(nvb, slots, launch)    launches the count kernel and names it (note_kernel)
#pragma once
#include "adc_search_launch.h"
#include "kernels_adc_screen.hip.h"

namespace pqh {

using namespace pqhip;

constexpr int64_t kAdcScreenWgsMax = 2048;       // 32,768 units: 2^20 counts per 32 queries of a pass for the one scan launch (it loops over any length)
constexpr size_t kAdcScreenLds = 160 * 1024;

struct AdcScreenLaunch {
    const uint8_t* codes;
    int64_t n, c_rs;
    const uint32_t* allow;
    const float* scales;
    const uint8_t* img;
    int M, K;
    int64_t rows_per_wg;
    unsigned grid;
    int nq_pass;
    int64_t words;
    int64_t* part;
    unsigned long long* hits;
    int* err;
    hipStream_t st;
};

// launches a count kernel of the signature both screens share with the whole LDS as its dynamic limit
template <typename Kern>
static int32_t launch_adc_screen_kernel(Kern kern, size_t lds, const AdcScreenLaunch& a)
{
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAdcScreenLds));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), lds, a.st, a.codes, a.n, a.c_rs, a.allow, a.scales, a.img, a.M, a.K, a.rows_per_wg,
                       a.nq_pass, a.words, a.part, a.hits, a.err);
    return PQHIP_OK;
}

// the most query slots of a pass whose image and parameters fit the LDS; 0 when the fewest do not
template <typename P>
static int adc_screen_slots(int M, int K)
{
    for (int c : P::kSlots)
        if (P::lds_bytes(M, K, c) <= kAdcScreenLds) return c;
    return 0;
}

// One 1,024-thread workgroup per CU by default (option "adc_screen_wgs" forces the number, up to 2,048), a contiguous row
// range each (a multiple of 1,024), cut into 16 wave sub-ranges by the kernel.  Passes of the most slots that fit; the
// last pass takes the least slot count that holds what is left.  Scratch of a pass: the largest scale, the image with
// its parameters, the partial counts [queries][units] and the hit bitmap, 8 bytes per (query slot, 64 rows) -- n / 8
// bytes per query, 4 n at most: a call needs no chunking beyond its passes.
template <typename P>
static int32_t adc_screen_run(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes, int32_t code_bytes,
                              int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t ip, const float* d_scales, const float* d_thr,
                              int64_t* d_lims, int64_t* d_idx, int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n < 0 || capacity < 0 || (ip != 0 && ip != 1) || (!ip && d_scales)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || cb->M > kAdcScreenMaxM) return PQHIP_EUNSUPPORTED;
    const int nvb = search_nv_bucket(((int)cb->M + 3) / 4);
    const int slots_max = adc_screen_slots<P>((int)cb->M, (int)cb->K);
    if (nvb == 0 || slots_max == 0) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || (n > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if (n > 0 && c_rs < cb->M) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first pass starts from it
    ErrFlag ef(cb, slot, st);
    const int M = (int)cb->M, K = (int)cb->K;
    const int64_t forced = cb->ctx->opt.adc_screen_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, kAdcScreenWgsMax)
                                   : std::min<int64_t>((int64_t)cb->ctx->devs[slot]->n_cus, kAdcScreenWgsMax);
    const int64_t rows_per_wg = round_up((n + wgs - 1) / wgs, 64 * kRangeWaves);
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    const int64_t units = grid * kRangeWaves;
    const int64_t words = (n + 63) / 64;
    const auto pass_slots = [&](int64_t left) {                     // the least slot count that holds what is left
        for (int c : {4, 8, 16})
            if (c < slots_max && left <= c) return c;
        return slots_max;
    };
    const int slots_call = pass_slots(nq);                          // the first pass is the widest
    const size_t head_bytes = 256;                                  // the largest scale
    const size_t img_bytes = (size_t)round_up((int64_t)P::lds_bytes(M, K, slots_call), 256);
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
        const int slots = pass_slots(nq - q);
        const int nqp = (int)std::min<int64_t>(nq - q, slots);
        P::prep(slots, st, d_tables + q * (int64_t)M * K, nqp, M, K, d_thr + q, (int)ip, d_scales ? 1 : 0, cmax, img,
                (AdcScreenPrm*)(img + P::image_bytes(M, K, slots)));
        HIPCHK(hipGetLastError());
        a.nq_pass = nqp;
        PQCHK(P::count(nvb, slots, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, (int64_t)nqp, d_lims + q);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) {                                         // capacity == 0: a pure count call
            hipLaunchKernelGGL(k_adc_screen_fill, dim3((unsigned)grid), dim3(1024), 0, st, hits, words, nqp, n, rows_per_wg, part,
                               capacity, d_idx);
            HIPCHK(hipGetLastError());
            note_kernel("k_adc_screen_fill");
        }
        q += nqp;
    }
    return PQHIP_OK;
}

}  // namespace pqh
