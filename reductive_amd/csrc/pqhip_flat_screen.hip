// pqhip_flat_screen.hip -- conservative range screen over resident vectors on the matrix cores (include/pqhip.h:
// pqhip_flat_screen_f32_dev): the entry point, its policy (checks, queries per pass, grid, scratch, the prep / count /
// scan / fill sequence) and the instantiations of kernels_flat_screen.hip.h.  The scan is the ADC range searches'
// k_adc_range_scan.  A unit of its own so that the build compiles its kernels beside the other searches; nothing refers
// to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_flat_screen.hip.h"

using namespace pqhip;

namespace pqh {

constexpr int64_t kFlatScreenWgsMax = 2048;      // 16,384 units: a pass of 64 queries has 2^20 counts, what one scan launch sums
constexpr int kFlatScreenWideD = 1024;           // 64 queries per pass while their image fits the LDS (129 KB), else 32

struct FlatScreenLaunch {
    const void* x;
    int64_t n;
    int d;
    int64_t x_rs;
    const uint32_t* allow;
    const unsigned short* img;
    int ldq;
    float cx, cxx;
    int al;
    int64_t rows_per_wg;
    unsigned grid;
    int nq_pass;
    int64_t* part;
    uint32_t* hits;
    hipStream_t st;
};

template <typename T, int NB>
static int32_t launch_flat_screen_t(const FlatScreenLaunch& a)
{
    auto kern = k_flat_screen<T, NB>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(64 * kFsWaves), flat_screen_image_bytes(32 * NB, a.d), a.st, (const T*)a.x, a.n, a.d,
                       a.x_rs, a.allow, a.img, a.ldq, a.cx, a.cxx, a.al, a.rows_per_wg, a.nq_pass, a.part, a.hits);
    return PQHIP_OK;
}

static int32_t launch_flat_screen(bool f16, int nb, const FlatScreenLaunch& a)
{
    const int32_t status = dispatch_int<0, 1>(f16, [&](auto h_c) {
        return dispatch_int<2, 1>(nb, [&](auto nb_c) {
            using T = std::conditional_t<decltype(h_c)::value != 0, _Float16, float>;
            return launch_flat_screen_t<T, decltype(nb_c)::value>(a);
        });
    });
    if (status != PQHIP_OK) return status;
    HIPCHK(hipGetLastError());
    note_kernel(nb == 2 ? "k_flat_screen<64 queries>" : "k_flat_screen<32 queries>");
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

// Two 512-thread workgroups per CU by default (option "flat_screen_wgs" forces the number, up to 2,048), a contiguous row
// range each (a multiple of 256), cut into 8 wave sub-ranges by the kernel.  Passes of 64 queries while d <= 1,024, else
// of 32; the last pass takes what is left (32 or fewer: one block).  Scratch of a pass: the f16 image with its (s, tau)
// pairs, the partial counts [queries][units] and the hit bitmap, 4 bytes per (query slot, tile of 32 rows).
int32_t pqhip_flat_screen_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, const void* d_x,
                                  int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t x_rs, const uint32_t* d_allow, int32_t metric,
                                  int32_t x_exp, const float* d_thr, int64_t* d_lims, int64_t* d_idx, int64_t capacity, void* stream)
{
    if (!cb || nq < 0 || n_rows < 0 || capacity < 0 || d < 1 || (metric != 0 && metric != 1)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if ((vec_bytes != 2 && vec_bytes != 4) || d > kFlatScreenMaxD) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_lims || !d_thr || (capacity > 0 && !d_idx) || !d_q || (n_rows > 0 && !d_x)) return PQHIP_EINVAL;
    if (q_rs < d || (n_rows > 0 && x_rs < d)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        HIPCHK(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
        return PQHIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));         // lims[0]: the scan of the first pass starts from it
    const int64_t forced = cb->ctx->opt.flat_screen_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, kFlatScreenWgsMax)
                                   : std::min<int64_t>(2 * (int64_t)cb->ctx->devs[slot]->n_cus, kFlatScreenWgsMax);
    const int64_t rows_per_wg = round_up((n_rows + wgs - 1) / wgs, kFsWaves * kFsTile);
    const int64_t grid = (n_rows + rows_per_wg - 1) / rows_per_wg;
    const int64_t units = grid * kFsWaves;
    const int64_t tiles = (n_rows + kFsTile - 1) / kFsTile;
    const int nb_max = d <= kFlatScreenWideD ? 2 : 1;
    const int ldq = flat_screen_dp((int)d) + kFsRowPad;
    const size_t img_bytes = (size_t)round_up((int64_t)flat_screen_image_bytes(32 * nb_max, (int)d), 256);
    const size_t part_bytes = (size_t)32 * nb_max * units * sizeof(int64_t);
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire(img_bytes + part_bytes + (size_t)32 * nb_max * tiles * sizeof(uint32_t)));
    unsigned short* img = (unsigned short*)lease.ptr();
    int64_t* part = (int64_t*)((char*)lease.ptr() + img_bytes);
    uint32_t* hits = (uint32_t*)((char*)lease.ptr() + img_bytes + part_bytes);
    const int xe = (int)std::max<int32_t>(-126, std::min<int32_t>(126, x_exp));   // beyond +-40 every query returns every allowed row
    const bool ip = metric != 0;
    const uint64_t low = (uint64_t)(uintptr_t)d_x | ((uint64_t)x_rs * (uint64_t)vec_bytes);   // what base and row stride are both multiples of
    const int al = low % 16 == 0 ? 16 : low % 8 == 0 ? 8 : low % 4 == 0 ? 4 : 2;
    FlatScreenLaunch a{d_x, n_rows, (int)d, x_rs, d_allow, img, ldq, std::ldexp(1.0f, xe),
                       ip ? -0.5f * kFlatScreenRel : 1.0f - kFlatScreenRel, al, rows_per_wg, (unsigned)grid, 0, part, hits, st};
    for (int64_t q = 0; q < nq;) {
        const int nb = nb_max == 2 && nq - q > 32 ? 2 : 1;
        const int qp = 32 * nb;
        const int nqp = (int)std::min<int64_t>(nq - q, qp);
        hipLaunchKernelGGL(k_flat_screen_prep, dim3(qp), dim3(kFsPrepThreads), 0, st, d_q + q * q_rs, q_rs, nqp, (int)d, ldq, d_thr + q,
                           ip ? 1 : 0, (int)x_exp, img, (float*)(img + (size_t)qp * ldq));
        HIPCHK(hipGetLastError());
        note_kernel("k_flat_screen_prep");
        a.nq_pass = nqp;
        PQCHK(launch_flat_screen(vec_bytes == 2, nb, a));
        hipLaunchKernelGGL(k_adc_range_scan, dim3(1), dim3(1024), 0, st, part, units, (int64_t)nqp, d_lims + q);
        HIPCHK(hipGetLastError());
        note_kernel("k_adc_range_scan");
        if (capacity > 0) {                                         // capacity == 0: a pure count call
            hipLaunchKernelGGL(k_flat_screen_fill, dim3((unsigned)grid), dim3(64 * kFsWaves), 0, st, hits, qp, nqp, n_rows, rows_per_wg,
                               part, capacity, d_idx);
            HIPCHK(hipGetLastError());
            note_kernel("k_flat_screen_fill");
        }
        q += nqp;
    }
    return PQHIP_OK;
}

}  // extern "C"
