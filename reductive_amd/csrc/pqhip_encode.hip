// pqhip_encode.hip -- PQ encode dispatch of libpqhip.so: plan_encode() decides which kernel family serves a call (pure: no
// HIP call, no allocation); one helper per family fills its arguments and launch geometry.
// (primitives.rs:64-104 -> kmeans.rs:133-159 -> linalg.rs:150-180, fused in every kernel.)
#include "pqhip_internal.h"

#include "kernels_anchor.hip.h"
#include "kernels_pair16.hip.h"
#include "encode_launch.h"
#include "opq_fused2_launch.h"
#include "smallk_launch.h"
#include "small16_launch.h"
#include "vor2_launch.h"
#include "wide_launch.h"

using namespace pqhip;

namespace pqh {

static EncodePlan planned(EncodeFamily f, const char* kernel) { EncodePlan p; p.family = f; p.kernel = kernel; return p; }
static EncodePlan unsupported() { EncodePlan p; p.status = PQHIP_EUNSUPPORTED; return p; }

static EncodePlan mfma_plan(const pqhip_codebook& cb, int kind)
{
    static const char* const names[2][3] = {{"k_encode_mfma<odd>", "k_encode_mfma<vec2>", "k_encode_mfma<vec4>"},
                                            {"k_encode_mfma_lds3<odd>", "k_encode_mfma_lds3<vec2>", "k_encode_mfma_lds3<vec4>"}};
    EncodePlan p = planned(EncodeFamily::mfma, "k_encode_mfma16");
    p.kind = kind; p.vec = cb.DP == cb.dsub; p.grp = (cb.DP % 4 == 0) ? 4 : 2;
    if (kind != 3) p.kernel = (!p.vec && cb.DP > 32) ? "k_encode_mfma_lds3<padded>" : names[kind / 2][p.vec ? p.grp / 2 : 0];
    return p;
}

EncodePlan plan_encode(const pqhip_codebook& cb, const EncodeCall& c, const Options& opt)
{
    const int v = cb.variant;
    const int DP = cb.DP, T = cb.T, dsub = (int)cb.dsub;
    const bool u8 = c.code_bytes == 1, u8_u32 = c.code_bytes == 1 || c.code_bytes == 4;
    const bool host_norms = cb.norms_ok && !c.bad_flag;    // the kernels that rely on the host's finite-norm check
    if (c.opq_rows) {
        // OPQ (pq.rs:276) in ONE kernel where kernels_opq_fused2.hip.h is instantiated (P block AND codebook fragments in LDS,
        // x straight from global memory, the rotated rows never leave the register file: no scratch buffer, no chunk loop).
        // Needs u8 codes from a codebook with finite norms and 16-byte aligned rows.  Variant 8.
        const bool fits = u8 && cb.groups == 1 && T != 0 && cb.norms_ok && dsub % 2 == 0 && dsub <= 32 && cb.d % 4 == 0 &&
                          c.rows_aligned && opq_fused2_has(dsub, T, (int)cb.d);
        // auto unless the context option "opq_fused" = 0 (or PQHIP_FUSED2_OPQ=0) keeps the two-kernel path (same-box A/B,
        // 10 M x 300: 29.95 vs 30.57 ms in steady state, and the HBM traffic of a step drops from 3.5x to ~1x the algorithmic bytes)
        const bool auto_ = opt.opq_fused.load(std::memory_order_relaxed) != 0;
        if (fits && (v == 8 || (v == 0 && auto_))) return planned(EncodeFamily::opq_fused, "k_opq_encode_fused2");
        return v == 8 ? unsupported() : planned(EncodeFamily::rotated, "");
    }
    if (v == 8) return unsupported();               // (the fused OPQ kernel reads the caller's rows only)
    if (v == 1) return u8_u32 ? planned(EncodeFamily::anchor, "k_encode_scalar") : unsupported();

    // 128 < dsub <= 1,024 (kernels_mfma_wide.hip.h) and K > 256 (the default kernel on groups of 256 centroids): launch_keyed
    const bool wide_fits = cb.wide && cb.norms_ok && u8_u32 && wide_has(T, DP);
    const bool grouped_fits = cb.groups > 1 && !cb.wide && cb.norms_ok && c.code_bytes == 4 && mfma_has(2, 8, DP, DP == dsub, 8);
    // 1- and 2-float sub-vectors, K <= 256: only the centroids that can win in the point's grid cell are evaluated
    // (kernels_vor2.hip.h; the tables exist for Pq handles whose centroids are finite and within range, and fit LDS).
    const bool vor2_fits = cb.vor2 && u8 && host_norms &&
                           vor2_has_grid((int)cb.M, (int)cb.K, dsub, cb.vor2_max_region_words, c.n, c.n_cus);
    // Auto above 16 centroids (tools: bench.py --d .. --variant 0 / 2 / 4, vectors/s against the best kernel that evaluates every
    // centroid): d=20 M=10 K=128 (the reference's test shape) 1.7e10 / 5.3e9, K=256 1.5e10 / 2.5e9, K=32 1.44e10 / 1.31e10;
    // d=64 M=32 K=128 6.3e9 / 1.75e9; d=300 M=150 K=256 9.3e8 / 1.7e8; one-float sub-vectors d=128 M=128 K=256 2.0e9 / 2.0e8.
    // Up to 16 centroids the pair kernel below is faster (d=128 M=64 K=16: 3.6e9 against 1.8e9 here).
    const bool vor2_auto = cb.K > 16 || dsub == 1;
    // K <= 16 with sub-vectors of 2 / 4 / 8 / 16 floats: one matrix tile serves two subquantizers, x is read once in whole
    // lines (kernels_pair16.hip.h).
    const bool pair_fits = cb.pair16 && u8 && host_norms;
    // Measured (tools/smallk_ab.sh, one box, vectors/s pair / VALU kernel / default MFMA kernel): d=128 M=64 (dsub 2) 3.59e9 / 3.31e9 /
    // 1.50e9; d=300 M=75 (dsub 4) 2.14e9 / 1.41e9 / 1.21e9; d=128 M=32 (dsub 4) 5.09e9 / 5.61e9 / 2.89e9; d=128 M=16 (dsub 8, the
    // reference's bench shape) 5.95e9 / 6.69e9 / 4.76e9; d=768 M=48 (dsub 16) 1.14e9 / 0.70e9 / 1.18e9 -- the zero blocks double the
    // matrix time, which the shared FP32 pipe charges in full, so auto takes it only where it wins: dsub 2, and dsub 4 with many
    // subquantizers.
    const bool pair_auto = dsub == 2 || (dsub == 4 && cb.M >= 48);
    // K <= 32, sub-vectors of 4 / 8 / 12 / 16 / 20 / 24 / 32 floats and 16-byte aligned rows: the 16x16x4 kernel with the
    // transposed codebook image in LDS (kernels_small16.hip.h).
    const bool s16_fits = cb.KP != 0 && small16_has(cb.KP, dsub) && u8 && host_norms && c.rows_aligned &&
                          small16_lds_bytes((int)cb.M, dsub, cb.KP) <= 96 * 1024;
    // Auto wherever it fits: it is the fastest kernel for every such shape measured (tools/small16_sweep.sh, vectors/s against the
    // best of the others): d=128 M=16 K=16 7.4e9 / 6.2e9, d=128 M=32 (dsub 4) 5.6e9 / 5.0e9, d=256 M=32 4.1e9 / 3.2e9, d=768 M=96
    // 1.29e9 / 0.85e9, d=64 M=8 1.41e10 / 1.10e10, K=32: d=128 M=16 5.2e9 / 4.5e9, d=300 M=75 1.49e9 / 1.25e9 -- except 4-float
    // sub-vectors from 48 subquantizers on at K <= 16, which stay with the pair kernel above (d=300 M=75: 1.95e9 / 2.07e9).
    // 16- and 32-float sub-vectors (tools/small16_sweep16.sh): d=768 M=48 K=16 1.48e9 / 1.11e9, d=128 M=8 8.0e9 / 6.3e9,
    // d=1024 M=64 1.09e9 / 0.85e9, d=1024 M=32 1.25e9 / 1.05e9, d=768 M=24 1.44e9 / 1.37e9, K=32: d=128 M=8 5.8e9 / 5.5e9;
    // 12 / 20 / 24 floats: d=300 M=25 3.0e9 / 2.25e9, d=300 M=15 K=16 (the headline shape with 4-bit codes) 3.2e9 / 2.7e9,
    // d=768 M=32 1.47e9 / 1.15e9, d=300 M=15 K=32 2.57e9 / 2.57e9.
    // Small codebooks (K <= 64): the VALU kernel reads x once, in whole row segments, and keeps the centroids on the scalar
    // path (kernels_smallk.hip.h).
    const bool smallk_fits = cb.KP != 0 && smallk_has(dsub) && u8 && host_norms;
    // Auto for K <= 16 with sub-vectors of <= 8 floats -- the reference's own bench shape, d = 128, M = 16, K = 16: 6.3e9
    // vectors/s against 4.4e9 for the MFMA kernel; for wider sub-vectors or K = 32 / 64 the MFMA kernels are still the faster
    // ones (tools/smallk_sweep.sh).
    const bool smallk_auto = cb.KP == 16 && dsub <= 8;
    // MFMA kernels (K <= 256, dsub <= 128): u8 codes from every kind, u32 codes (k-means assignments, wide index types) from
    // kinds 2 and 3
    const bool mfma_fits = !cb.wide && cb.groups == 1 && T != 0 && (cb.norms_ok || c.bad_flag) && u8_u32;
    // kind 0, the VALU-argmin kernel, keeps all T * DP/2 fragments in registers: small codebooks only
    const bool kind0_fits = mfma_fits && DP <= 32 && T * (DP / 2) <= 128 && u8 && mfma_has(0, T, DP, DP == dsub, c.code_bytes);
    // auto: for sub-vectors of <= 2 floats the per-distance work outweighs the MFMA chain and the
    // LDS pipe (one atomic per 64 distances) becomes the bound: the VALU-argmin kernel is 4-20 % faster
    // (round 3: with the hybrid lane-local + LDS argmin of the default kernel, 4-float sub-vectors moved to the default:
    // d=300 M=75 2.98e8 vs 2.80e8 vectors/s; 2-float ones stay here: M=150 1.62e8 vs 1.69e8, d=20 M=10 K=128 4.3e9 vs 5.1e9)
    const bool kind0_auto = DP <= 2 && u8;
    // kind 3 (k_encode_mfma16: the same epilogue as kind 2 on v_mfma_f32_16x16x4_f32, four waves per SIMD) is instantiated for
    // >= 64 centroids and sub-vectors of 4, 8, .., 32 real floats
    const bool kind3_fits = mfma_fits && mfma_has(3, T, DP, DP == dsub, c.code_bytes);
    // auto takes it where it wins on one box (tools/mfma16_shapes.sh, profiles/r3_encode_experiments.md): K > 128 and 12..24
    // floats -- +2 % at 12 / 24, +2.5 % at 20, +5 % at 16; shorter chains lose to the hybrid argmin of kind 2 (-15 % at 4
    // floats), 32 floats leave only 3 waves per SIMD (-2.4 %), and with 64 / 128 centroids the per-tile work (norms, row loads,
    // code bytes) weighs more (-1 .. -18 %).  (beside_update: the k-means assignment step, whose update kernels run beside it on
    // a second stream: with four encode waves per SIMD the iteration was 2 % slower -- 20.4 vs 19.95 ms per 10 M rows -- so that
    // caller stays on kind 2)
    const bool kind3_auto = T == 8 && DP >= 12 && DP <= 24 && !c.beside_update && !diag().no_mfma16;

    constexpr int kEveryVariant = -1;
    struct Rule { EncodeFamily family; int kind, variant; bool fits, auto_; const char* kernel; };
    const Rule rules[] = {
        {EncodeFamily::wide, 0, kEveryVariant, wide_fits, true, "k_encode_mfma_wide"},
        {EncodeFamily::grouped, 2, kEveryVariant, grouped_fits, true, "k_encode_mfma_lds3<grouped>"},
        {EncodeFamily::vor2, 0, 11, vor2_fits, vor2_auto, "k_encode_vor2"},
        {EncodeFamily::pair16, 0, 7, pair_fits, pair_auto, "k_encode_pair16"},
        {EncodeFamily::small16, 0, 10, s16_fits, true, "k_encode_small16"},
        {EncodeFamily::smallk, 0, 6, smallk_fits, smallk_auto, "k_encode_smallk"},
        {EncodeFamily::mfma, 0, 2, kind0_fits, kind0_auto, nullptr},
        {EncodeFamily::mfma, 3, 9, kind3_fits, kind3_auto, nullptr},
        {EncodeFamily::mfma, 2, 4, mfma_fits && mfma_has(2, T, DP, DP == dsub, c.code_bytes), true, nullptr},   // the default
    };
    for (const Rule& r : rules) {
        const bool take = r.variant == v ? r.fits : (v == 0 || r.variant == kEveryVariant) && r.fits && r.auto_;
        if (take) return r.family == EncodeFamily::mfma ? mfma_plan(cb, r.kind) : planned(r.family, r.kernel);
        if (r.variant == v) return unsupported();
    }
    return u8_u32 ? planned(EncodeFamily::anchor, "k_encode_scalar") : unsupported();
}

EncodeCall encode_call(const pqhip_codebook* cb, int slot, const EncodeIo& io, int64_t n, int code_bytes)
{
    EncodeCall c;
    c.n = n; c.code_bytes = code_bytes;
    c.rows_aligned = io.x_rs % 4 == 0 && ((uintptr_t)io.x & 15) == 0;
    c.word_codes = io.o_rs % 4 == 0 && ((uintptr_t)io.codes & 3) == 0;
    c.bad_flag = io.bad_flag != nullptr;
    c.n_cus = cb->ctx->devs[slot]->n_cus;
    return c;
}

// ---- launch helpers: arguments and geometry of the planned kernel ---------------------------------------------------
static int32_t no_instantiation(const char* kernel) { g_hip_err = std::string("no instantiation: ") + kernel; return PQHIP_EHIP; }
// the answer of a family's launcher (launch_dispatch.h): a kernel the plan names and the launcher does not have is an error
static int32_t launched(int32_t status, const char* kernel) { return status == PQHIP_OK ? PQHIP_OK : no_instantiation(kernel); }

// wide and grouped: one 64-bit key {ordered distance, global index} per (row, group of <= 128 / 256 centroids), k_merge_keys ->
// codes; the wide kernel takes squared norms from a pre-pass.  Keys and norms: one leased scratch buffer, rows chunked to <= 1 GiB.
static int32_t launch_keyed(pqhip_codebook* cb, int slot, const EncodePlan& p, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    const bool wide = p.family == EncodeFamily::wide;
    const int64_t n = c.n, Mv = cb->M * cb->groups;
    const int64_t per_row = Mv * 8 + (wide ? cb->M * 4 : 0);
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(4096, (1ll << 30) / per_row));
    ScratchLease buf(cb, slot, io.st);
    PQCHK(buf.acquire((size_t)chunk * per_row));
    unsigned long long* keys = (unsigned long long*)buf.ptr();
    float* xx = (float*)(keys + chunk * Mv);
    // grouped: 4 row streams per 4,096 items, <= 1,024 rows each; wide: one wave per SIMD, one workgroup per CU, <= 512 rows
    const int64_t per_item = wide ? 1024 : 4096, rpi_max = wide ? 512 : 1024;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min<int64_t>(chunk, n - r0);
        const float* x = io.x + r0 * io.x_rs;
        if (wide) { launch_row_norms(x, rows, io.x_rs, (int)cb->M, (int)cb->dsub, xx, io.st); note_kernel("k_row_norms"); }
        EncodeArgs a;
        a.x = x; a.n = rows; a.x_rs = io.x_rs; a.out = keys; a.o_rs = Mv;
        a.frags = cd.frags; a.cc = cd.cc; a.cb = cd.cb;
        a.M = (int)Mv; a.K = (int)cb->K; a.dsub = (int)cb->dsub; a.k_pad = cb->k_pad;
        a.groups = cb->groups; a.bad_flag = nullptr;
        const int64_t rpi = std::max<int64_t>(32, std::min<int64_t>(rpi_max, round_up((rows * Mv + 4 * per_item - 1) / (4 * per_item), 32)));
        a.rows_per_item = (int)rpi;
        a.n_chunks = (rows + 4 * rpi - 1) / (4 * rpi);
        a.chunks_per_xcd = (a.n_chunks + 7) / 8;
        const dim3 grid((unsigned)(a.chunks_per_xcd * Mv * 8));
        PQCHK(launched(wide ? launch_encode_wide(cb->T, cb->DP, a, xx, grid, io.st)
                            : launch_encode_mfma(2, 8, cb->DP, cb->DP == cb->dsub, 8, a, grid, io.st, diag().lds_pad),
                       p.kernel));
        note_kernel(p.kernel);
        const unsigned mg = (unsigned)std::min<int64_t>((rows * cb->M + 255) / 256, 256 * 32);
        if (c.code_bytes == 4)
            hipLaunchKernelGGL((k_merge_keys<uint32_t>), dim3(mg), dim3(256), 0, io.st, (const unsigned long long*)keys, rows, (int)cb->M,
                               cb->groups, (uint32_t*)io.codes + r0 * io.o_rs, io.o_rs);
        else
            hipLaunchKernelGGL((k_merge_keys<uint8_t>), dim3(mg), dim3(256), 0, io.st, (const unsigned long long*)keys, rows, (int)cb->M,
                               cb->groups, (uint8_t*)io.codes + r0 * io.o_rs, io.o_rs);
        HIPCHK(hipGetLastError());
        note_kernel("k_merge_keys");
    }
    return PQHIP_OK;
}

static int32_t launch_opq_fused(pqhip_codebook* cb, int slot, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    const int DP = (int)cb->dsub;
    OpqFusedArgs a;
    a.x = io.x; a.n = c.n; a.x_rs = io.x_rs; a.P = cd.P; a.d = (int)cb->d;
    a.frags = cd.frags; a.cc = cd.cc; a.cb = cd.cb; a.out = (uint8_t*)io.codes; a.o_rs = io.o_rs;
    a.M = (int)cb->M; a.K = (int)cb->K; a.k_pad = cb->k_pad;
    const int nm = opq_fused2_slots(DP, cb->T, (int)cb->d) / DP;      // sub-vectors per column block (64 or 32 slots)
    a.ncb = (int)((cb->M + nm - 1) / nm);
    // tiles of 32 rows per wave: as many as leave ~8 rounds of workgroups (one per CU) for the whole launch, 4 .. 96
    // (10 M x 300, one box: 12 tiles 29.84 ms, 24: 29.57, 48: 29.40, 96: 29.24, 160: 30.6, 192 (4 rounds): 38.8 --
    // the P block and three fragment sets, 138 KB, are staged once per workgroup)
    const int64_t want_rg = std::max<int64_t>(1, 8ll * c.n_cus / a.ncb);
    const int f2_tiles = diag().fused2_tiles ? diag().fused2_tiles : (int)std::max<int64_t>(4, std::min<int64_t>(96, (c.n / want_rg + 255) / 256));
    a.rows_per_wg = 8 * 32 * f2_tiles;              // 8 waves x f2_tiles tiles of 32 rows
    const int64_t n_rg = (c.n + a.rows_per_wg - 1) / a.rows_per_wg;
    a.rg_per_xcd = (n_rg + 7) / 8;
    const dim3 grid((unsigned)(a.rg_per_xcd * a.ncb * 8));
    StampRun stamps;      // (diagnostic builds: in-kernel s_memtime summary of the launch)
    PQCHK(stamps.begin(diag().fused_stamp, (size_t)grid.x * 8 * 5, io.st));
    a.stamps = stamps.ptr();
    const int e = launch_opq_fused2(DP, cb->T, a, grid, io.st);
    if (e < 0) return no_instantiation("k_opq_encode_fused2");
    if (e > 0) { g_hip_err = std::string("k_opq_encode_fused2: ") + hipGetErrorString((hipError_t)e); return PQHIP_EHIP; }
    return stamps.report5(io.st, "fused2", "rotation", "encode");
}

static int32_t launch_vor2_family(pqhip_codebook* cb, int slot, const EncodeCall& c, const EncodeIo& io)
{
    const CodebookDev& cd = cb->dev[slot];
    const Vor2Launch l{io.x, c.n, io.x_rs, (uint8_t*)io.codes, io.o_rs, cd.cb, cd.cc, cd.vor2_tab, cd.vor2_off,
                       (int)cb->M, (int)cb->K, cb->k_pad, (int)cb->dsub, cb->vor2_max_region_words, c.n_cus};
    return launched(launch_vor2(l, io.st), "k_encode_vor2");
}

template <int D>
static int32_t pair16(const Pair16Args& a, unsigned grid, size_t lds, hipStream_t st)
{
    if constexpr (!pair16_has(D)) {
        return PQHIP_EUNSUPPORTED;
    } else {
        HIPCHK(hipFuncSetAttribute((const void*)k_encode_pair16<D>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((k_encode_pair16<D>), dim3(grid), dim3(256), lds, st, a);
        return PQHIP_OK;
    }
}

static int32_t launch_pair16(pqhip_codebook* cb, int slot, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    Pair16Args a;
    const int NP = (int)((cb->M + 1) / 2);
    a.x = io.x; a.n = c.n; a.x_rs = io.x_rs; a.out = (uint8_t*)io.codes; a.o_rs = io.o_rs;
    a.fragp = cd.fragp; a.ccp = cd.fragp + (int64_t)NP * cb->dsub * 64; a.cb = cd.cb; a.cc = cd.cc;
    a.M = (int)cb->M; a.K = (int)cb->K; a.k_pad = cb->k_pad; a.NP = NP;
    a.n_tiles = (c.n + 31) / 32;
    const size_t lds = ((size_t)NP * cb->dsub * 64 + (size_t)NP * 32 + 4 * 2 * 32 * 36) * sizeof(float);
    const int per_cu = std::max<int>(1, std::min<int>(3, (int)(160 * 1024 / lds)));
    const unsigned grid = (unsigned)std::min<int64_t>((a.n_tiles + 3) / 4, (int64_t)c.n_cus * per_cu);
    // candidates: the power-of-two sub-vector lengths up to 32 floats
    const int32_t status = dispatch_int<1, 2, 4, 8, 16, 32>((int)cb->dsub, [&](auto d_c) { return pair16<decltype(d_c)::value>(a, grid, lds, io.st); });
    return status == PQHIP_EUNSUPPORTED ? no_instantiation("k_encode_pair16") : status;
}

// the small-codebook kernels: k_encode_small16 (16x16x4, codebook image in LDS) and k_encode_smallk (VALU)
static int32_t launch_small(pqhip_codebook* cb, int slot, const EncodePlan& p, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    SmallKArgs a;
    a.x = io.x; a.n = c.n; a.x_rs = io.x_rs; a.out = (uint8_t*)io.codes; a.o_rs = io.o_rs;
    a.cbt = cd.cbt; a.cc = cd.cc; a.cb = cd.cb;
    a.M = (int)cb->M; a.K = (int)cb->K; a.k_pad = cb->k_pad;
    if (p.family == EncodeFamily::smallk)
        return launched(launch_smallk(cb->KP, (int)cb->dsub, a, dim3((unsigned)((c.n + 255) / 256)), io.st), p.kernel);
    // consecutive 64-row tiles per wave: the codebook image is staged once per workgroup, so as many as leave about
    // eight rounds of workgroups for the launch
    const int64_t tile_rows = small16_tile_rows((int)cb->dsub);
    const int64_t n_tiles = (c.n + tile_rows - 1) / tile_rows;
    const int64_t wg_slots = (int64_t)c.n_cus * 4 * 8;
    a.word_stores = c.word_codes ? 1 : 0;
    a.tiles_per_wave = (int)std::max<int64_t>(1, std::min<int64_t>(kSmall16TilesMax, n_tiles / (4 * wg_slots)));
    const size_t lds = small16_lds_bytes(a.M, (int)cb->dsub, cb->KP);
    const dim3 grid((unsigned)((n_tiles + 4 * a.tiles_per_wave - 1) / (4 * a.tiles_per_wave)));
    return launched(launch_small16(cb->KP, (int)cb->dsub, a, grid, lds, io.st), p.kernel);
}

static int32_t launch_mfma(pqhip_codebook* cb, int slot, const EncodePlan& p, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    const int64_t n = c.n;
    EncodeArgs a;
    a.x = io.x; a.n = n; a.x_rs = io.x_rs; a.out = io.codes; a.o_rs = io.o_rs;
    a.frags = cd.frags; a.cc = cd.cc; a.cb = cd.cb;
    a.M = (int)cb->M; a.K = (int)cb->K; a.dsub = (int)cb->dsub; a.k_pad = cb->k_pad;
    a.groups = 1; a.bad_flag = io.bad_flag;
    a.screen_img = cd.screen_img;
    // the screen body of k_encode_mfma16 reads the prepared image and nothing else: without one there is no launch
    if (p.kind == 3 && mfma16_screen_shape(cb->T, cb->DP)) {
        if (!a.screen_img) return no_instantiation("k_encode_mfma16 (no screen image)");
        // a training handle whose centroids moved since its image was built: build it now, in front of the launch that reads it
        if (cd.screen_img_stale) PQCHK(build_screen_image(cb, slot, io.st));
    }
    dim3 grid;
    if (p.kind >= 2) {
        // one workgroup = one subquantizer x 4 row streams (one per wave)
        const int64_t rpi_max = diag().rpi_max, rpi_min = diag().rpi_min;
        int64_t rpi = round_up((n * cb->M + 4 * 4096 - 1) / (4 * 4096), 32);
        rpi = std::max<int64_t>(rpi_min, std::min<int64_t>(rpi_max, rpi));
        if (p.kind == 3) rpi = std::min<int64_t>(rpi, 32 * kMfma16MaxTiles);   // one bit per row tile in the wave's exact-path mask
        a.rows_per_item = (int)rpi;
        a.n_chunks = (n + 4 * rpi - 1) / (4 * rpi);       // row groups
        a.chunks_per_xcd = (a.n_chunks + 7) / 8;
        grid = dim3((unsigned)(a.chunks_per_xcd * cb->M * 8));
    } else {
        // ~2 items per wave slot (256 CUs x 8 waves), 32..1024 rows each
        const int64_t rpi = std::max<int64_t>(32, std::min<int64_t>(1024, round_up((n * cb->M + 4095) / 4096, 32)));
        a.rows_per_item = (int)rpi;
        a.n_chunks = (n + rpi - 1) / rpi;
        a.chunks_per_xcd = (a.n_chunks + 7) / 8;
        grid = dim3((unsigned)((a.chunks_per_xcd * cb->M + 3) / 4 * 8));     // four items per workgroup
    }
    // (row alignment does not matter: the loads are dword-aligned wide loads)
    StampRun stamps;      // (diagnostic builds: in-kernel s_memtime summary of the launch)
    const int stamp_words = (p.kind == 3 && mfma16_screen_shape(cb->T, cb->DP)) ? kScreenStampWords : 5;
    PQCHK(stamps.begin(diag().enc_stamp && p.kind >= 2, (size_t)grid.x * 4 * stamp_words, io.st));
    a.stamps = stamps.ptr();
    PQCHK(launched(launch_encode_mfma(p.kind, cb->T, cb->DP, p.vec, c.code_bytes, a, grid, io.st, diag().lds_pad), p.kernel));
    // k_encode_mfma16 (kind 3) leaves row counts in word 2: of the rows the screen does not decide, those with at most
    // one candidate per lane half (two at most: the rows encode_rows_few can take), and all others (both zero in its FP32 body);
    // kinds 0 and 2 leave the seam cycles there.  The screen body adds the
    // image-staging cycles as a sixth word, the few-candidate rows that found their wave's list full as a seventh,
    // the cycles after the loop as an eighth, and of those the cycles in encode_rows_few and in encode_rows_cand_f16
    // as a ninth and a tenth.
    if (p.kind == 3) return stamps.report5(io.st, "encode", "steps", "one-per-half / other off-screen", true, stamp_words);
    return stamps.report5(io.st, "encode", "steps", "seam");
}

static int32_t launch_anchor(pqhip_codebook* cb, int slot, const EncodeCall& c, const EncodeIo& io)
{
    CodebookDev& cd = cb->dev[slot];
    const unsigned grid = (unsigned)std::min<int64_t>((c.n * cb->M + 255) / 256, 256 * 32);
    if (c.code_bytes == 1)
        hipLaunchKernelGGL((k_encode_scalar<uint8_t>), dim3(grid), dim3(256), 0, io.st, io.x, c.n, io.x_rs, (uint8_t*)io.codes, io.o_rs, cd.cb,
                           cd.cc, (int)cb->M, (int)cb->K, (int)cb->dsub, cb->k_pad);
    else
        hipLaunchKernelGGL((k_encode_scalar<uint32_t>), dim3(grid), dim3(256), 0, io.st, io.x, c.n, io.x_rs, (uint32_t*)io.codes, io.o_rs,
                           cd.cb, cd.cc, (int)cb->M, (int)cb->K, (int)cb->dsub, cb->k_pad);
    return PQHIP_OK;
}

int32_t encode_planned(pqhip_codebook* cb, int slot, const EncodePlan& p, const EncodeCall& c, const EncodeIo& io)
{
    if (p.status != PQHIP_OK) return p.status;
    switch (p.family) {
    case EncodeFamily::wide: case EncodeFamily::grouped: PQCHK(launch_keyed(cb, slot, p, c, io)); break;
    case EncodeFamily::opq_fused: PQCHK(launch_opq_fused(cb, slot, c, io)); break;
    case EncodeFamily::vor2: PQCHK(launch_vor2_family(cb, slot, c, io)); break;
    case EncodeFamily::pair16: PQCHK(launch_pair16(cb, slot, c, io)); break;
    case EncodeFamily::small16: case EncodeFamily::smallk: PQCHK(launch_small(cb, slot, p, c, io)); break;
    case EncodeFamily::mfma: PQCHK(launch_mfma(cb, slot, p, c, io)); break;
    case EncodeFamily::anchor: PQCHK(launch_anchor(cb, slot, c, io)); break;
    default: return no_instantiation("(no encode kernel planned)");
    }
    HIPCHK(hipGetLastError());
    if (p.family != EncodeFamily::wide && p.family != EncodeFamily::grouped) note_kernel(p.kernel);   // (launch_keyed: chunk by chunk)
    cb->last_kernel = p.kernel;
    return PQHIP_OK;
}

int32_t encode_plain_dev(pqhip_codebook* cb, int slot, const float* d_x, int64_t n, int64_t x_rs,
                         void* d_codes, int code_bytes, int64_t o_rs, hipStream_t st,
                         const int* bad_flag, bool beside_update)
{
    if (n == 0) return PQHIP_OK;
    const EncodeIo io{d_x, x_rs, d_codes, o_rs, st, bad_flag};
    EncodeCall c = encode_call(cb, slot, io, n, code_bytes);
    c.beside_update = beside_update;
    return encode_planned(cb, slot, plan_encode(*cb, c, cb->ctx->opt), c, io);
}

}  // namespace pqh
