// pqhip_adc_packed4.hip -- 4-bit packed codes (include/pqhip.h: pqhip_pack_codes4_dev, pqhip_unpack_codes4_dev and the
// six pqhip_adc_*search*_packed4_f32_dev).  The unit holds the entry points, the policy of the packed searches -- the
// choices of adc_search / adc_search_lists of pqhip_adc.hip restated for packed rows: queries per pass, list length,
// grid, scratch, the plan and the merge, which it reaches through adc_search_launch.h -- and the instantiations of the
// exhaustive producers and of the pack / unpack kernels (kernels_adc_packed4.hip.h).  The list producers are
// instantiated in pqhip_adc_packed4_lists.hip.  Nothing in pqhip_adc.hip refers to this unit.
#include "adc_search_launch.h"

#define PQHIP_ADC_TEMPLATES_ONLY   // kernels_adc.hip.h: its non-template kernels belong to pqhip_adc.hip
#include "kernels_adc_packed4.hip.h"

using namespace pqhip;

namespace pqh {

// Packed dwords fetched per row: ceil(PB / 4) rounded up to an instantiated width (a wider window only reads past the
// row inside the matrix; adc_fetch_row takes byte loads at its ends).  M <= 100: at most 13.
static int packed4_nv_bucket(int nv)
{
    for (int b : {1, 2, 4, 8, kPacked4MaxValueWords})
        if (nv <= b) return b;
    return 0;
}

static int packed4_lists_nv_bucket(int nv)
{
    for (int b : {2, 8, kPacked4MaxValueWords})
        if (nv <= b) return b;
    return 0;
}

template <bool IP, int NV, int NQ, int L>
int32_t launch_search_p4(const SearchLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    if constexpr (NQ * L > 16) {
        return PQHIP_EUNSUPPORTED;
    } else {
        HIPCHK(hipFuncSetAttribute((const void*)k_adc_search_p4<IP, NV, NQ, L>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((k_adc_search_p4<IP, NV, NQ, L>), dim3(a.grid), dim3(1024), lds, a.st, packed, a.n, a.c_rs, a.allow, lut,
                           a.scales, a.M, a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
        if (IP) note_kernel(NQ == 8 ? "k_adc_ip_search_p4_mq<8 queries>" : NQ == 4 ? "k_adc_ip_search_p4_mq<4 queries>" : "k_adc_ip_search_p4");
        else note_kernel(NQ == 8 ? "k_adc_search_p4_mq<8 queries>" : NQ == 4 ? "k_adc_search_p4_mq<4 queries>" : "k_adc_search_p4");
        return PQHIP_OK;
    }
}

template <bool IP, int NQ, int L>
int32_t launch_search_p4_nv(int nvb, const SearchLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    switch (nvb) {
    case 1: return launch_search_p4<IP, 1, NQ, L>(a, packed, lut, lds);
    case 2: return launch_search_p4<IP, 2, NQ, L>(a, packed, lut, lds);
    case 4: return launch_search_p4<IP, 4, NQ, L>(a, packed, lut, lds);
    case 8: return launch_search_p4<IP, 8, NQ, L>(a, packed, lut, lds);
    case kPacked4MaxValueWords: return launch_search_p4<IP, kPacked4MaxValueWords, NQ, L>(a, packed, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

template <bool IP, int NQ>
int32_t launch_search_p4_l(int L, int nvb, const SearchLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    switch (L) {
    case 1: return launch_search_p4_nv<IP, NQ, 1>(nvb, a, packed, lut, lds);
    case 2: return launch_search_p4_nv<IP, NQ, 2>(nvb, a, packed, lut, lds);
    case 4: return launch_search_p4_nv<IP, NQ, 4>(nvb, a, packed, lut, lds);
    case 8: return launch_search_p4_nv<IP, NQ, 8>(nvb, a, packed, lut, lds);
    case 16: return launch_search_p4_nv<IP, NQ, 16>(nvb, a, packed, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

template <bool IP>
int32_t launch_search_p4_q(int nqp, int L, int nvb, const SearchLaunch& a, const uint8_t* packed, const float* lut, size_t lds)
{
    switch (nqp) {
    case 8: return launch_search_p4_l<IP, 8>(L, nvb, a, packed, lut, lds);
    case 4: return launch_search_p4_l<IP, 4>(L, nvb, a, packed, lut, lds);
    case 1: return launch_search_p4_l<IP, 1>(L, nvb, a, packed, lut, lds);
    default: return PQHIP_EUNSUPPORTED;
    }
}

// The exhaustive packed searches: adc_search's policy on its u8 route.  The table image in LDS is M x 16 entries per
// query whatever K is (kernels_adc_packed4.hip.h), which is what the queries per pass are chosen from.
static int32_t adc_search_packed4(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const uint8_t* d_packed,
                                  int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales, int32_t k, float* d_val,
                                  int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!cb || nq < 0 || n < 0 || k < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16 || cb->M > 100 || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_val || !d_idx || (n > 0 && (!d_tables || !d_packed))) return PQHIP_EINVAL;
    const int M = (int)cb->M, K = (int)cb->K, PB = (M + 1) / 2;
    if ((n > 0 && c_rs < PB) || v_rs < k || i_rs < k) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const int L = search_list_regs(k);
    if (n == 0) {      // padding only
        for (int64_t q = 0; q < nq; q += 65535) {
            const int nqp = (int)std::min<int64_t>(nq - q, 65535);
            PQCHK(adc_search_merge(ip, L, nqp, 0, k, nullptr, nullptr, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
            HIPCHK(hipGetLastError());
        }
        return PQHIP_OK;
    }
    ErrFlag ef(cb, slot, st);
    const size_t table = (size_t)M * 16 * sizeof(float);
    const int nvb = packed4_nv_bucket((PB + 3) / 4);
    const bool mq_on = cb->ctx->opt.adc_single_query.load(std::memory_order_relaxed) == 0;
    int nqp_first = 1;
    if (mq_on) {
        for (int c : {8, 4}) {
            if (c * L <= 16 && search_lds(table * c, c, L) <= 160 * 1024 && nq >= c) { nqp_first = c; break; }
        }
    }
    // one 1,024-thread workgroup per CU over a contiguous row range, at least 4,096 rows each; option "adc_packed4_wgs"
    // forces the number of workgroups (rows per workgroup stay a multiple of 1,024: a wave's rows share two mask words)
    const int64_t forced = cb->ctx->opt.adc_packed4_wgs.load(std::memory_order_relaxed);
    const int64_t wgs = forced > 0 ? std::min<int64_t>(forced, 65536) : cb->ctx->devs[slot]->n_cus;
    int64_t rows_per_wg = round_up((n + wgs - 1) / wgs, 1024);
    if (forced <= 0) rows_per_wg = std::max<int64_t>(rows_per_wg, 4096);
    rows_per_wg = std::min<int64_t>(rows_per_wg, (int64_t)1 << 30);
    const int64_t grid = (n + rows_per_wg - 1) / rows_per_wg;
    const size_t list_entries = (size_t)nqp_first * grid * 64 * L;
    ScratchLease part(cb, slot, st);
    PQCHK(part.acquire(list_entries * (sizeof(unsigned) + sizeof(uint64_t))));
    uint64_t* part_i = (uint64_t*)part.ptr();
    unsigned* part_k = (unsigned*)(part_i + list_entries);
    SearchLaunch a{n, c_rs, rows_per_wg, (unsigned)grid, M, K, k, ip ? d_scales : nullptr, part_k, part_i, ef.flag, st, d_allow};
    int64_t q = 0;
    for (int nqp : {8, 4, 1}) {
        if (nqp > nqp_first) continue;
        if (nqp == 4 && !(mq_on && 4 * L <= 16 && search_lds(table * 4, 4, L) <= 160 * 1024)) continue;
        for (; q + nqp <= nq; q += nqp) {
            const float* lut = d_tables + q * (int64_t)M * K;
            const size_t lds = search_lds(table * nqp, nqp, L);
            if (ip) PQCHK(launch_search_p4_q<true>(nqp, L, nvb, a, d_packed, lut, lds));
            else PQCHK(launch_search_p4_q<false>(nqp, L, nvb, a, d_packed, lut, lds));
            HIPCHK(hipGetLastError());
            PQCHK(adc_search_merge(ip, L, nqp, (int)grid, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
            HIPCHK(hipGetLastError());
        }
    }
    return PQHIP_OK;
}

// The packed list searches: adc_search_lists' checks, plan, chunking and merge around the packed producer.
// res != null: the residual searches; d_scales then holds the row terms of the distance search (required).
static int32_t adc_search_lists_packed4(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                        const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                        const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                        int64_t p_rs, const float* d_scales, int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx,
                                        int64_t i_rs, void* stream, const ListsResidual* res)
{
    if (!cb || nq < 0 || n < 0 || k < 1 || n_lists < 0 || n_probe < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16 || cb->M > 100 || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, K = (int)cb->K, PB = (M + 1) / 2;
    const int L = search_list_regs(k);
    if (n > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;                          // positions are offered as 32-bit values
    const size_t plan_q = ((size_t)n_probe * 2 + 1) * sizeof(int64_t);
    if (plan_q > kListsScratchBytes / 2) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_val || !d_idx || !d_list_off || !d_probes || (n > 0 && (!d_tables || !d_packed))) return PQHIP_EINVAL;
    if (res && (!res->bias || (!ip && !d_scales))) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < PB) || v_rs < k || i_rs < k || p_rs < n_probe) return PQHIP_ESHAPE;
    if (res && res->b_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_lists == 0) {      // padding only
        for (int64_t q = 0; q < nq; q += 65535) {
            const int nqp = (int)std::min<int64_t>(nq - q, 65535);
            PQCHK(adc_search_merge(ip, L, nqp, 0, k, nullptr, nullptr, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
            HIPCHK(hipGetLastError());
        }
        return PQHIP_OK;
    }
    ErrFlag ef(cb, slot, st);
    const size_t table = (size_t)M * 16 * sizeof(float);
    const int nvb = packed4_lists_nv_bucket((PB + 3) / 4);
    const int64_t forced = cb->ctx->opt.adc_lists_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : lists_wgs_per_query(n, n_lists, n_probe, std::min<int64_t>(nq, 65535), cb->ctx->devs[slot]->n_cus);
    const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / (plan_q + lists_q))}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * (plan_q + lists_q)));
    // 8-byte items first: part_i [chunk][G][64 L], seg_begin [chunk][n_probe], seg_cum [chunk][n_probe + 1]; then the keys
    uint64_t* part_i = (uint64_t*)lease.ptr();
    int64_t* seg_begin = (int64_t*)(part_i + (size_t)chunk * G * 64 * L);
    int64_t* seg_cum = seg_begin + (size_t)chunk * n_probe;
    unsigned* part_k = (unsigned*)(seg_cum + (size_t)chunk * ((size_t)n_probe + 1));
    const size_t lds = search_lds(table, 1, L);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        PQCHK(launch_lists_plan(d_list_off, n_lists, d_probes + q * p_rs, (int)n_probe, p_rs, n, seg_begin, seg_cum, nqc, ef.flag, st));
        ListsLaunch a{n, c_rs, (unsigned)G, nqc, M, K, k, (int)n_probe, (ip || res) ? d_scales : nullptr,
                      res ? res->bias + q * res->b_rs : nullptr, res ? res->b_rs : 0, seg_begin, seg_cum, part_k, part_i, ef.flag, st,
                      d_allow};
        PQCHK(launch_lists_packed4(ip, L, nvb, a, d_packed, d_tables + q * (int64_t)M * K, lds));
        HIPCHK(hipGetLastError());
        PQCHK(adc_search_merge(ip, L, (int)nqc, (int)G, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
        HIPCHK(hipGetLastError());
    }
    return PQHIP_OK;
}

// one lane per aligned dword of the span [p, p + bytes)
static int64_t span_blocks(const void* p, int64_t bytes)
{
    const int64_t dwords = (bytes + (int64_t)((uintptr_t)p & 3) + 3) / 4;
    return (dwords + 255) / 256;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_pack_codes4_dev(pqhip_codebook* cb, int32_t slot, const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                              uint8_t* d_packed, int64_t p_rs, void* stream)
{
    if (!cb || n < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16 || (code_bytes != 1 && code_bytes != 4)) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, PB = (M + 1) / 2;
    if (n > 0 && p_rs >= PB && (n - 1) > (((int64_t)1 << 39) - PB) / p_rs) return PQHIP_EUNSUPPORTED;
    if (n == 0) return PQHIP_OK;
    if (!d_codes || !d_packed) return PQHIP_EINVAL;
    if (c_rs < M || p_rs < PB) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const unsigned blocks = (unsigned)span_blocks(d_packed, (n - 1) * p_rs + PB);
    if (code_bytes == 1)
        hipLaunchKernelGGL(k_pack_codes4<uint8_t>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)d_codes, n, c_rs, M, (int)cb->K,
                           d_packed, p_rs, ef.flag);
    else
        hipLaunchKernelGGL(k_pack_codes4<uint32_t>, dim3(blocks), dim3(256), 0, st, (const uint32_t*)d_codes, n, c_rs, M, (int)cb->K,
                           d_packed, p_rs, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_pack_codes4");
    return PQHIP_OK;
}

int32_t pqhip_unpack_codes4_dev(pqhip_codebook* cb, int32_t slot, const uint8_t* d_packed, int64_t n, int64_t p_rs,
                                const int64_t* d_rows, int64_t n_rows, uint8_t* d_out, int64_t o_rs, void* stream)
{
    if (!cb || n < 0 || (d_rows && n_rows < 0)) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (cb->K > 16) return PQHIP_EUNSUPPORTED;
    const int M = (int)cb->M, PB = (M + 1) / 2;
    const int64_t n_out = d_rows ? n_rows : n;
    if (n_out > 0 && o_rs >= M && (n_out - 1) > (((int64_t)1 << 39) - M) / o_rs) return PQHIP_EUNSUPPORTED;
    if (n_out == 0) return PQHIP_OK;
    if (!d_out || (n > 0 && !d_packed)) return PQHIP_EINVAL;
    if (o_rs < M || (n > 0 && p_rs < PB)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    const unsigned blocks = (unsigned)span_blocks(d_out, (n_out - 1) * o_rs + M);
    hipLaunchKernelGGL(k_unpack_codes4, dim3(blocks), dim3(256), 0, st, d_packed, n, p_rs, d_rows, n_out, M, d_out, o_rs, ef.flag);
    HIPCHK(hipGetLastError());
    note_kernel("k_unpack_codes4");
    return PQHIP_OK;
}

int32_t pqhip_adc_search_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const uint8_t* d_packed,
                                         int64_t n, int64_t c_rs, const uint32_t* d_allow, int32_t k, float* d_dist, int64_t d_rs,
                                         int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_ip_search_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                            const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                            const float* d_scales, int32_t k, float* d_score, int64_t s_rs, int64_t* d_idx,
                                            int64_t i_rs, void* stream)
{
    return adc_search_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_search_lists_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                               const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                               const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                               int64_t p_rs, int32_t k, float* d_dist, int64_t d_rs, int64_t* d_idx, int64_t i_rs,
                                               void* stream)
{
    return adc_search_lists_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream, nullptr);
}

int32_t pqhip_adc_ip_search_lists_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                  const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                  const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                  int32_t n_probe, int64_t p_rs, const float* d_scales, int32_t k, float* d_score,
                                                  int64_t s_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_lists_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, nullptr);
}

int32_t pqhip_adc_search_lists_residual_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                        const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                        const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                        int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                        const float* d_row_terms, int32_t k, float* d_dist, int64_t d_rs,
                                                        int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_packed4(false, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_row_terms, k, d_dist, d_rs, d_idx, i_rs, stream, &res);
}

int32_t pqhip_adc_ip_search_lists_residual_packed4_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                           const uint8_t* d_packed, int64_t n, int64_t c_rs, const uint32_t* d_allow,
                                                           const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                           int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                           const float* d_scales, int32_t k, float* d_score, int64_t s_rs,
                                                           int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists_packed4(true, cb, slot, d_tables, nq, d_packed, n, c_rs, d_allow, d_list_off, n_lists, d_probes, n_probe,
                                    p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, &res);
}

}  // extern "C"
