// pqhip_adc_among.hip -- ADC search among given rows (include/pqhip.h: pqhip_adc_among_f32_dev,
// pqhip_adc_ip_among_f32_dev): the entry points, the host policy and the instantiations of k_adc_among_u8
// (kernels_adc_among.hip.h).  List length, NV bucket, LDS budget and the merge of the partial lists are the list
// searches' (adc_search_launch.h); this unit owns the workgroups per query and the chunking of the queries.  A unit of
// its own so that the build compiles its 80 producers beside the other searches; nothing refers to it.
#define PQHIP_ADC_TEMPLATES_ONLY   // the non-template kernels of the headers below belong to pqhip_adc.hip
#include "adc_search_launch.h"
#include "kernels_adc_among.hip.h"

using namespace pqhip;

namespace pqh {

struct AmongLaunch {
    int64_t n, c_rs;
    unsigned G, nq;          // grid (G, nq)
    int M, K, k;
    const float* extra;      // scales (IP) or row terms (residual distance) or null
    const int64_t *lims, *ids;
    int64_t n_ids;
    const int64_t* row_list; // residual: [n] list of every row, else null
    int64_t n_lists;
    const float* bias;       // residual: bias rows of the launch's queries, else null
    int64_t b_rs;
    unsigned* part_k;
    uint64_t* part_i;
    int* err;
    hipStream_t st;
};

template <bool IP, bool RESIDUAL, int NV, int L>
static int32_t launch_among_u8_t(const AmongLaunch& a, const uint8_t* codes, const float* lut, size_t lds)
{
    static const char* const names[2][2] = {{"k_adc_among_u8", "k_adc_among_residual_u8"},
                                            {"k_adc_ip_among_u8", "k_adc_ip_among_residual_u8"}};
    HIPCHK(hipFuncSetAttribute((const void*)k_adc_among_u8<IP, RESIDUAL, NV, L>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
    hipLaunchKernelGGL((k_adc_among_u8<IP, RESIDUAL, NV, L>), dim3(a.G, a.nq), dim3(1024), lds, a.st, codes, a.n, a.c_rs, lut, a.extra,
                       a.M, a.K, a.k, a.lims, a.ids, a.n_ids, a.part_k, a.part_i, a.err, a.row_list, a.n_lists, a.bias, a.b_rs);
    note_kernel(names[IP][RESIDUAL]);
    return PQHIP_OK;
}

// a.bias != null: the residual producer
static int32_t launch_among_u8(bool ip, int L, int nvb, const AmongLaunch& a, const void* codes, const float* lut, size_t lds)
{
    return dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_int<0, 1>(a.bias != nullptr, [&](auto res_c) {
            return dispatch_list_regs(L, [&](auto l_c) {
                return dispatch_int<4, 8, 13, kAdcMaxValueWords>(nvb, [&](auto nv_c) {
                    return launch_among_u8_t<decltype(ip_c)::value != 0, decltype(res_c)::value != 0, decltype(nv_c)::value,
                                             decltype(l_c)::value>(a, (const uint8_t*)codes, lut, lds);
                });
            });
        });
    });
}

// Workgroups per query.  The host cannot see the lengths of the queries' ranges without a synchronisation, so it takes
// their mean (n_ids with a shared list): at least 4,096 places per workgroup -- below that a workgroup's table load and
// list merge outweigh its rows, the bound of lists_wgs_per_query -- and no more than the CUs the queries of a launch
// leave each other.  The estimate only sets the grid: slices are cut from the clamped range on the device.
static int64_t among_wgs_per_query(int64_t mean_ids, int64_t nq, int n_cus)
{
    const int64_t by_rows = (mean_ids + 4095) / 4096;
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min(by_rows, by_cus));
}

// Both searches.  Checks in the order of the list searches: EINVAL for what no shape excuses, ENODEV, EUNSUPPORTED,
// nq == 0, null pointers and the pairing of the residual inputs, ESHAPE; then the padding-only path, G, the chunking
// and the producer -> merge loop.  d_extra: the scales (ip) or the row terms.
static int32_t adc_among(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                         int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids, int64_t n_ids,
                         const int64_t* d_row_list, int64_t n_lists, const float* d_bias, int64_t b_rs, const float* d_extra, int32_t k,
                         float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (!cb || nq < 0 || n < 0 || n_ids < 0 || n_lists < 0 || k < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    const size_t table = (size_t)cb->M * cb->K * sizeof(float);
    const int nvb = lists_nv_bucket(((int)cb->M + 3) / 4);
    const int L = search_list_regs(k);
    if (nvb == 0 || search_lds(table, 1, L) > 160 * 1024) return PQHIP_EUNSUPPORTED;   // the table must fit LDS beside the queues
    if (n > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;                          // rows are offered as 32-bit values
    if (nq == 0) return PQHIP_OK;
    const bool residual = d_row_list != nullptr;
    if (!d_val || !d_idx || (n_ids > 0 && !d_ids) || (n > 0 && n_ids > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if ((d_row_list != nullptr) != (d_bias != nullptr) || (residual && !ip && !d_extra)) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < cb->M) || v_rs < k || i_rs < k || (residual && b_rs < n_lists)) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || n_ids == 0) return adc_search_merge(ip, L, nq, 0, k, nullptr, nullptr, d_val, v_rs, d_idx, i_rs, st);
    ErrFlag ef(cb, slot, st);
    const int64_t forced = cb->ctx->opt.adc_among_wgs_per_query.load(std::memory_order_relaxed);
    const int64_t G = forced > 0 ? std::min<int64_t>(forced, 4096)
                                 : among_wgs_per_query(d_lims ? n_ids / nq : n_ids, std::min<int64_t>(nq, 65535),
                                                       cb->ctx->devs[slot]->n_cus);
    const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, (int64_t)(kListsScratchBytes / lists_q)}));
    ScratchLease lease(cb, slot, st);
    PQCHK(lease.acquire((size_t)chunk * lists_q));
    uint64_t* part_i = (uint64_t*)lease.ptr();                                         // [chunk][G][64 L], then the keys
    unsigned* part_k = (unsigned*)(part_i + (size_t)chunk * G * 64 * L);
    const int M = (int)cb->M, K = (int)cb->K;
    const size_t lds = search_lds(table, 1, L);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        const AmongLaunch a{n, c_rs, (unsigned)G, nqc, M, K, k, (ip || residual) ? d_extra : nullptr, d_lims ? d_lims + q : nullptr,
                            d_ids, n_ids, d_row_list, n_lists, residual ? d_bias + q * b_rs : nullptr, residual ? b_rs : 0, part_k,
                            part_i, ef.flag, st};
        PQCHK(launch_among_u8(ip, L, nvb, a, d_codes, d_tables + q * (int64_t)M * K, lds));
        HIPCHK(hipGetLastError());
        PQCHK(adc_search_merge(ip, L, nqc, (int)G, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
    }
    return PQHIP_OK;
}

}  // namespace pqh

using namespace pqh;

extern "C" {

int32_t pqhip_adc_among_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids,
                                int64_t n_ids, const int64_t* d_row_list, int64_t n_lists, const float* d_list_bias, int64_t b_rs,
                                const float* d_row_terms, int32_t k, float* d_dist, int64_t d_rs, int64_t* d_idx, int64_t i_rs,
                                void* stream)
{
    return adc_among(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_lims, d_ids, n_ids, d_row_list, n_lists, d_list_bias,
                     b_rs, d_row_terms, k, d_dist, d_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_ip_among_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                   int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_lims, const int64_t* d_ids,
                                   int64_t n_ids, const int64_t* d_row_list, int64_t n_lists, const float* d_list_bias, int64_t b_rs,
                                   const float* d_scales, int32_t k, float* d_score, int64_t s_rs, int64_t* d_idx, int64_t i_rs,
                                   void* stream)
{
    return adc_among(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_lims, d_ids, n_ids, d_row_list, n_lists, d_list_bias,
                     b_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
}

}  // extern "C"
