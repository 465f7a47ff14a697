// pqhip_adc.hip -- asymmetric distance computation over a resident code matrix ("next" row):
// per-query lookup tables (linalg.rs:118-148 applied to the sub-vectors of the query) and the table-sum scans.
#include "adc_search_u8_launch.hip.h"

using namespace pqhip;

namespace pqh {

template <int NV>
int32_t launch_adc_nv(int nv, const uint8_t* codes, int64_t n, int64_t c_rs, const float* lut, int M, int K, float* out,
                      int n_cus, size_t lds, int* err, hipStream_t st)
{
    if constexpr (NV > kAdcMaxValueWords) {
        return PQHIP_EUNSUPPORTED;
    } else {
        if (nv != NV) return launch_adc_nv<NV + 1>(nv, codes, n, c_rs, lut, M, K, out, n_cus, lds, err, st);
        HIPCHK(hipFuncSetAttribute((const void*)k_adc_scan_u8<NV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        // all workgroups resident at once (occupancy API: registers and the LDS table both count), one contiguous
        // row range each -- the table is loaded once per workgroup
        const int adc_wgs = diag().adc_wgs;
        const int64_t max_wgs = (int64_t)n_cus * (adc_wgs ? adc_wgs : resident_wgs((const void*)k_adc_scan_u8<NV>, lds));
        int64_t rows_per_wg = round_up((n + max_wgs - 1) / max_wgs, 256);
        rows_per_wg = std::max<int64_t>(rows_per_wg, 1024);
        const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
        hipLaunchKernelGGL((k_adc_scan_u8<NV>), dim3(grid), dim3(256), lds, st, codes, n, c_rs, lut, M, K, out, rows_per_wg, err);
        note_kernel("k_adc_scan_u8");
        return PQHIP_OK;
    }
}

template <int NV, int NQ>
int32_t launch_adc_mq(int nv, const uint8_t* codes, int64_t n, int64_t c_rs, const float* lut, int M, int K, float* out,
                      int64_t o_rs, int n_cus, size_t lds, int* err, hipStream_t st)
{
    if constexpr (NV > kAdcMaxValueWords) {
        return PQHIP_EUNSUPPORTED;
    } else {
        if (nv != NV) return launch_adc_mq<NV + 1, NQ>(nv, codes, n, c_rs, lut, M, K, out, o_rs, n_cus, lds, err, st);
        HIPCHK(hipFuncSetAttribute((const void*)k_adc_scan_u8_mq<NV, NQ>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        // one 1,024-thread workgroup per CU (the table image fills most of the LDS), one contiguous row range each
        int64_t rows_per_wg = round_up((n + n_cus - 1) / n_cus, 1024);
        rows_per_wg = std::max<int64_t>(rows_per_wg, 4096);
        const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
        hipLaunchKernelGGL((k_adc_scan_u8_mq<NV, NQ>), dim3(grid), dim3(1024), lds, st, codes, n, c_rs, lut, M, K, out, o_rs, rows_per_wg, err);
        note_kernel(NQ == 8 ? "k_adc_scan_u8_mq<8 queries>" : "k_adc_scan_u8_mq<4 queries>");
        return PQHIP_OK;
    }
}

// ---- ADC search (kernels_adc_search.hip.h) ---------------------------------------------------------------------------
// List length: 64 L >= k entries per (wave, query), L in {1, 2, 4, 8, 16}.
int search_list_regs(int k) { int lk = 64; while (lk < k) lk <<= 1; return lk / 64; }

// Code dwords fetched per row on the u8 path: ceil(M / 4) rounded up to one of the instantiated widths (a wider window
// only reads past the row inside the code matrix -- adc_fetch_row falls back to byte loads at its end).
int search_nv_bucket(int nv)
{
    for (int b : {1, 2, 4, 8, 13, kAdcMaxValueWords})
        if (nv <= b) return b;
    return 0;
}

// SearchLaunch, SearchRoute, ListsRoute and the drivers' contract: adc_search_launch.h; the u8 producers' launchers:
// adc_search_u8_launch.hip.h (shared with the masked producers of pqhip_adc_masked.hip)

// the producer's dynamic LDS: max(table image + queues, combine lists)
size_t search_lds(size_t table_bytes, int nq, int L)
{
    const size_t queues = (size_t)kSearchWaves * nq * kSearchQueue * 2 * sizeof(unsigned);
    const size_t comb = (size_t)kSearchWaves * nq * 64 * L * 2 * sizeof(unsigned);
    return std::max(table_bytes + queues, comb);
}

// The generic producer, a SearchProducer for one query per pass: any code width, the table in LDS when it fits there
// beside the queues (names "..._wide"), else read through L2 ("..._any").  It sizes its own LDS from that choice: the
// driver's `lds`, like the queries per pass and the NV bucket, is for the u8 and packed producers and is not used here.
template <typename IdxT>
int32_t launch_search_any(bool ip, int, int L, int, const SearchLaunch& a, const void* codes, const float* lut, size_t)
{
    const bool tab_lds = !diag().adc_any && search_lds((size_t)a.M * a.K * sizeof(float), 1, L) <= 160 * 1024;
    const size_t lds = search_lds(tab_lds ? (size_t)a.M * a.K * sizeof(float) : 0, 1, L);
    const int32_t status = dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_int<0, 1>(tab_lds, [&](auto tab_c) {
            return dispatch_list_regs(L, [&](auto l_c) -> int32_t {
                auto kern = k_adc_search_any<decltype(ip_c)::value != 0, IdxT, decltype(l_c)::value, decltype(tab_c)::value != 0>;
                HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                hipLaunchKernelGGL(kern, dim3(a.grid), dim3(1024), lds, a.st, (const IdxT*)codes, a.n, a.c_rs, lut, a.scales, a.M,
                                   a.K, a.k, a.rows_per_wg, a.part_k, a.part_i, a.err);
                return PQHIP_OK;
            });
        });
    });
    if (status != PQHIP_OK) return status;
    if (ip) note_kernel(tab_lds ? "k_adc_ip_search_wide" : "k_adc_ip_search_any");
    else note_kernel(tab_lds ? "k_adc_search_wide" : "k_adc_search_any");
    return PQHIP_OK;
}

// k_adc_search_merge over the partial lists of nq queries; n_lists == 0 writes the padding only
int32_t launch_search_merge(bool ip, int L, int nq, int n_lists, int k, const unsigned* part_k, const uint64_t* part_i, float* d_val,
                            int64_t v_rs, int64_t* d_idx, int64_t i_rs, hipStream_t st)
{
    const int32_t status = dispatch_int<0, 1>(ip, [&](auto ip_c) {
        return dispatch_list_regs(L, [&](auto l_c) -> int32_t {
            constexpr int LL = decltype(l_c)::value;
            auto kern = k_adc_search_merge<decltype(ip_c)::value != 0, LL>;
            const size_t lds = (size_t)kSearchMergeWaves * 64 * LL * (sizeof(unsigned) + sizeof(uint64_t));
            HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(64 * kSearchMergeWaves), lds, st, part_k, part_i, n_lists, k, d_val, v_rs,
                               d_idx, i_rs);
            return PQHIP_OK;
        });
    });
    if (status != PQHIP_OK) return status;
    note_kernel(ip ? "k_adc_ip_search_merge" : "k_adc_search_merge");
    HIPCHK(hipGetLastError());
    return PQHIP_OK;
}

// no row to search: index -1 and +Inf resp. -Inf for every query
int32_t search_padding_only(bool ip, int L, int64_t nq, int k, float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, hipStream_t st)
{
    for (int64_t q = 0; q < nq; q += 65535) {
        const int nqp = (int)std::min<int64_t>(nq - q, 65535);
        PQCHK(launch_search_merge(ip, L, nqp, 0, k, nullptr, nullptr, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
    }
    return PQHIP_OK;
}

// the door of adc_search_launch.h
int32_t adc_search_merge(bool ip, int L, int64_t nq, int G, int k, const unsigned* part_k, const uint64_t* part_i, float* d_val,
                         int64_t v_rs, int64_t* d_idx, int64_t i_rs, hipStream_t st)
{
    if (G == 0) return search_padding_only(ip, L, nq, k, d_val, v_rs, d_idx, i_rs, st);
    return launch_search_merge(ip, L, (int)nq, G, k, part_k, part_i, d_val, v_rs, d_idx, i_rs, st);
}

// Lookup tables for both searches: the query is rotated first for an OPQ codebook (pq.rs:293), then one thread per
// (q, m, j) writes the squared distance (k_adc_tables) or, IP, the inner product alone (k_adc_ip_tables).
int32_t adc_tables(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs, float* d_tables,
                   void* stream)
{
    if (!cb || nq < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (nq == 0) return PQHIP_OK;
    if (!d_q || !d_tables) return PQHIP_EINVAL;
    if (q_rs < cb->d) return PQHIP_ESHAPE;
    if (nq > (1 << 20)) return PQHIP_EUNSUPPORTED;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    CodebookDev& cd = cb->dev[slot];
    const float* y = d_q;
    int64_t y_rs = q_rs;
    ScratchLease rot(cb, slot, st);
    if (cb->has_proj) {       // pq.rs:293: the query is rotated like a vector to be quantized
        PQCHK(rot.acquire((size_t)nq * cb->d * sizeof(float)));
        const int64_t total = nq * cb->d;
        hipLaunchKernelGGL(k_adc_rotate_queries, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_q, q_rs,
                           (int)nq, cd.P, (int)cb->d, (float*)rot.ptr());
        note_kernel("k_adc_rotate_queries");
        y = (const float*)rot.ptr();
        y_rs = cb->d;
    }
    const int64_t total = nq * cb->M * cb->K;
    if (ip) {
        hipLaunchKernelGGL(k_adc_ip_tables, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, y_rs, (int)nq, cd.cb,
                           (int)cb->M, (int)cb->K, (int)cb->dsub, d_tables);
    } else {
        hipLaunchKernelGGL(k_adc_tables, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, y_rs, (int)nq, cd.cb,
                           cd.cc, (int)cb->M, (int)cb->K, (int)cb->dsub, cb->k_pad, d_tables);
    }
    HIPCHK(hipGetLastError());
    note_kernel(ip ? "k_adc_ip_tables" : "k_adc_tables");
    return PQHIP_OK;
}

// The fused scan + exact top-k of every exhaustive search, one policy: the checks that follow the caller's, queries per
// pass (NQ L <= 16 and the 160 KB of LDS, option "adc_single_query"), the partial lists in the codebook's scratch, one
// merge per pass.  ip: similarity (d_scales may be null); else distance.
int32_t adc_search_run(bool ip, pqhip_codebook* cb, int32_t slot, const SearchRoute& r, const float* d_tables, int64_t nq,
                       const void* d_codes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const float* d_scales, int32_t k,
                       float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    if (nq == 0) return PQHIP_OK;
    if (!d_val || !d_idx || (n > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < r.row_len) || v_rs < k || i_rs < k) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const int L = search_list_regs(k);
    if (n == 0) return search_padding_only(ip, L, nq, k, d_val, v_rs, d_idx, i_rs, st);
    ErrFlag ef(cb, slot, st);
    const int M = (int)cb->M, K = (int)cb->K;
    const size_t table = r.table_bytes;
    // Queries per pass: every query of a pass keeps a list of 64 L entries (2 L VGPRs) per wave, so NQ L <= 16 (at most
    // 32 list VGPRs beside the row sum; 1,024-thread workgroups leave 128 VGPRs per lane): 8 queries up to k = 128, 4 up
    // to k = 256, one beyond -- and only while NQ table images plus the queues fit the 160 KB of LDS.
    // Option "adc_single_query" = 1 keeps one query per pass, as for the scan.
    const bool mq_on = r.multi_query && cb->ctx->opt.adc_single_query.load(std::memory_order_relaxed) == 0;
    auto pass_fits = [&](int c) { return mq_on && c * L <= 16 && search_lds(table * c, c, L) <= 160 * 1024; };
    int nqp_first = 1;
    for (int c : {8, 4}) {
        if (pass_fits(c) && nq >= c) { nqp_first = c; break; }
    }
    // one 1,024-thread workgroup per CU, a contiguous row range each (offsets within it are 32-bit: < 2^31 rows) of at
    // least 4,096 rows; a forced number of workgroups keeps the rows per workgroup a multiple of 1,024 (a wave's rows
    // share two mask words)
    const int64_t wgs = r.forced_wgs > 0 ? std::min<int64_t>(r.forced_wgs, 65536) : cb->ctx->devs[slot]->n_cus;
    int64_t rows_per_wg = round_up((n + wgs - 1) / wgs, 1024);
    if (r.forced_wgs <= 0) rows_per_wg = std::max<int64_t>(rows_per_wg, 4096);
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
        if (nqp == 4 && !pass_fits(4)) continue;
        for (; q + nqp <= nq; q += nqp) {
            PQCHK(r.launch(ip, nqp, L, r.nvb, a, d_codes, d_tables + q * (int64_t)M * K, search_lds(table * nqp, nqp, L)));
            HIPCHK(hipGetLastError());
            PQCHK(launch_search_merge(ip, L, nqp, (int)grid, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
        }
    }
    return PQHIP_OK;
}

// The exhaustive searches over u8 / 32-bit codes: the u8 producer when the codes are bytes and the table fits LDS beside
// the queues, else the generic kernel.  mask != null: the masked producer in the place of the u8 one; a call that the
// u8 route does not serve (4-byte codes, a table beyond LDS) is PQHIP_EUNSUPPORTED -- never another path.
// Option "adc_search_wgs" forces the number of producer workgroups, whichever producer runs.
int32_t adc_search(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes, int32_t code_bytes,
                   int64_t n, int64_t c_rs, const float* d_scales, int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx,
                   int64_t i_rs, void* stream, const RowMask* mask = nullptr)
{
    if (!cb || nq < 0 || n < 0 || k < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if ((code_bytes != 1 && code_bytes != 4) || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    const size_t table = (size_t)cb->M * cb->K * sizeof(float);
    const int nvb = search_nv_bucket(((int)cb->M + 3) / 4);
    const bool fast = code_bytes == 1 && nvb != 0 && search_lds(table, 1, search_list_regs(k)) <= 160 * 1024;
    if (mask && !fast) return PQHIP_EUNSUPPORTED;                   // a mask: the u8 route or nothing
    const SearchProducer producer = mask ? mask->search : fast ? launch_search_u8<false>
                                    : code_bytes == 1 ? launch_search_any<uint8_t> : launch_search_any<uint32_t>;
    const SearchRoute r{cb->M, table, nvb, fast, cb->ctx->opt.adc_search_wgs.load(std::memory_order_relaxed), producer};
    return adc_search_run(ip, cb, slot, r, d_tables, nq, d_codes, n, c_rs, mask ? mask->words : nullptr, d_scales, k, d_val, v_rs, d_idx,
                          i_rs, stream);
}

// ---- ADC search over probed lists (kernels_adc_search_lists.hip.h) ----------------------------------------------------
// ListsLaunch: adc_search_launch.h

// Code dwords per row of the list producers: fewer widths than search_nv_bucket (a wider window is always correct)
int lists_nv_bucket(int nv)
{
    for (int b : {4, 8, 13, kAdcMaxValueWords})
        if (nv <= b) return b;
    return 0;
}

// Workgroups per query, from what the host knows: the expected number of probed rows (lists of average size) in units
// of 4,096 rows -- below that a workgroup's table load and list merge outweigh its rows, the bound of the exhaustive
// search -- and no more than the CUs the queries of a launch leave each other (one 1,024-thread workgroup per CU).
int64_t lists_wgs_per_query(int64_t n, int64_t n_lists, int64_t n_probe, int64_t nq, int n_cus)
{
    const double frac = (double)std::min(n_probe, n_lists) / (double)n_lists;
    const int64_t expected = (int64_t)((double)n * frac) + 1;
    const int64_t by_rows = (expected + 4095) / 4096;
    const int64_t by_cus = std::max<int64_t>(1, n_cus / std::max<int64_t>(nq, 1));
    return std::max<int64_t>(1, std::min(by_rows, by_cus));
}

// kListsScratchBytes (plan + partial lists of one chunk of queries): adc_search_launch.h

int32_t launch_lists_plan(const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int n_probe, int64_t p_rs, int64_t n,
                          int64_t* seg_begin, int64_t* seg_cum, unsigned nq, int* err, hipStream_t st)
{
    hipLaunchKernelGGL(k_adc_lists_plan, dim3(nq), dim3(1024), 0, st, d_list_off, n_lists, d_probes, n_probe, p_rs, n, seg_begin,
                       seg_cum, err);
    HIPCHK(hipGetLastError());
    note_kernel("k_adc_lists_plan");
    return PQHIP_OK;
}

// ListsResidual (probe bias rows; the row terms travel in the place of the scales): adc_search_launch.h

// All list searches: the checks that follow the caller's in the order of adc_search_run, the plan kernel (the only
// reader of the offsets and probes), the producer over a (G, queries) grid and one merge, per chunk of queries that fits
// the scratch lease.
int32_t adc_search_lists_run(bool ip, pqhip_codebook* cb, int32_t slot, const ListsRoute& r, const float* d_tables, int64_t nq,
                             const void* d_codes, int64_t n, int64_t c_rs, const uint32_t* d_allow, const int64_t* d_list_off,
                             int64_t n_lists, const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales,
                             int32_t k, float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream,
                             const ListsResidual* res)
{
    if (n > (int64_t)0xfffffffell) return PQHIP_EUNSUPPORTED;                          // positions are offered as 32-bit values
    const size_t plan_q = ((size_t)n_probe * 2 + 1) * sizeof(int64_t);
    if (plan_q > kListsScratchBytes / 2) return PQHIP_EUNSUPPORTED;
    if (nq == 0) return PQHIP_OK;
    if (!d_val || !d_idx || !d_list_off || !d_probes || (n > 0 && (!d_tables || !d_codes))) return PQHIP_EINVAL;
    if (res && (!res->bias || (!ip && !d_scales))) return PQHIP_EINVAL;
    if ((n > 0 && c_rs < r.row_len) || v_rs < k || i_rs < k || p_rs < n_probe) return PQHIP_ESHAPE;
    if (res && res->b_rs < n_probe) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)cb->M, K = (int)cb->K, L = search_list_regs(k);
    if (n == 0 || n_lists == 0) return search_padding_only(ip, L, nq, k, d_val, v_rs, d_idx, i_rs, st);
    ErrFlag ef(cb, slot, st);
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
    const size_t lds = search_lds(r.table_bytes, 1, L);
    for (int64_t q = 0; q < nq; q += chunk) {
        const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);
        PQCHK(launch_lists_plan(d_list_off, n_lists, d_probes + q * p_rs, (int)n_probe, p_rs, n, seg_begin, seg_cum, nqc, ef.flag, st));
        ListsLaunch a{n, c_rs, (unsigned)G, nqc, M, K, k, (int)n_probe, (ip || res) ? d_scales : nullptr,
                      res ? res->bias + q * res->b_rs : nullptr, res ? res->b_rs : 0, seg_begin, seg_cum, part_k, part_i, ef.flag, st,
                      d_allow};
        PQCHK(r.launch(ip, L, r.nvb, a, d_codes, d_tables + q * (int64_t)M * K, lds));
        HIPCHK(hipGetLastError());
        PQCHK(launch_search_merge(ip, L, (int)nqc, (int)G, k, part_k, part_i, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st));
    }
    return PQHIP_OK;
}

// The list searches over u8 codes.  mask != null: the masked producers (pqhip_adc_masked.hip) behind the same plan,
// before the same merge.
int32_t adc_search_lists(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                         int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_list_off, int64_t n_lists,
                         const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales, int32_t k, float* d_val,
                         int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream, const ListsResidual* res = nullptr,
                         const RowMask* mask = nullptr)
{
    if (!cb || nq < 0 || n < 0 || k < 1 || n_lists < 0 || n_probe < 1) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 || k > kSearchMaxK) return PQHIP_EUNSUPPORTED;
    const size_t table = (size_t)cb->M * cb->K * sizeof(float);
    const int nvb = lists_nv_bucket(((int)cb->M + 3) / 4);
    if (nvb == 0 || search_lds(table, 1, search_list_regs(k)) > 160 * 1024) return PQHIP_EUNSUPPORTED;   // the table must fit LDS beside the queues
    const ListsRoute r{cb->M, table, nvb, mask ? mask->lists : launch_lists_u8<false>};
    return adc_search_lists_run(ip, cb, slot, r, d_tables, nq, d_codes, n, c_rs, mask ? mask->words : nullptr, d_list_off, n_lists,
                                d_probes, n_probe, p_rs, d_scales, k, d_val, v_rs, d_idx, i_rs, stream, res);
}

// The doors of pqhip_adc_masked.hip into the two routines above
int32_t adc_search_masked(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                          int32_t code_bytes, int64_t n, int64_t c_rs, const float* d_scales, int32_t k, float* d_val, int64_t v_rs,
                          int64_t* d_idx, int64_t i_rs, void* stream, const RowMask& mask)
{
    return adc_search(ip, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_scales, k, d_val, v_rs, d_idx, i_rs, stream, &mask);
}

int32_t adc_search_lists_masked(bool ip, pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_list_off, int64_t n_lists,
                                const int64_t* d_probes, int32_t n_probe, int64_t p_rs, const float* d_scales, int32_t k,
                                float* d_val, int64_t v_rs, int64_t* d_idx, int64_t i_rs, void* stream, const ListsResidual* res,
                                const RowMask& mask)
{
    return adc_search_lists(ip, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe, p_rs,
                            d_scales, k, d_val, v_rs, d_idx, i_rs, stream, res, &mask);
}
}  // namespace pqh

using namespace pqh;

extern "C" {

// ---- "next" row: asymmetric distance computation over a resident code matrix ----------------------
int32_t pqhip_adc_tables_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs,
                                 float* d_tables, void* stream)
{
    return adc_tables(false, cb, slot, d_q, nq, q_rs, d_tables, stream);
}

// similarity search: the inner-product tables (the dp term of the distance tables)
int32_t pqhip_adc_ip_tables_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_q, int64_t nq, int64_t q_rs,
                                    float* d_tables, void* stream)
{
    return adc_tables(true, cb, slot, d_q, nq, q_rs, d_tables, stream);
}

int32_t pqhip_adc_scan_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                               int32_t code_bytes, int64_t n, int64_t c_rs, float* d_out, int64_t o_rs, void* stream)
{
    if (!cb || nq < 0 || n < 0) return PQHIP_EINVAL;
    if (slot < 0 || slot >= (int)cb->dev.size()) return PQHIP_ENODEV;
    if (code_bytes != 1 && code_bytes != 4) return PQHIP_EUNSUPPORTED;
    if (nq == 0 || n == 0) return PQHIP_OK;
    if (!d_tables || !d_codes || !d_out) return PQHIP_EINVAL;
    if (c_rs < cb->M || o_rs < n) return PQHIP_ESHAPE;
    SET_DEVICE(cb->ctx->devs[slot]->ordinal);
    hipStream_t st = (hipStream_t)stream;
    ErrFlag ef(cb, slot, st);
    int* err = ef.flag;
    const int M = (int)cb->M, K = (int)cb->K;
    const size_t lds = (size_t)M * K * sizeof(float);
    const int nv = (M + 3) / 4;
    const bool fast = code_bytes == 1 && lds <= 160 * 1024 && nv <= kAdcMaxValueWords;
    // several queries per pass over the code matrix: 8 (or 4) tables interleaved in LDS when they fit
    // (context option "adc_single_query" = 1: one pass per query, the round-2 form, for A/B)
    const bool mq_on = cb->ctx->opt.adc_single_query.load(std::memory_order_relaxed) == 0;   // option "adc_single_query"
    const bool adc_any = diag().adc_any;   // the generic kernel for 32-bit codes (A/B, diagnostic builds)
    int64_t q = 0;
    if (fast && mq_on) {
        const int n_cus = cb->ctx->devs[slot]->n_cus;
        for (int nqp : {8, 4}) {
            const size_t lds_q = lds * nqp;
            if (lds_q > 160 * 1024) continue;
            for (; q + nqp <= nq; q += nqp) {
                const float* lut = d_tables + q * (int64_t)M * K;
                float* out = d_out + q * o_rs;
                if (nqp == 8) PQCHK((launch_adc_mq<1, 8>(nv, (const uint8_t*)d_codes, n, c_rs, lut, M, K, out, o_rs, n_cus, lds_q, err, st)));
                else PQCHK((launch_adc_mq<1, 4>(nv, (const uint8_t*)d_codes, n, c_rs, lut, M, K, out, o_rs, n_cus, lds_q, err, st)));
                HIPCHK(hipGetLastError());
            }
        }
    }
    for (; q < nq; ++q) {
        const float* lut = d_tables + q * (int64_t)M * K;
        float* out = d_out + q * o_rs;
        if (fast) {
            PQCHK(launch_adc_nv<1>(nv, (const uint8_t*)d_codes, n, c_rs, lut, M, K, out, cb->ctx->devs[slot]->n_cus, lds, err, st));
        } else if (code_bytes == 4 && lds <= 160 * 1024 && !adc_any) {
            // 32-bit codes, table within LDS (K <= 2,048 at M = 15): one 1,024-thread workgroup per CU, contiguous row ranges
            const int n_cus = cb->ctx->devs[slot]->n_cus;
            const int64_t rows_per_wg = round_up((n + n_cus - 1) / n_cus, 1024);
            const unsigned grid = (unsigned)((n + rows_per_wg - 1) / rows_per_wg);
            HIPCHK(hipFuncSetAttribute((const void*)k_adc_scan_wide, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            hipLaunchKernelGGL(k_adc_scan_wide, dim3(grid), dim3(1024), lds, st, (const uint32_t*)d_codes, n, c_rs, lut, M, K, out, rows_per_wg, err);
            note_kernel("k_adc_scan_wide");
        } else {
            const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32);
            if (code_bytes == 1)
                hipLaunchKernelGGL((k_adc_scan_any<uint8_t>), dim3(grid), dim3(256), 0, st, (const uint8_t*)d_codes, n, c_rs, lut, M, K, out, err);
            else
                hipLaunchKernelGGL((k_adc_scan_any<uint32_t>), dim3(grid), dim3(256), 0, st, (const uint32_t*)d_codes, n, c_rs, lut, M, K, out, err);
            note_kernel("k_adc_scan_any");
        }
        HIPCHK(hipGetLastError());
    }
    return PQHIP_OK;
}

int32_t pqhip_adc_search_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                 int32_t code_bytes, int64_t n, int64_t c_rs, int32_t k, float* d_dist, int64_t d_rs,
                                 int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_ip_search_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                    int32_t code_bytes, int64_t n, int64_t c_rs, const float* d_scales, int32_t k,
                                    float* d_score, int64_t s_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_search_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq, const void* d_codes,
                                       int32_t code_bytes, int64_t n, int64_t c_rs, const int64_t* d_list_off, int64_t n_lists,
                                       const int64_t* d_probes, int32_t n_probe, int64_t p_rs, int32_t k, float* d_dist,
                                       int64_t d_rs, int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_lists(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, nullptr, k, d_dist, d_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_ip_search_lists_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                          const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                          const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes, int32_t n_probe,
                                          int64_t p_rs, const float* d_scales, int32_t k, float* d_score, int64_t s_rs,
                                          int64_t* d_idx, int64_t i_rs, void* stream)
{
    return adc_search_lists(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                  p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream);
}

int32_t pqhip_adc_search_lists_residual_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                const float* d_row_terms, int32_t k, float* d_dist, int64_t d_rs,
                                                int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists(false, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                   p_rs, d_row_terms, k, d_dist, d_rs, d_idx, i_rs, stream, &res);
}

int32_t pqhip_adc_ip_search_lists_residual_f32_dev(pqhip_codebook* cb, int32_t slot, const float* d_tables, int64_t nq,
                                                   const void* d_codes, int32_t code_bytes, int64_t n, int64_t c_rs,
                                                   const int64_t* d_list_off, int64_t n_lists, const int64_t* d_probes,
                                                   int32_t n_probe, int64_t p_rs, const float* d_probe_bias, int64_t b_rs,
                                                   const float* d_scales, int32_t k, float* d_score, int64_t s_rs,
                                                   int64_t* d_idx, int64_t i_rs, void* stream)
{
    const ListsResidual res{d_probe_bias, b_rs};
    return adc_search_lists(true, cb, slot, d_tables, nq, d_codes, code_bytes, n, c_rs, d_list_off, n_lists, d_probes, n_probe,
                                  p_rs, d_scales, k, d_score, s_rs, d_idx, i_rs, stream, &res);
}

}  // extern "C"
