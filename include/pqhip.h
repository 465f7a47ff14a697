/*
 * pqhip.h -- C ABI of libpqhip.so: MI355X (gfx950) product-quantizer encode / reconstruct.
 *
 * This is the drop-in boundary for ONE hot path of finalfusion/reductive v0.9.0: the bodies of
 *   QuantizeVector::quantize_batch_into   src/pq/pq.rs:268-283  (-> src/pq/primitives.rs:64-104,
 *                                          src/kmeans.rs:133-159, src/linalg.rs:150-180)
 *   Reconstruct::reconstruct_batch_into   src/pq/pq.rs:309-327  (-> src/pq/primitives.rs:110-173)
 * for A = f32.  The reference has no FFI of its own (it is a pure-Rust crate); the entry points
 * below are exactly what a `extern "C"` block inside `impl QuantizeVector<f32> for Pq<f32>` binds
 * (binding shown in INTEGRATION.md and rust/pqhip_ffi.rs).  Plain pointers and sizes only.
 *
 * Conventions
 *  - every function returns a pqhip_status (0 = OK); nothing throws, nothing aborts;
 *  - strides are in ELEMENTS (ndarray convention), may be any non-negative value for host entry
 *    points; device entry points need unit column stride;
 *  - host pointers are only read/written during the call; handles own their device memory;
 *  - all entry points are re-entrant and may be called concurrently from many threads
 *    (`Pq<f32>` is `Send + Sync`; reference hot path is `&self`);
 *  - results: u8/u16/u32 codes are bit-identical to the CANON-F32 arithmetic declared in
 *    DESIGN.md (first index wins ties, NaN ordered last as ordered-float does); PQ
 *    reconstructions are exact copies of codebook rows; OPQ reconstructions follow the same
 *    chain rule and agree with the reference within 1e-5 relative.
 *  - there is NO CPU fallback in this library: without a usable gfx950 device every compute
 *    entry point returns PQHIP_ENODEV.
 */
#ifndef PQHIP_H
#define PQHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQHIP_VERSION 100 /* 0.1.0 */

typedef enum pqhip_status {
    PQHIP_OK = 0,
    PQHIP_EINVAL = 1,       /* null pointer / negative size / bad argument                     */
    PQHIP_ESHAPE = 2,       /* "Quantizer and vector length mismatch" (primitives.rs:74-78),
                               output-shape asserts (primitives.rs:80-87, 159-167),
                               projection shape (pq.rs:46-55), empty quantizers (pq.rs:39-42)  */
    PQHIP_ECODE_RANGE = 3,  /* a code >= K in reconstruct (reference: ndarray index_axis panic,
                               primitives.rs:146)                                              */
    PQHIP_EINDEX_WIDTH = 4, /* K-1 does not fit the index type (primitives.rs:31-34)           */
    PQHIP_ENODEV = 5,       /* no gfx950 device / device index out of range                    */
    PQHIP_EHIP = 6,         /* a HIP runtime call failed (pqhip_last_hip_error() has the text) */
    PQHIP_ENOMEM = 7,       /* host or device allocation failed                                */
    PQHIP_EUNSUPPORTED = 8  /* valid request this build has no kernel for                      */
} pqhip_status;

typedef struct pqhip_ctx pqhip_ctx;           /* a set of devices + per-device staging/streams */
typedef struct pqhip_codebook pqhip_codebook; /* device-resident image of one `Pq<f32>`         */

int32_t pqhip_version(void);
const char *pqhip_strerror(int32_t status);
/* text of the last failing HIP call on this thread ("" if none) */
const char *pqhip_last_hip_error(void);

/* number of visible HIP devices (0 and PQHIP_ENODEV if none) */
int32_t pqhip_device_count(int32_t *out_count);

/* devices == NULL / n_devices == 0  ->  all visible devices. */
int32_t pqhip_ctx_create(const int32_t *devices, int32_t n_devices, pqhip_ctx **out);
void pqhip_ctx_destroy(pqhip_ctx *ctx);
int32_t pqhip_ctx_n_devices(const pqhip_ctx *ctx);

/*
 * Upload one product quantizer (replaces `Pq::new`, pq.rs:38-61, on the device side).
 *   quantizers : [M][K][dsub] f32, C order          (Pq.quantizers, pq.rs:31)
 *   projection : [d][d] f32 row-major, d = M*dsub, applied as x.dot(P) (pq.rs:276); NULL = plain PQ
 * The codebook is replicated on every device of the ctx (<= 3 MB), no collective involved.
 */
int32_t pqhip_codebook_create(pqhip_ctx *ctx, const float *quantizers, int64_t n_subquantizers,
                              int64_t n_centroids, int64_t sub_dim, const float *projection,
                              pqhip_codebook **out);
void pqhip_codebook_destroy(pqhip_codebook *cb);
int64_t pqhip_codebook_quantized_len(const pqhip_codebook *cb);     /* M      pq.rs:300-302 */
int64_t pqhip_codebook_reconstructed_len(const pqhip_codebook *cb); /* M*dsub pq.rs:345-347 */
int64_t pqhip_codebook_n_centroids(const pqhip_codebook *cb);       /* K      pq.rs:103-105 */
int32_t pqhip_codebook_has_projection(const pqhip_codebook *cb);

/*
 * HOST-buffer entry points: what `Pq::quantize_batch_into` / `reconstruct_batch_into` call.
 * Rows are sharded contiguously over the ctx's devices, streamed through
 * pinned staging buffers, results land in the caller's strided buffer.  code_bytes is
 * sizeof(I) for the Rust index type I: 1 (u8), 2 (u16), 4 (u32) or 8 (usize/u64).
 */
int32_t pqhip_quantize_batch_f32(pqhip_codebook *cb, const float *x, int64_t n_rows,
                                 int64_t x_row_stride, int64_t x_col_stride, void *codes,
                                 int32_t code_bytes, int64_t codes_row_stride,
                                 int64_t codes_col_stride);

int32_t pqhip_reconstruct_batch_f32(pqhip_codebook *cb, const void *codes, int32_t code_bytes,
                                    int64_t n_rows, int64_t codes_row_stride,
                                    int64_t codes_col_stride, float *out, int64_t out_row_stride,
                                    int64_t out_col_stride);

/*
 * DEVICE-resident entry points (inputs/outputs already in the HBM of device `device_slot` of the
 * ctx; unit column stride; row strides in elements).  Asynchronous on `stream` (a hipStream_t
 * passed as void*, NULL = the device's default stream); the caller synchronises.  code_bytes in
 * {1, 2, 4, 8} as for the host entry points (traits.rs:77-88 is generic over the index type): the
 * kernels produce / consume u8 and u32 codes, 2- and 8-byte matrices are converted on the device
 * through a leased scratch matrix (the row-lookup, ADC and k-means entry points take 1- and 4-byte
 * codes only).  Scratch for the OPQ variants is managed inside the codebook handle.
 */
int32_t pqhip_quantize_batch_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_x,
                                     int64_t n_rows, int64_t x_row_stride, void *d_codes,
                                     int32_t code_bytes, int64_t codes_row_stride, void *stream);

int32_t pqhip_reconstruct_batch_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                        const void *d_codes, int32_t code_bytes, int64_t n_rows,
                                        int64_t codes_row_stride, float *d_out,
                                        int64_t out_row_stride, void *stream);

/*
 * "Next" row: the lookup path of a consumer that keeps a quantized
 * matrix resident (finalfusion's quantized embedding storage is the out-of-tree example): row
 * select, `Reconstruct::reconstruct_batch` (src/pq/traits.rs:109-117 -> src/pq/pq.rs:309-327) of the
 * selected code rows, and an optional per-row rescale, fused into one pass over HBM:
 *     out[i][:] = reconstruct(codes[rows[i]][:]) * scales[rows[i]]        (scales == NULL: no rescale)
 * d_codes [n_codes][M] (1- or 4-byte codes, row stride in elements), d_rows [n] int64 and d_scales
 * [n_codes] f32 live in HBM; out [n][d].  With a projection the un-rotation (pq.rs:323-326) runs
 * before the rescale.  A row index outside [0, n_codes) is ndarray's `select` panic: it raises the
 * same asynchronous flag as a code >= K (query with pqhip_check_codes_dev -> PQHIP_ECODE_RANGE).
 * The multiply is one rounded f32 multiply per element, so results equal
 * `reconstruct_batch(codes.select(Axis(0), rows)) * scales.select(rows)` bit for bit.
 */
int32_t pqhip_reconstruct_rows_f32_dev(pqhip_codebook *cb, int32_t device_slot, const void *d_codes,
                                       int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                       const int64_t *d_rows, int64_t n_rows, const float *d_scales,
                                       float *d_out, int64_t out_row_stride, void *stream);

/*
 * The same lookup over INTERLEAVED records: a resident matrix of n_codes records of `record_bytes` bytes, each
 * holding the M codes of a row at offset 0 and its f32 scale at `scale_offset_bytes` (both multiples of 4 bytes;
 * `record_bytes` also a multiple of `code_bytes`).  With 32-byte records at M = 15 (15 code bytes, 1 pad, the scale
 * at offset 16, 12 pad) a lookup touches ONE 128-byte line where the split layout above touches one for the 15-byte
 * code row (12 % of which straddle two) and one for the scale -- the layout `reductive_amd.Pq.interleave_records`
 * builds and `Pq.reconstruct_records_device` consumes.  Semantics and results are those of
 * pqhip_reconstruct_rows_f32_dev with d_scales given.
 */
int32_t pqhip_reconstruct_rows_records_f32_dev(pqhip_codebook *cb, int32_t device_slot, const void *d_records,
                                               int32_t code_bytes, int64_t n_codes, int64_t record_bytes,
                                               int64_t scale_offset_bytes, const int64_t *d_rows, int64_t n_rows,
                                               float *d_out, int64_t out_row_stride, void *stream);

/*
 * "Next" row: asymmetric distance computation -- the scan that follows
 * encode in a PQ pipeline, over a code matrix kept resident in HBM.  Not a function of reductive; it
 * is defined from the reference's own vector-to-matrix distance so that it has an exact meaning:
 *   tables[q][m][j] = y_q[m*dsub .. (m+1)*dsub).squared_euclidean_distance(quantizers[m])[j]
 *                     (src/linalg.rs:118-148 -- the distances `kmeans::cluster_assignment`,
 *                     kmeans.rs:111-126, minimises inside `Pq::quantize_vector`, pq.rs:285-298), with
 *                     y_q = query_q.dot(projection) first for an OPQ quantizer (pq.rs:293);
 *                     hence argmin_j tables[q][m][j] == quantize_vector(query_q)[m];
 *   out[q][i]       = sum over m = 0 .. M-1, in that order, from +0, of tables[q][m][codes[i][m]]
 *                     (f32 adds; the estimate of |query_q - reconstruct(codes[i])|^2 for plain PQ).
 * d_queries [n_queries][q_row_stride] f32 and d_tables [n_queries][M][K] f32 live in HBM; d_codes
 * [n_codes][codes_row_stride] are 1- or 4-byte codes; d_out [n_queries][out_row_stride] f32.
 * A code >= K raises the stream's range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE).
 * Both calls are asynchronous on `stream`.
 */
int32_t pqhip_adc_tables_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_queries,
                                 int64_t n_queries, int64_t q_row_stride, float *d_tables, void *stream);
int32_t pqhip_adc_scan_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                               int64_t n_queries, const void *d_codes, int32_t code_bytes, int64_t n_codes,
                               int64_t codes_row_stride, float *d_out, int64_t out_row_stride, void *stream);

/*
 * ADC search: the k nearest rows of every query, without the [n_queries][n_codes] distance matrix.  For query q,
 * dist_q[i] is exactly what pqhip_adc_scan_f32_dev writes for row i (the same sequential f32 sum over m from +0), and
 * rows are ordered by (key(dist_q[i]), i) ascending: key is the first-minimum order of cluster_assignments
 * (src/kmeans.rs:133-159) -- -0 == +0, all NaNs equal and above +Inf -- and equal distances go to the smaller row
 * index.  Row q of d_dist [n_queries][dist_row_stride] f32 and d_idx [n_queries][idx_row_stride] int64 receives the
 * first min(k, n_codes) rows in that order, sorted, so d_idx[q][0] is the first minimum of the scan's row q; a NaN
 * distance is returned as the canonical quiet NaN.  When k > n_codes, slots n_codes .. k-1 hold index -1 and +Inf.
 * The order is strict, so the selection is exact and the results do not depend on the grid, the row ranges of the
 * workgroups or the number of queries served per pass over the codes.  Indices are local to the code matrix passed
 * in: a caller that shards the codes adds each shard's offset.
 * 1 <= k <= 1024 (k < 1: PQHIP_EINVAL, k > 1024: PQHIP_EUNSUPPORTED); code_bytes 1 or 4; codes_row_stride < M or a
 * row stride of an output < k: PQHIP_ESHAPE.  n_queries == 0 launches nothing; n_codes == 0 writes the padding only.
 * A code >= K reads entry 0 and raises the stream's range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE).
 * Asynchronous on `stream`; per-workgroup partial lists live in the codebook's scratch, the caller allocates only the
 * outputs.
 * Host policy: one producer workgroup per CU with at least 4,096 rows each; option "adc_search_wgs" forces the number of
 * producer workgroups of this call, of pqhip_adc_ip_search_f32_dev and of their _masked forms (rows per workgroup stay a
 * multiple of 1,024).  The results do not depend on it.
 */
int32_t pqhip_adc_search_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                 const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                 int32_t k, float *d_dist, int64_t dist_row_stride,
                                 int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * ADC similarity search: the k rows of largest inner product with every query.
 *   ip_tables[q][m][j] = unrolled_dot(quantizers[m][j], y_q[m*dsub .. (m+1)*dsub)), y_q as for pqhip_adc_tables_f32_dev
 *                        (query_q.dot(projection) first for an OPQ quantizer, the same sequential dot).  This is the dp
 *                        term of the distance table, so bit for bit tables == fl(fl(yy + cc) - fl(ip + ip)); in real
 *                        arithmetic sum_m ip_tables[q][m][codes[i][m]] = <query_q, reconstruct(codes[i])>, OPQ included.
 *   score[q][i]        = fl(s[q][i] * scales[i]), s[q][i] the scan's row sum over the IP tables (sequential f32 over m
 *                        from +0); without d_scales (NULL) the score is s itself.  pqhip_adc_scan_f32_dev over IP
 *                        tables already yields the unscaled scores of every row; no separate entry point is needed.
 * Rows are ordered by (key(-score), i) ascending, key as for pqhip_adc_search_f32_dev: the largest score first, -0 == +0,
 * every NaN after every number (-Inf included), equal scores to the smaller row index; the order is strict, so the
 * result does not depend on the grid or the merge order.  Row q of d_score / d_idx receives the first min(k, n_codes)
 * rows in that order; slots past the last row hold index -1 and -Inf.  A returned score is the row's score bit for bit,
 * except that a zero comes back as +0 and a NaN as the canonical quiet NaN (the key keeps neither distinction).
 * d_scales [n_codes] f32 or NULL.  Limits, status codes and their precedence are those of pqhip_adc_search_f32_dev
 * (EINVAL, ENODEV, EUNSUPPORTED, ESHAPE; 1 <= k <= 1024; code_bytes 1 or 4); n_queries == 0 launches nothing,
 * n_codes == 0 writes the padding only; a code >= K reads entry 0 and raises the stream's range flag.  The table call
 * checks its arguments as pqhip_adc_tables_f32_dev does.  Both calls are asynchronous on `stream`.
 */
int32_t pqhip_adc_ip_tables_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_queries,
                                    int64_t n_queries, int64_t q_row_stride, float *d_tables, void *stream);
int32_t pqhip_adc_ip_search_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                    const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                    const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                    int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * ADC search over a partitioned code matrix (IVFADC without residual encoding): both searches above restricted, per
 * query, to the rows of the lists the query probes.  d_list_off [n_lists + 1] int64: list l is rows
 * [list_off[l], list_off[l + 1]) of d_codes.  d_probes [n_queries][probes_row_stride] int64: the first n_probe entries
 * of row q are list ids; -1 is padding and is skipped; any other value outside [0, n_lists) is skipped and raises the
 * stream's range flag.  A list named twice in one row is a caller error: its rows may be returned twice.
 * S_q = the rows of the lists named by probe row q.  Row q of the outputs receives the first min(k, |S_q|) rows of S_q
 * ordered by (key(dist), position) ascending -- the similarity search: (key(-score), position) -- with dist, score and
 * key exactly as for pqhip_adc_search_f32_dev / pqhip_adc_ip_search_f32_dev and position the row's index in d_codes;
 * index -1 and +Inf (similarity: -Inf) after them.  Returned indices are positions in d_codes; returned values follow
 * the rules of the exhaustive searches (NaN canonical, a similarity zero as +0).
 * Hence: the result equals that of pqhip_adc_search_f32_dev / pqhip_adc_ip_search_f32_dev on the same matrix with
 * every row outside S_q removed, indices mapped back.  The codes are those of the vectors themselves, so approximation
 * comes only from which lists are probed; with every list probed the result is the exhaustive search's.  The order is
 * strict: the result does not depend on the number of workgroups that share a query (chosen on the host from n_codes,
 * n_lists, n_probe, n_queries and the CU count; option "adc_lists_wgs_per_query" forces it).
 * No byte outside the code matrix is read whatever the offsets and probes hold: a range is clamped to [0, n_codes] and
 * an inverted range is empty; both raise the range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE), as does a
 * code >= K, which reads entry 0.
 * Status codes and their precedence as for pqhip_adc_search_f32_dev (EINVAL, ENODEV, EUNSUPPORTED, ESHAPE), plus:
 * n_lists < 0, n_probe < 1, or a null d_list_off / d_probes with n_queries > 0: PQHIP_EINVAL; probes_row_stride <
 * n_probe: PQHIP_ESHAPE; code_bytes != 1, M > 100, a table that does not fit the 160 KB of LDS beside the queues,
 * n_codes > 2^32 - 2 (positions are compared as 32-bit values) or n_probe >= 2^24: PQHIP_EUNSUPPORTED.
 * n_queries == 0 launches nothing; n_codes == 0 or n_lists == 0 writes the padding only.  Asynchronous on `stream`;
 * the per-query segment plan and the partial lists live in the codebook's scratch (queries are processed in chunks
 * that keep them within 512 MB).
 */
int32_t pqhip_adc_search_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                       const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                       const int64_t *d_list_off, int64_t n_lists,
                                       const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                       int32_t k, float *d_dist, int64_t dist_row_stride,
                                       int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                          const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                          const int64_t *d_list_off, int64_t n_lists,
                                          const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                          const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                          int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * ADC search over a partitioned matrix of RESIDUAL codes (IVFADC with residual encoding): row i of list l stores the
 * code of x_i - c_l, c_l the coarse centroid of the list, and cb is the quantizer of those residuals.  With r^_i the
 * reconstruction of the row's code (inverse rotation included for an OPQ quantizer),
 *   |q - c_l - r^_i|^2 = |q - c_l|^2 + (|r^_i|^2 + 2 <c_l, r^_i>) - 2 <q, r^_i>      <q, c_l + r^_i> = <q, c_l> + <q, r^_i>
 * so one table per query serves every list: d_tables are the INNER-PRODUCT tables of the query in both calls
 * (pqhip_adc_ip_tables_f32_dev of the residual quantizer), the first term is the probe bias d_probe_bias
 * [n_queries][bias_row_stride] f32, one value per (query, probe slot), and the middle term is the row term d_row_terms
 * [n_codes] f32, query-free, laid out in row order as the scales are.  The caller computes both; the library does not
 * interpret them.  The values, as definition -- every operation one rounded f32 operation, no contraction; s is the
 * scan's sequential row sum over m from +0 of d_tables[q][m][codes[i][m]], p the probe slot through which row i is
 * reached:
 *   dist  = fl( fl(bias[q][p] + term[i]) - fl(s + s) )          ordered by (key(dist), position)
 *   score = fl( fl(bias[q][p] + s) * scale[i] )                 ordered by (key(-score), position)
 *           without d_scales (NULL): score = fl(bias[q][p] + s)
 * Row q of the outputs receives the first min(k, |S_q|) rows of S_q under that strict order, with S_q, key, position,
 * the canonical NaN, the similarity zero as +0 (a zero distance likewise comes back as +0: the key does not keep its
 * sign), the padding with -1 and +Inf / -Inf, the treatment of -1 probes, bad ids, clamped and inverted ranges and
 * codes >= K, the independence from the number of workgroups per query (option "adc_lists_wgs_per_query"), scratch and
 * query chunking all as pqhip_adc_search_lists_f32_dev / pqhip_adc_ip_search_lists_f32_dev define them.  The bias of a
 * skipped probe (-1, a bad id, an empty or emptied range) is never read into a result.
 * Arguments, checks, status codes and precedence are those of pqhip_adc_ip_search_lists_f32_dev, plus: d_probe_bias ==
 * NULL with n_queries > 0, or d_row_terms == NULL with n_queries > 0 in the distance call: PQHIP_EINVAL;
 * bias_row_stride < n_probe: PQHIP_ESHAPE.
 */
int32_t pqhip_adc_search_lists_residual_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                int64_t n_codes, int64_t codes_row_stride,
                                                const int64_t *d_list_off, int64_t n_lists,
                                                const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                const float *d_probe_bias, int64_t bias_row_stride,
                                                const float *d_row_terms, int32_t k, float *d_dist, int64_t dist_row_stride,
                                                int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_lists_residual_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                   int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                   int64_t n_codes, int64_t codes_row_stride,
                                                   const int64_t *d_list_off, int64_t n_lists,
                                                   const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                   const float *d_probe_bias, int64_t bias_row_stride,
                                                   const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                                   int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * The six searches above restricted to an allowed set of rows (deleted rows, subsets, skip sets): each _masked call is
 * the unmasked signature with a row mask d_allow inserted after codes_row_stride.  d_allow holds ceil(n_codes / 32)
 * 32-bit words in HBM, in the row order of d_codes (position order for a partitioned matrix): bit i & 31 of word i >> 5
 * set means that row i may be returned.  Bits of the last word at or beyond n_codes are ignored, whatever they hold; no
 * byte outside those words is read, and a word is read only for a row that the unmasked call would have read.
 * d_allow == NULL means no filter: the call then IS the unmasked call -- same kernels, same launch log, same results.
 * With A the set of rows whose bit is set, row q of the outputs receives the first min(k, |A|) rows of A (exhaustive
 * calls) resp. the first min(k, |S_q n A|) rows of S_q n A (list calls) in the unmasked call's own strict order.  Hence:
 * the result is what the unmasked call returns on the matrix with every disallowed row removed, indices mapped back --
 * values, keys, the canonical NaN, zeros as +0 and the padding (-1 with +Inf / -Inf) exactly the unmasked call's, bit for
 * bit.  Everything else the unmasked call defines is unchanged: -1 probes, bad ids, clamped and inverted ranges, the
 * independence from the number of workgroups per query, scratch, query chunking, status codes and their precedence.
 * A row whose bit is clear is NOT READ: its codes are not interpreted (a code >= K in it does not raise the range flag)
 * and its scale, row term or bias enters nothing (a NaN there changes nothing).  An all-zero mask writes the padding only.
 * One mask serves all queries of a call.  Per-query masks are out of scope: at n_codes / 8 bytes per query they are a
 * different design.
 * Scope with a non-NULL mask: the exhaustive calls serve 1-byte codes whose table fits the 160 KB of LDS beside the
 * queues and M <= 100 (the route of the 8 / 4 / 1 queries per pass); code_bytes == 4 or a larger table is
 * PQHIP_EUNSUPPORTED (in the place of the k > 1024 check) -- never another path.  The list calls have the scope of the
 * list calls.
 */
int32_t pqhip_adc_search_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                        const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                        const uint32_t *d_allow,
                                        int32_t k, float *d_dist, int64_t dist_row_stride,
                                        int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                           const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                           const uint32_t *d_allow,
                                           const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                           int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_search_lists_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                              int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                              int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                              const int64_t *d_list_off, int64_t n_lists,
                                              const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                              int32_t k, float *d_dist, int64_t dist_row_stride,
                                              int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_lists_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                 int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                 int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                                 const int64_t *d_list_off, int64_t n_lists,
                                                 const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                 const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                                 int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_search_lists_residual_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                       int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                       int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                                       const int64_t *d_list_off, int64_t n_lists,
                                                       const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                       const float *d_probe_bias, int64_t bias_row_stride,
                                                       const float *d_row_terms, int32_t k, float *d_dist,
                                                       int64_t dist_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                                       void *stream);
int32_t pqhip_adc_ip_search_lists_residual_masked_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                          int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                          int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                                          const int64_t *d_list_off, int64_t n_lists,
                                                          const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                          const float *d_probe_bias, int64_t bias_row_stride,
                                                          const float *d_scales, int32_t k, float *d_score,
                                                          int64_t score_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                                          void *stream);

/*
 * Builds the words of a row mask on the device: for p in [0, n), bit p & 31 of d_words[p >> 5] is
 * d_allow_bytes[d_perm ? d_perm[p] : p] != 0; the bits of the last word at or beyond n are written as 0.  d_allow_bytes
 * [n_src] u8, nonzero = allowed; d_perm NULL or [n] int64 (for a partitioned matrix: the original row number of each
 * position); d_words [ceil(n / 32)].  A source index outside [0, n_src) gives bit 0 and raises the stream's range flag
 * (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE).  n < 0, n_src < 0, or a null d_allow_bytes / d_words with n > 0:
 * PQHIP_EINVAL; n > (2^31 - 1) 256 (one launch): PQHIP_EUNSUPPORTED; n == 0 launches nothing.  Asynchronous on `stream`.  A mask is rebuilt from its bytes; there are no
 * in-place bit updates.
 */
int32_t pqhip_pack_row_mask_dev(pqhip_codebook *cb, int32_t device_slot,
                                const uint8_t *d_allow_bytes, int64_t n_src,
                                const int64_t *d_perm, int64_t n,
                                uint32_t *d_words, void *stream);

/*
 * 4-bit packed codes: two codes per byte for quantizers with K <= 16 centroids, and the six top-k searches over them.
 * Format.  A packed row of M codes is PB = ceil(M / 2) bytes.  Code m lives in byte m >> 1: the low nibble holds even m
 * and the high nibble holds odd m.  For odd M the high nibble of the last byte is written as 0 by the packer and IGNORED
 * by every reader: it enters no sum and raises no flag whatever it holds.  Rows are packed_row_stride >= PB bytes apart.
 * No alignment is required of the base pointer or of the stride (M = 5 gives 3-byte rows at odd addresses).  Only
 * quantizers with K <= 16 are served; K need not be 16 or a power of two.  A nibble >= K in a row that is read raises the
 * stream's range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE) and reads entry 0, as a byte code >= K does.
 *
 * pqhip_pack_codes4_dev packs d_codes [n][M] (code_bytes 1 or 4, codes_row_stride in elements) into d_packed.  A code
 * >= K packs as 0 and raises the range flag.  Only the PB bytes of each row are written: bytes between PB and the stride
 * are left alone.
 * pqhip_unpack_codes4_dev writes u8 codes [*][M] (out_row_stride >= M bytes).  d_rows == NULL: all n rows in order
 * (n_rows is ignored).  Else d_rows is int64 [n_rows] and row r of the output is packed row d_rows[r]; a row id outside
 * [0, n) writes a zero row and raises the range flag.  Nibbles are copied as they are (no range check); the pad nibble of
 * an odd M is not emitted.
 * Both: a null cb or a negative count PQHIP_EINVAL; the slot PQHIP_ENODEV; K > 16, code_bytes not 1 or 4, or more than
 * 2^39 output bytes (one launch) PQHIP_EUNSUPPORTED; nothing to write: PQHIP_OK without a launch; then null buffers
 * PQHIP_EINVAL and a stride below the row PQHIP_ESHAPE.  Asynchronous on `stream`.
 *
 * The six searches: each is the _masked search of the same name with (d_packed, n_codes, packed_row_stride) in the place
 * of (d_codes, code_bytes, n_codes, codes_row_stride).  d_allow may be NULL for no filter.  The tables are the ones
 * pqhip_adc_tables_f32_dev / pqhip_adc_ip_tables_f32_dev produce ([n_queries][M][K]).
 * Definition: the result of a packed call equals, bit for bit, values and indices and padding, the result of the corresponding existing entry point on the unpacked u8 codes with the same tables, probes, biases, row terms, scales and mask.
 * The row sum stays the sequential f32 chain over m = 0 .. M-1 from +0, one table entry per code.  Order key, NaN and zero
 * handling, -1 probes, bad ids, clamped and inverted ranges, disallowed rows not being read, the independence from the
 * grid and from the queries per pass, scratch and chunking are all inherited.
 * Status codes, in the precedence of pqhip_adc_search_f32_dev (EINVAL, ENODEV, EUNSUPPORTED, then nq == 0, null buffers,
 * ESHAPE): K > 16, M > 100 (13 packed dwords per row) or k > 1024 is PQHIP_EUNSUPPORTED; packed_row_stride < PB (with
 * n_codes > 0) is PQHIP_ESHAPE; the list calls keep their own limits (n_codes <= 2^32 - 2, n_probe < 2^24).  Anything
 * not served is PQHIP_EUNSUPPORTED, never another path.
 * Host policy: queries per pass (8 / 4 / 1, option "adc_single_query"), list length, grid and workgroups per query
 * (option "adc_lists_wgs_per_query") are chosen as for the u8 searches; option "adc_packed4_wgs" forces the producer
 * workgroups of the exhaustive packed calls.
 */
int32_t pqhip_pack_codes4_dev(pqhip_codebook *cb, int32_t device_slot, const void *d_codes, int32_t code_bytes,
                              int64_t n, int64_t codes_row_stride, uint8_t *d_packed, int64_t packed_row_stride,
                              void *stream);
int32_t pqhip_unpack_codes4_dev(pqhip_codebook *cb, int32_t device_slot, const uint8_t *d_packed, int64_t n,
                                int64_t packed_row_stride, const int64_t *d_rows /* or NULL */, int64_t n_rows,
                                uint8_t *d_codes_out, int64_t out_row_stride, void *stream);
int32_t pqhip_adc_search_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                         const uint8_t *d_packed, int64_t n_codes, int64_t packed_row_stride,
                                         const uint32_t *d_allow,
                                         int32_t k, float *d_dist, int64_t dist_row_stride,
                                         int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                            const uint8_t *d_packed, int64_t n_codes, int64_t packed_row_stride,
                                            const uint32_t *d_allow,
                                            const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                            int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_search_lists_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                               int64_t n_queries, const uint8_t *d_packed,
                                               int64_t n_codes, int64_t packed_row_stride, const uint32_t *d_allow,
                                               const int64_t *d_list_off, int64_t n_lists,
                                               const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                               int32_t k, float *d_dist, int64_t dist_row_stride,
                                               int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_ip_search_lists_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                  int64_t n_queries, const uint8_t *d_packed,
                                                  int64_t n_codes, int64_t packed_row_stride, const uint32_t *d_allow,
                                                  const int64_t *d_list_off, int64_t n_lists,
                                                  const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                  const float *d_scales, int32_t k, float *d_score, int64_t score_row_stride,
                                                  int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_adc_search_lists_residual_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                        int64_t n_queries, const uint8_t *d_packed,
                                                        int64_t n_codes, int64_t packed_row_stride, const uint32_t *d_allow,
                                                        const int64_t *d_list_off, int64_t n_lists,
                                                        const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                        const float *d_probe_bias, int64_t bias_row_stride,
                                                        const float *d_row_terms, int32_t k, float *d_dist,
                                                        int64_t dist_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                                        void *stream);
int32_t pqhip_adc_ip_search_lists_residual_packed4_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                           int64_t n_queries, const uint8_t *d_packed,
                                                           int64_t n_codes, int64_t packed_row_stride, const uint32_t *d_allow,
                                                           const int64_t *d_list_off, int64_t n_lists,
                                                           const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                           const float *d_probe_bias, int64_t bias_row_stride,
                                                           const float *d_scales, int32_t k, float *d_score,
                                                           int64_t score_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                                           void *stream);

/*
 * ADC range search: EVERY row within a radius resp. at or above a similarity, exhaustive and over probed lists, without
 * the [n_queries][n_codes] matrix -- the question beside "the best k".  Everything is exact; there is no tolerance and no
 * k.  Query q has a threshold d_threshold[q] (f32) and a value v[q][i] per row:
 *   pqhip_adc_range_f32_dev        v = what pqhip_adc_scan_f32_dev writes for row i (the sequential f32 sum over m from
 *                                  +0); row i qualifies iff v <= thr[q] as an IEEE comparison: a NaN value never
 *                                  qualifies, a NaN threshold matches nothing, +Inf matches every non-NaN row.
 *   pqhip_adc_ip_range_f32_dev     v = fl(s * scale[i]), s without d_scales, exactly the score of
 *                                  pqhip_adc_ip_search_f32_dev; row i qualifies iff v >= thr[q] (-Inf: every non-NaN row).
 *   pqhip_adc_range_lists_f32_dev / pqhip_adc_ip_range_lists_f32_dev
 *                                  the same two values over S_q, the rows of the probed lists.  Probes, -1 padding, bad
 *                                  ids, clamped and inverted ranges and the range flag are exactly those of
 *                                  pqhip_adc_search_lists_f32_dev (the same plan kernel reads them).
 *   pqhip_adc_range_lists_residual_f32_dev / pqhip_adc_ip_range_lists_residual_f32_dev
 *                                  dist = fl(fl(bias[q][p] + term[i]) - fl(s + s)), score = fl(fl(bias[q][p] + s) *
 *                                  scale[i]) (without d_scales: fl(bias[q][p] + s)), the formulas of
 *                                  pqhip_adc_search_lists_residual_f32_dev over the same inner-product tables.  The bias
 *                                  of a skipped probe is never read into a result.
 * Output is CSR.  d_lims [n_queries + 1] int64: lims[0] = 0 and lims[q + 1] - lims[q] is the number of qualifying rows
 * of query q.  d_val (f32) and d_idx (int64) are flat arrays of `capacity` entries.  Exhaustive calls: the rows of query
 * q occupy slots lims[q] .. lims[q + 1] - 1 in ascending row index.  List calls: they come in the order of the
 * concatenation of the probed lists -- probe slot first, then position; a list named twice returns its rows twice.
 * d_idx holds row indices (positions in d_codes for the list calls); d_val holds the value bit for bit -- nothing is
 * ordered by value, so there is no key: the sign of a zero is kept.  The order is a function of the inputs alone: the
 * result does not depend on the grid, the row ranges, the number of queries per pass or the number of workgroups per
 * query (options "adc_range_wgs", "adc_range_wgs_per_query" force them).
 * Capacity protocol.  d_lims always receives the true counts.  An entry whose global slot is < capacity is written; an
 * entry at or beyond capacity is not, and no byte past `capacity` entries is touched: what was written is a valid prefix
 * of the result.  capacity == 0 is a pure count call (d_val / d_idx may be NULL).  A caller reads lims[n_queries]; if it
 * exceeds the capacity it passed, it allocates that many entries and calls again: the second call always suffices.
 * Row filter.  d_allow is NULL (no filter) or the mask words of pqhip_pack_row_mask_dev, as in the _masked searches: the
 * result is that of the unmasked call on the matrix with every disallowed row removed, indices mapped back.  A row whose
 * bit is clear is NOT READ: a code >= K there raises no flag, a NaN scale, term or bias there changes nothing.
 * Scope: code_bytes == 1, M <= 100 and a table that fits the 160 KB of LDS -- anything else is PQHIP_EUNSUPPORTED, never
 * another path; the list calls also want n_codes <= 2^32 - 2 and n_probe < 2^24.  Status codes in the precedence of
 * pqhip_adc_search_f32_dev (EINVAL, ENODEV, EUNSUPPORTED, ESHAPE): a null cb, a negative count, capacity < 0 (list calls:
 * n_lists < 0, n_probe < 1): PQHIP_EINVAL; then the slot, then the scope; n_queries == 0 launches nothing and writes
 * nothing; then a null d_lims or d_threshold, null outputs with capacity > 0, null tables or codes with n_codes > 0 (list
 * calls: null d_list_off / d_probes; residual: null d_probe_bias, null d_row_terms in the distance call): PQHIP_EINVAL;
 * then codes_row_stride < M, probes_row_stride or bias_row_stride < n_probe: PQHIP_ESHAPE.  n_codes == 0 (list calls: or
 * n_lists == 0) writes all-zero lims.  A code >= K in a row that is read reads entry 0 and raises the stream's range flag.
 * All calls are asynchronous on `stream`; partial counts (and the plan of the list calls) live in the codebook's scratch,
 * and queries are processed in chunks that keep them bounded.  Results are not sorted by value: sort on the caller's side.
 */
int32_t pqhip_adc_range_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                const uint32_t *d_allow,
                                const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val, int64_t *d_idx,
                                int64_t capacity, void *stream);
int32_t pqhip_adc_ip_range_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                   const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                   const uint32_t *d_allow, const float *d_scales,
                                   const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val, int64_t *d_idx,
                                   int64_t capacity, void *stream);
int32_t pqhip_adc_range_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                      const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                      const uint32_t *d_allow, const int64_t *d_list_off, int64_t n_lists,
                                      const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                      const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val,
                                      int64_t *d_idx, int64_t capacity, void *stream);
int32_t pqhip_adc_ip_range_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                         const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                         const uint32_t *d_allow, const int64_t *d_list_off, int64_t n_lists,
                                         const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                         const float *d_scales,
                                         const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val,
                                         int64_t *d_idx, int64_t capacity, void *stream);
int32_t pqhip_adc_range_lists_residual_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                               int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                               int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                               const int64_t *d_list_off, int64_t n_lists,
                                               const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                               const float *d_probe_bias, int64_t bias_row_stride,
                                               const float *d_row_terms,
                                               const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val,
                                               int64_t *d_idx, int64_t capacity, void *stream);
int32_t pqhip_adc_ip_range_lists_residual_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables,
                                                  int64_t n_queries, const void *d_codes, int32_t code_bytes,
                                                  int64_t n_codes, int64_t codes_row_stride, const uint32_t *d_allow,
                                                  const int64_t *d_list_off, int64_t n_lists,
                                                  const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                                  const float *d_probe_bias, int64_t bias_row_stride,
                                                  const float *d_scales,
                                                  const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val,
                                                  int64_t *d_idx, int64_t capacity, void *stream);

/*
 * ADC search among given rows: exact top-k over per-query lists of candidate ids -- "rank exactly these rows".  The
 * searches above decide by themselves which rows they read (all rows, the rows of the probed lists, either under one
 * mask shared by the queries of a call); here the caller names the rows of every query: a tenant's rows, what a range
 * search has just returned (its lims and idx as they are), a graph's neighbour lists, a shortlist from another index,
 * or the allowed rows of a very sparse filter.
 * Candidate set.  C_q is the set of entries of d_ids[lims[q] .. lims[q + 1]) that lie in [0, n_codes); with d_lims ==
 * NULL every query takes d_ids[0 .. n_ids).  -1 is padding and is skipped; any other value outside the range is skipped
 * and raises the stream's range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE).  An id named twice is a caller error
 * and may be returned twice (the wording of pqhip_rerank_f32_dev).  Ids need not be sorted.
 * d_lims is device memory and is not trusted: both ends are clamped to [0, n_ids] and an inverted range is empty; both
 * cases raise the flag.  No byte outside d_ids[0 .. n_ids) is read.
 * Values.  With s the scan's sequential f32 row sum, the value of row i for query q is the list producers', operation
 * for operation.  Plain (d_row_list == d_list_bias == NULL): s, resp. fl(s * scale[i]) (s alone with d_scales == NULL).
 * Residual (both non-NULL): fl(fl(b + term[i]) - fl(s + s)), resp. fl(fl(b + s) * scale[i]), with b =
 * d_list_bias[q][d_row_list[i]]; d_tables are the INNER-PRODUCT tables in both residual calls; d_row_list [n_codes]
 * holds the list of every row and d_list_bias [n_queries][bias_row_stride] one value per (query, list), |q - c_l|^2
 * resp. <q, c_l>.  A d_row_list[i] outside [0, n_lists) on a named row skips the row and raises the flag.
 * Result.  Row q of the outputs receives the first min(k, |C_q|) members of C_q ordered by (key(value), row id), resp.
 * (key(-score), row id); key, the canonical NaN, zero as +0 and the padding (-1 with +Inf / -Inf) are those of
 * pqhip_adc_search_f32_dev / pqhip_adc_ip_search_f32_dev.  The order is strict, so the result does not depend on the
 * order of the ids, the grid or the chunking.  Hence for distinct in-range ids the result equals, bit for bit, that of
 * pqhip_adc_search_masked_f32_dev / pqhip_adc_ip_search_masked_f32_dev with the mask of C_q, run for that query alone,
 * and in the residual form that of pqhip_adc_*search_lists_residual_masked_f32_dev probing every list once with
 * bias[q][p] = d_list_bias[q][probe p] and the same mask.
 * A row that is not named is not read: its codes are not interpreted (a code >= K there raises nothing) and its scale,
 * term and list id enter nothing.  A named row's code >= K reads entry 0 and raises the flag.
 * Status codes follow the precedence of pqhip_adc_search_lists_f32_dev.  PQHIP_EINVAL: cb == NULL, k < 1, a negative
 * count; then PQHIP_ENODEV; then PQHIP_EUNSUPPORTED: code_bytes != 1, more than 100 subquantizers, a table that does not
 * fit LDS beside the queues, k > 1024, n_codes > 2^32 - 2.  n_queries == 0 launches nothing and returns PQHIP_OK.  Then
 * PQHIP_EINVAL: a NULL output, d_ids == NULL with n_ids > 0, NULL tables or codes with rows to read, only one of
 * d_row_list / d_list_bias given, d_row_terms == NULL in the residual distance call; then PQHIP_ESHAPE: codes_row_stride
 * below the row length, an output stride below k, bias_row_stride < n_lists.  n_ids == 0 or n_codes == 0 writes the
 * padding only.  Anything not served is PQHIP_EUNSUPPORTED, never another path.
 * Host policy: the workgroups that share a query are chosen from the mean number of ids per query (n_ids / n_queries,
 * n_ids with d_lims == NULL) -- at least 4,096 places each, bounded by the CU count over the queries of a launch; option
 * "adc_among_wgs_per_query" forces the number.  The partial lists live in the codebook's scratch; queries are processed
 * in chunks that keep them within 512 MB.  One query per workgroup set, also for a shared list.
 */
int32_t pqhip_adc_among_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                const int64_t *d_lims /* [n_queries + 1] or NULL */, const int64_t *d_ids, int64_t n_ids,
                                const int64_t *d_row_list /* [n_codes] or NULL */, int64_t n_lists,
                                const float *d_list_bias /* [n_queries][bias_row_stride] or NULL */, int64_t bias_row_stride,
                                const float *d_row_terms /* [n_codes]; residual form only */,
                                int32_t k, float *d_dist, int64_t dist_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                void *stream);
int32_t pqhip_adc_ip_among_f32_dev(pqhip_codebook *cb, int32_t device_slot, const float *d_tables, int64_t n_queries,
                                   const void *d_codes, int32_t code_bytes, int64_t n_codes, int64_t codes_row_stride,
                                   const int64_t *d_lims /* [n_queries + 1] or NULL */, const int64_t *d_ids, int64_t n_ids,
                                   const int64_t *d_row_list /* [n_codes] or NULL */, int64_t n_lists,
                                   const float *d_list_bias /* [n_queries][bias_row_stride] or NULL */, int64_t bias_row_stride,
                                   const float *d_scales /* [n_codes] or NULL */,
                                   int32_t k, float *d_score, int64_t score_row_stride, int64_t *d_idx, int64_t idx_row_stride,
                                   void *stream);

/*
 * Exact re-ranking of search candidates against resident vectors ("IVFADC+R", refine): the stage after an ADC search
 * that replaces the quantizer's estimate by the distance to the stored vector.  For query q, the first n_cand entries of
 * row q of d_cand [n_queries][cand_row_stride] int64 name rows of d_vectors [n_rows][vec_row_stride], vec_bytes = 4 (f32)
 * or 2 (IEEE f16; an element is converted exactly to f32 and then takes the same arithmetic); d_queries
 * [n_queries][q_row_stride] f32; d is the width of both.  cb supplies the device slot, the scratch and the stream's range
 * flag (pqhip_check_codes_dev), as for the other _dev calls; its quantizer is not read and d need not equal its width.
 * Value of a row x for query q, as definition -- every operation one rounded f32 operation, no contraction:
 *   for l = 0 .. 63 the partial p_l is the sequential chain from +0 over j = l, l + 64, l + 128, .. < d of
 *       squared L2 (metric 0):     p_l <- fl(p_l + fl(t * t)),  t = fl(q_j - x_j)
 *       inner product (metric 1):  p_l <- fl(p_l + fl(q_j * x_j))
 *   then the fixed tree: for s = 32, 16, 8, 4, 2, 1:  p_l <- fl(p_l + p_(l+s)) for every l < s;  the value is p_0.
 * (One wave reads a row with coalesced 256-byte loads, lane l owning chain l, and reduces with a fixed butterfly.)
 * C_q = the entries of candidate row q that lie in [0, n_rows).  -1 is padding and is skipped; any other value outside
 * the range is skipped and raises the stream's range flag (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE); no byte outside
 * d_vectors is read for it.  An id named twice is a caller error and may be returned twice.  Row q of d_val
 * [n_queries][val_row_stride] f32 and d_idx [n_queries][idx_row_stride] int64 receives the first min(k, |C_q|) members
 * of C_q ordered by (key(dist), row id) ascending -- inner product: (key(-score), row id), the largest score first -- key
 * exactly as for pqhip_adc_search_f32_dev (-0 == +0, every NaN equal and after every number, ties to the smaller row
 * id).  A returned value is the row's value bit for bit, except that a NaN comes back as the canonical quiet NaN and a
 * zero as +0.  Slots past the last candidate hold index -1 and +Inf (inner product: -Inf).  The order is strict, so the
 * result does not depend on how candidates are spread over waves and workgroups (chosen on the host from n_cand,
 * n_queries and the CU count; option "rerank_wgs_per_query" forces the workgroups that share a query).
 * Status codes, in the precedence of pqhip_adc_search_f32_dev (EINVAL, ENODEV, EUNSUPPORTED, ESHAPE):
 *   k < 1, n_cand < 1, d < 1, n_queries < 0, n_rows < 0, metric not 0 / 1: PQHIP_EINVAL;
 *   vec_bytes not 2 / 4, k > 1024, n_cand > 1024, d > 16384 (the query is held in 64 KB of LDS), n_rows > 2^32 - 2 (an
 *   entry keeps the row id in 32 bits): PQHIP_EUNSUPPORTED;
 *   with n_queries > 0, a null d_queries, d_cand, d_val or d_idx, or a null d_vectors with n_rows > 0: PQHIP_EINVAL;
 *   q_row_stride < d, vec_row_stride < d (n_rows > 0), cand_row_stride < n_cand, val_row_stride < k or idx_row_stride < k:
 *   PQHIP_ESHAPE.
 * n_queries == 0 launches nothing; n_rows == 0 writes the padding only (every id other than -1 raises the flag).
 * Asynchronous on `stream`; two kernels per chunk of queries (distances -> 64-bit (key, row id) entries in the codebook's
 * scratch, at most 64 MB per chunk; one workgroup per query sorts them and writes the first k); the caller allocates only
 * the outputs.
 */
int32_t pqhip_rerank_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                             const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                             const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                             const int64_t *d_cand, int32_t n_cand, int64_t cand_row_stride,
                             int32_t metric /* 0 = squared L2, 1 = inner product */, int32_t k,
                             float *d_val, int64_t val_row_stride, int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * Exact search over resident vectors: the exhaustive top-k of every query by its true squared distance or inner product
 * to ALL rows of d_vectors [n_rows][vec_row_stride], vec_bytes = 4 (f32) or 2 (IEEE f16, converted exactly); d_queries
 * [n_queries][q_row_stride] f32; d is the width of both.  It is the ground truth of the quantized searches, the search of
 * rows that are not encoded and the values that `refine` returns.  cb supplies the device slot and the scratch, as for
 * pqhip_rerank_f32_dev; its quantizer is not read and d need not equal its width.
 * Value of a row x for query q: the value pqhip_rerank_f32_dev defines, operation for operation -- the 64 lane chains from
 * +0 over j = l, l + 64, .. with fl(p + fl(t * t)), t = fl(q_j - x_j) (metric 0) or fl(p + fl(q_j * x_j)) (metric 1),
 * then the tree p_l <- fl(p_l + p_(l+s)), s = 32 .. 1; no contraction.
 * A = all rows in [0, n_rows), or with d_allow != NULL those whose bit is set: d_allow is ceil(n_rows / 32) words in the
 * format of the _masked searches (bit r & 31 of word r >> 5; bits beyond n_rows are ignored).  Row q of d_val
 * [n_queries][val_row_stride] and d_idx [n_queries][idx_row_stride] receives the first min(k, |A|) rows of A ordered by
 * (key(value), row) ascending -- inner product: (key(-score), row), the largest score first -- key as for
 * pqhip_adc_search_f32_dev (-0 == +0, every NaN equal and last, ties to the smaller row).  A returned value is the row's
 * value bit for bit, a zero as +0 and a NaN as the canonical quiet NaN; the padding is index -1 with +Inf (inner product:
 * -Inf).  Consequence: for n_rows <= 1024 the call equals pqhip_rerank_f32_dev with the candidate list 0 .. n_rows - 1
 * (or the allowed rows), bit for bit.
 * The order is strict: the result does not depend on the number of workgroups, on the rows each takes or on how many
 * queries share a pass.  A row whose bit is clear enters nothing and none of its bytes is loaded (a NaN in it changes
 * nothing).  No byte outside [d_vectors, last row + d elements) is read, whatever the strides; rows may start at any
 * multiple of the element size.
 * Status codes, in the precedence of pqhip_rerank_f32_dev (EINVAL, ENODEV, EUNSUPPORTED, ESHAPE):
 *   null cb, k < 1, d < 1, n_queries < 0, n_rows < 0, metric not 0 / 1: PQHIP_EINVAL;
 *   vec_bytes not 2 / 4, k > 1024, d > 16384 (one query image is 64 KB of LDS): PQHIP_EUNSUPPORTED;
 *   with n_queries > 0, a null d_queries, d_val or d_idx, or a null d_vectors with n_rows > 0: PQHIP_EINVAL;
 *   q_row_stride < d, vec_row_stride < d (n_rows > 0), val_row_stride < k or idx_row_stride < k: PQHIP_ESHAPE.
 * n_queries == 0 launches nothing; n_rows == 0 or an all-zero mask writes the padding only.
 * Asynchronous on `stream`.  One 1,024-thread producer workgroup per CU over a contiguous range of rows (a multiple of
 * 1,024, so mask words never straddle workgroups; option "flat_search_wgs" forces the number of workgroups) streams the
 * rows once for all queries of a pass -- 4 queries while k <= 128 and d <= 9216, else one; further queries take further
 * passes -- and keeps an exact top-k per wave; the workgroups' partial lists go to the codebook's scratch and one merge
 * kernel per pass writes the outputs, as in pqhip_adc_search_f32_dev.
 */
int32_t pqhip_flat_search_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                  const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                  const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                  const uint32_t *d_allow /* ceil(n_rows / 32) words or NULL */,
                                  int32_t metric /* 0 = squared L2, 1 = inner product */, int32_t k,
                                  float *d_val, int64_t val_row_stride, int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * Exact search in probed lists (IVF-Flat): the search above restricted, per query, to the rows of the lists the query
 * probes.  d_vectors [n_rows][vec_row_stride], f32 or f16 as above, holds the rows in LIST ORDER: with d_list_off
 * [n_lists + 1] int64, list l is the rows [list_off[l], list_off[l + 1]).  d_probes [n_queries][probes_row_stride] int64:
 * the first n_probe entries of row q are list ids; -1 is padding and is skipped; any other value outside [0, n_lists) is
 * skipped and raises the stream's range flag; a range is clamped to [0, n_rows] and an inverted range is empty, and both
 * raise the flag too (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE) -- exactly as for pqhip_adc_search_lists_f32_dev, whose
 * plan kernel reads them here as well.  A list named twice in one row is a caller error: its rows may be returned twice.
 * S_q = the rows of the lists named by probe row q, and with d_allow != NULL those of them whose bit is set: d_allow is
 * ceil(n_rows / 32) words in POSITION order (bit p & 31 of word p >> 5 for the row at position p of d_vectors).
 * Value of a row: the value pqhip_rerank_f32_dev defines, operation for operation -- the 64 lane chains, then the fixed
 * tree, no contraction -- as for pqhip_flat_search_f32_dev.  Row q of the outputs receives the first min(k, |S_q|) rows of
 * S_q ordered by (key(value), position) ascending -- inner product: (key(-score), position) -- with the library's key
 * (-0 == +0, every NaN equal and last); returned indices are positions in d_vectors; the padding is index -1 with +Inf
 * (inner product: -Inf); a returned zero is +0 and a NaN the canonical quiet NaN.
 * Consequences: the result of query q equals pqhip_flat_search_f32_dev on the same matrix with the mask of S_q, query by
 * query, bit for bit.  With every list probed once, in any order, the result equals the unmasked exhaustive call.
 * The order is strict: the result depends neither on the number of workgroups that share a query (chosen on the host
 * from the expected probed bytes, n_queries and the CU count; option "flat_lists_wgs_per_query" forces it) nor on the
 * order of the probes.  No byte outside [d_vectors, last row + d elements) is read, whatever the offsets, probes and
 * strides hold.  No byte of a disallowed or unprobed row is loaded (a NaN in it changes nothing).
 * Status codes, in the precedence EINVAL, ENODEV, EUNSUPPORTED, ESHAPE -- the union of the checks of
 * pqhip_flat_search_f32_dev and pqhip_adc_search_lists_f32_dev:
 *   null cb, k < 1, d < 1, n_queries < 0, n_rows < 0, metric not 0 / 1, n_lists < 0, n_probe < 1: PQHIP_EINVAL;
 *   vec_bytes not 2 / 4, k > 1024, d > 16384, n_rows > 2^32 - 2 (positions are compared as 32-bit values) or
 *   n_probe >= 2^24: PQHIP_EUNSUPPORTED;
 *   with n_queries > 0, a null d_queries, d_val, d_idx, d_list_off or d_probes, or a null d_vectors with n_rows > 0:
 *   PQHIP_EINVAL;
 *   q_row_stride < d, vec_row_stride < d (n_rows > 0), val_row_stride < k, idx_row_stride < k or probes_row_stride <
 *   n_probe: PQHIP_ESHAPE.
 * n_queries == 0 launches nothing; n_rows == 0 or n_lists == 0 writes the padding only.  Asynchronous on `stream`.  One
 * query per 1,024-thread workgroup, grid (workgroups per query, queries): a wave reduces tiles of 16 consecutive places of
 * the query's concatenated probed rows, whatever lists they fall in; the per-query segment plan and the partial lists
 * live in the codebook's scratch (queries are processed in chunks that keep them within 512 MB) and one merge kernel per
 * chunk writes the outputs.
 */
int32_t pqhip_flat_search_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                        const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                        const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                        const int64_t *d_list_off, int64_t n_lists,
                                        const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                        const uint32_t *d_allow /* ceil(n_rows / 32) words in POSITION order, or NULL */,
                                        int32_t metric /* 0 = squared L2, 1 = inner product */, int32_t k,
                                        float *d_val, int64_t val_row_stride, int64_t *d_idx, int64_t idx_row_stride, void *stream);

/*
 * Exact range search over resident vectors: EVERY row whose true squared distance to query q is <= d_threshold[q]
 * (metric 0) resp. whose inner product with it is >= d_threshold[q] (metric 1), over ALL rows of d_vectors
 * (pqhip_flat_range_f32_dev) or over the rows of the lists the query probes (pqhip_flat_range_lists_f32_dev), as CSR.  It
 * is the exact counterpart of the ADC range searches: the ground truth of their recall, the radius question for a
 * collection kept as raw vectors, and the only way to true values for a radius query (re-ranking stops at 1,024
 * candidates).  Every clause is that of an existing call, taken over unchanged.  d_vectors, vec_bytes, d_queries, d and cb
 * are those of pqhip_flat_search_f32_dev (f32 or IEEE f16 converted exactly, d <= 16384; the quantizer of cb is not read).
 * Value of a row: the value pqhip_rerank_f32_dev defines, operation for operation -- the 64 lane chains from +0, then the
 * fixed tree, no contraction.  Predicate: that of pqhip_adc_range_f32_dev -- metric 0: v <= thr[q] as an IEEE comparison,
 * metric 1: v >= thr[q]; a NaN on either side never qualifies; +Inf resp. -Inf matches every non-NaN row.  The value is
 * stored bit for bit; nothing is ordered by value, so there is no key.  The chains start at +0, so a value is never -0:
 * every returned value equals, bit for bit, what pqhip_flat_search_f32_dev returns for that row.
 * Output, order and capacity: d_lims [n_queries + 1] int64, d_val (f32) and d_idx (int64) flat arrays of `capacity`
 * entries, with exactly the capacity protocol of the ADC range calls: d_lims always holds the true counts, only slots
 * < capacity are written and nothing past them is touched, capacity == 0 is a count call (d_val / d_idx may be NULL).
 * Exhaustive call: the rows of query q in ascending row index.  List call: in the order of the concatenation of the probed
 * lists -- probe slot first, then position; d_idx holds positions in d_vectors; a list named twice returns its rows twice.
 * The result is a function of the inputs alone: it does not depend on the grid, the workgroups per query or the queries
 * per pass (options "flat_range_wgs", "flat_range_wgs_per_query" force the grids).
 * Mask and probes: d_allow is NULL or the mask words of the flat searches, in row order for the exhaustive call and in
 * POSITION order for the list call; a disallowed row is not loaded (a NaN in it changes nothing).  d_list_off, d_probes,
 * -1 padding, bad ids, clamped and inverted ranges and the range flag are exactly those of pqhip_flat_search_lists_f32_dev
 * (the same plan kernel reads them).  No byte outside [d_vectors, last row + d elements) is read.
 * Status codes, in the precedence EINVAL, ENODEV, EUNSUPPORTED, ESHAPE -- the union of the checks of
 * pqhip_flat_search_f32_dev resp. pqhip_flat_search_lists_f32_dev and of the ADC range calls, without k:
 *   null cb, d < 1, n_queries < 0, n_rows < 0, capacity < 0, metric not 0 / 1 (list call: n_lists < 0, n_probe < 1):
 *   PQHIP_EINVAL;
 *   vec_bytes not 2 / 4, d > 16384 (list call: n_rows > 2^32 - 2 or n_probe >= 2^24): PQHIP_EUNSUPPORTED;
 *   with n_queries > 0, a null d_lims, d_threshold or d_queries, null outputs with capacity > 0, a null d_vectors with
 *   n_rows > 0 (list call: a null d_list_off or d_probes): PQHIP_EINVAL;
 *   q_row_stride < d, vec_row_stride < d (n_rows > 0) (list call: probes_row_stride < n_probe): PQHIP_ESHAPE.
 * n_queries == 0 launches nothing and writes nothing; n_rows == 0 (list call: or n_lists == 0) writes all-zero lims.
 * Asynchronous on `stream`.  Two passes with a prefix scan between them, as for the ADC range calls: the count pass streams
 * the rows -- once for the 4 queries of a pass while d <= 9216, else one query per pass; the list call one query per
 * workgroup set -- and leaves, beside the partial counts, a bitmap of the hits in the codebook's scratch (one bit per row
 * and query of the pass, n_rows / 8 bytes per query; the list call sizes it for every row probed once); the fill pass loads
 * only the rows that hit, recomputes their values (the same arithmetic on the same bytes: the same bits) and stores them.  A
 * selective radius therefore costs one stream of the matrix plus its hits; a radius that admits every row costs two.  A
 * count call launches no fill.  Queries of the list call are processed in chunks that keep plan, counts and bitmap within
 * 512 MB of scratch.  Results are not sorted by value: sort on the caller's side.
 */
int32_t pqhip_flat_range_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                 const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                 const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                 const uint32_t *d_allow /* ceil(n_rows / 32) words or NULL */,
                                 int32_t metric /* 0 = squared L2, 1 = inner product */,
                                 const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val, int64_t *d_idx,
                                 int64_t capacity, void *stream);
int32_t pqhip_flat_range_lists_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                       const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                       const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                       const uint32_t *d_allow /* ceil(n_rows / 32) words in POSITION order, or NULL */,
                                       const int64_t *d_list_off, int64_t n_lists,
                                       const int64_t *d_probes, int32_t n_probe, int64_t probes_row_stride,
                                       int32_t metric /* 0 = squared L2, 1 = inner product */,
                                       const float *d_threshold /* [n_queries] */, int64_t *d_lims, float *d_val, int64_t *d_idx,
                                       int64_t capacity, void *stream);

/*
 * Exact search among given rows: the exact top-k (pqhip_flat_among_f32_dev) and the exact range result
 * (pqhip_flat_range_among_f32_dev) of every query over the rows that a list of candidate ids names, by the true squared
 * distance or inner product to resident f32 / f16 vectors -- "rank exactly these rows" and "which of these rows lie
 * within the radius" with true values: the (lims, idx) of a range search over codes as they are, a tenant's rows, a
 * graph's neighbour lists, a shortlist of any length from another index.  Every clause is that of an existing call, taken
 * over unchanged.  d_vectors, vec_bytes, d_queries, d and cb are those of pqhip_flat_search_f32_dev (f32 or IEEE f16
 * converted exactly, d <= 16384; the quantizer of cb is not read).
 * Candidates: exactly those of pqhip_adc_among_f32_dev.  The places of query q are d_ids[lims[q] .. lims[q + 1]), with
 * d_lims == NULL every query takes d_ids[0 .. n_ids); C_q is the set of their entries that lie in [0, n_rows).  -1 is
 * padding and is skipped; any other value outside the range is skipped and raises the stream's range flag
 * (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE); no address is formed for it.  An id named twice is a caller error and may
 * be returned twice (the wording of pqhip_rerank_f32_dev).  Ids need not be sorted.  d_lims is device memory and is not
 * trusted: both ends are clamped to [0, n_ids] and an inverted range is empty; both cases raise the flag.  No byte outside
 * d_ids[0 .. n_ids) is read.  A row that is not named is not loaded (a NaN in it changes nothing); no byte outside
 * [d_vectors, last row + d elements) is read.
 * Value of a row: exactly that of pqhip_rerank_f32_dev, operation for operation -- the 64 lane chains from +0, then the
 * fixed tree, no contraction, f16 converted exactly.  It is therefore, bit for bit, the value the flat searches return
 * for that row.
 * Top-k call.  Row q of d_val / d_idx receives the first min(k, |C_q|) members of C_q ordered by (key(value), row id),
 * resp. (key(-score), row id) for the inner product; key, the canonical NaN, zero as +0 and the padding (-1 with +Inf /
 * -Inf) are exactly those of pqhip_flat_search_f32_dev.  The order is strict, so the result depends on neither the order
 * of the ids, nor the grid, nor the chunking.  Hence for distinct in-range ids the result equals, bit for bit, that of
 * pqhip_flat_search_f32_dev with the mask of C_q, run for that query alone, and with at most 1,024 ids per query that of
 * pqhip_rerank_f32_dev on the same candidates.
 * Range call.  The predicate is exactly that of pqhip_flat_range_f32_dev: metric 0: v <= thr[q] as an IEEE comparison,
 * metric 1: v >= thr[q]; a NaN on either side never qualifies.  The output of query q is the SUB-SEQUENCE OF ITS PLACES
 * THAT QUALIFY, IN THE ORDER IN WHICH THEY WERE NAMED: d_idx holds the id as named, d_val its value bit for bit, and a
 * row named twice is returned twice.  The capacity protocol is exactly that of the other range calls: d_out_lims
 * [n_queries + 1] always holds the true counts, only slots < capacity are written and nothing past them is touched,
 * capacity == 0 is a count call (d_val / d_idx may be NULL).  The result is a function of the inputs alone.  Hence with
 * d_ids = 0 .. n_rows - 1 shared it equals pqhip_flat_range_f32_dev without a mask; with ascending distinct ids the masked
 * call with the mask of C_q; and fed the (lims, idx) of any range call at a threshold that admits a superset it returns
 * the exact range result restricted to that superset.
 * Status codes, in the precedence EINVAL, ENODEV, EUNSUPPORTED, null pointers, ESHAPE -- the union of the checks of
 * pqhip_flat_search_lists_f32_dev resp. pqhip_flat_range_lists_f32_dev and of pqhip_adc_among_f32_dev:
 *   null cb, d < 1, n_queries < 0, n_rows < 0, n_ids < 0, metric not 0 / 1 (top-k: k < 1; range: capacity < 0):
 *   PQHIP_EINVAL;  then PQHIP_ENODEV;
 *   vec_bytes not 2 / 4, d > 16384, n_rows > 2^32 - 2 (top-k: k > 1024): PQHIP_EUNSUPPORTED;
 *   with n_queries > 0, a null d_queries, d_ids == NULL with n_ids > 0, a null d_vectors with n_rows > 0 (top-k: a null
 *   output; range: a null d_out_lims or d_threshold, null outputs with capacity > 0): PQHIP_EINVAL;
 *   q_row_stride < d, vec_row_stride < d (n_rows > 0) (top-k: an output stride below k): PQHIP_ESHAPE.
 * n_queries == 0 launches nothing and writes nothing.  n_ids == 0 or n_rows == 0 writes the padding resp. all-zero lims;
 * with n_rows == 0 every id other than -1 raises the flag.  Anything not served is PQHIP_EUNSUPPORTED, never another path.
 * Both calls are asynchronous on `stream`.  One query per workgroup set, also for a shared list; the workgroups that share
 * a query are chosen from the mean number of ids per query (n_ids / n_queries, n_ids with d_lims == NULL) and the row
 * bytes by the rule of pqhip_flat_search_lists_f32_dev (options "flat_among_wgs_per_query",
 * "flat_range_among_wgs_per_query" force the number).  The range call makes two passes with a prefix scan between them:
 * the count pass leaves a bitmap of the hits in scratch and the fill pass loads only the rows that hit; a count call
 * launches no fill.  Scratch comes from the codebook, the caller allocates only the outputs; queries are processed in
 * chunks that keep partial lists resp. counts and bitmaps within 512 MB.
 */
int32_t pqhip_flat_among_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                 const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                 const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                 const int64_t *d_lims /* [n_queries + 1] or NULL */, const int64_t *d_ids, int64_t n_ids,
                                 int32_t metric /* 0 = squared L2, 1 = inner product */, int32_t k,
                                 float *d_val, int64_t val_row_stride, int64_t *d_idx, int64_t idx_row_stride, void *stream);
int32_t pqhip_flat_range_among_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                       const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                       const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                       const int64_t *d_lims /* [n_queries + 1] or NULL */, const int64_t *d_ids, int64_t n_ids,
                                       int32_t metric /* 0 = squared L2, 1 = inner product */,
                                       const float *d_threshold /* [n_queries] */, int64_t *d_out_lims, float *d_val,
                                       int64_t *d_idx, int64_t capacity, void *stream);

/*
 * Conservative range screen over resident vectors on the matrix cores: for a BATCH of queries, per query a superset of
 * what pqhip_flat_range_f32_dev returns at the same thresholds, as ascending row ids (CSR, no values).  It is the first
 * stage of the exact searches for query batches: screen, then resolve the candidates exactly with
 * pqhip_flat_range_among_f32_dev / pqhip_flat_among_f32_dev, whose results are those of the exhaustive calls bit for bit.
 * One stream of the matrix serves up to 64 queries.  Arguments: those of pqhip_flat_range_f32_dev without d_val, and
 * x_exp: every row element is multiplied by 2^x_exp (exact) before it is rounded to f16 -- choose it so that the largest
 * |element| of the matrix lands below 2^15 (and well above 2^-14).  The quantizer of cb is not read.
 * Contract.  Let R_q be the ids pqhip_flat_range_f32_dev returns for query q at d_threshold[q] (same vectors, mask and
 * metric; values as pqhip_rerank_f32_dev defines them), O_q the ids of this call, A the allowed rows.
 *   Sound, unconditionally: R_q is a subset of O_q, O_q of A.  A row is left out only when the kernel has proved that its
 *   exact value misses the threshold; whatever the proof does not cover is returned -- a non-finite element in the row or
 *   the query, a scaled row element that overflows f16, a NaN or an infinity out of the matrix instruction, a NaN
 *   threshold, |x_exp| > 40, a query whose largest |element| is outside [2^-40, 2^40) and not zero.
 *   Tight on regular rows (finite elements, every scaled element below 2^15, ||x||^2 within f32, a finite query that the
 *   proof covers, d <= 2048): a regular row is returned only if its exact value v satisfies v <= thr + slack (metric 0)
 *   resp. v >= thr - slack / 2 (metric 1), slack = 2^-8 (||x||^2 + ||q||^2) + 2^-12 2^-x_exp ||q||_1 + 2^-99.  The
 *   bound behind it is derived in DESIGN.md section 5c; its constants are kFlatScreenRel, kFlatScreenAbsX and
 *   kFlatScreenAbs of kernels_flat_screen.hip.h.
 * Output, order and capacity: d_lims [n_queries + 1] int64 and d_idx (int64) of `capacity` entries; the ids of a query
 * ascend; the capacity protocol is exactly that of the range calls (true counts always, only slots < capacity written,
 * capacity == 0 a count call with d_idx NULL).  The count pass leaves the hit bitmap in the codebook's scratch (4 bytes
 * per tile of 32 rows and query slot of a pass); the fill pass turns bitmaps into ids and does not read the matrix.
 * A function of the inputs alone: every (row, query) product sum is one chain of v_mfma_f32_32x32x16_f16 in a fixed k
 * order; the result depends neither on the grid (option "flat_screen_wgs") nor on how queries are grouped into passes.
 * Memory: no byte outside [d_vectors, last row + d elements) is read; rows may start at any multiple of the element
 * size (16-, 8- and 4-byte loads are used only when base and row stride are multiples of that size); a disallowed row is not loaded.
 * vec_bytes 2: the f16 rows are used as they are, x_exp is still applied.
 * Status codes, in the precedence of the range call: null cb, d < 1, n_queries < 0, n_rows < 0, capacity < 0, metric not
 * 0 / 1: PQHIP_EINVAL; vec_bytes not 2 / 4, d > 2048: PQHIP_EUNSUPPORTED; with n_queries > 0 a null d_lims, d_threshold or
 * d_queries, a null d_idx with capacity > 0, a null d_vectors with n_rows > 0: PQHIP_EINVAL; q_row_stride < d,
 * vec_row_stride < d (n_rows > 0): PQHIP_ESHAPE.  n_queries == 0 launches nothing; n_rows == 0 writes all-zero lims.
 * Asynchronous on `stream`; per pass of 64 queries (32 while d > 1024): a prep kernel (the f16 query image with one
 * power-of-two scale per query), the count pass, the prefix scan of the range calls, the fill pass (none for a count call).
 */
int32_t pqhip_flat_screen_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                  const float *d_queries, int64_t n_queries, int64_t q_row_stride,
                                  const void *d_vectors, int32_t vec_bytes, int64_t n_rows, int64_t d, int64_t vec_row_stride,
                                  const uint32_t *d_allow /* ceil(n_rows / 32) words or NULL */,
                                  int32_t metric /* 0 = squared L2, 1 = inner product */, int32_t x_exp,
                                  const float *d_threshold /* [n_queries] */, int64_t *d_lims, int64_t *d_idx,
                                  int64_t capacity, void *stream);

/*
 * Merge of two list-ordered row arrays: the primitive under growing a partitioned matrix (rows added to an index, two
 * indexes over the same lists joined).  d_a is [n_a] rows of row_bytes bytes in list order under d_off_a [n_lists + 1]
 * (list l = rows off_a[l] .. off_a[l + 1] - 1), d_b likewise [n_b] rows under d_off_b; d_out is [n_a + n_b] rows.  For
 * every list l the output rows from off_a[l] + off_b[l] on are the rows a[off_a[l] : off_a[l + 1]] followed by the rows
 * b[off_b[l] : off_b[l + 1]], copied byte for byte; d_off_out, if given, receives off_out[l] = off_a[l] + off_b[l] for
 * l in [0, n_lists], the offsets of the merged lists.  Rows are contiguous: the stride of all three arrays is row_bytes.
 * None of the three base pointers needs any alignment (stores are 16 bytes wide on the 16-byte grid of the destination
 * address whatever it is; the sources are read at the byte addresses they have).  d_out must not overlap an input.
 * cb supplies the device slot, the scratch and the stream's range flag, as for pqhip_rerank_f32_dev; its quantizer is
 * not read.
 * The offsets are device memory and are NOT TRUSTED.  An offset array is valid iff off[0] == 0, it is non-decreasing
 * and off[n_lists] == n.  If either array is invalid, no byte of d_out is written, no byte outside the inputs is read
 * (no row is read at all), the stream's range flag is raised (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE) and the
 * contents of d_off_out are unspecified.  A small plan kernel is the only reader of the offsets; it writes the table
 * of the 2 n_lists output segments into the codebook's scratch, and the mover -- each workgroup a contiguous slice of
 * the output bytes -- runs only behind a valid plan.  The value of an output byte depends on its position alone: the
 * result does not depend on the number of workgroups (chosen from the size and the CU count; option "lists_merge_wgs"
 * forces it).
 * Status codes: a null cb, a negative count, row_bytes < 1, n_lists == 0 with n_a + n_b > 0: PQHIP_EINVAL; then the
 * slot (PQHIP_ENODEV); row_bytes > PQHIP_LISTS_MERGE_MAX_ROW_BYTES, n_lists > PQHIP_LISTS_MERGE_MAX_LISTS (the plan is
 * one workgroup, the table 32 bytes per list) or more than 2^49 rows in an input: PQHIP_EUNSUPPORTED; with n_a + n_b > 0
 * a null d_off_a, d_off_b or d_out, a null d_a with n_a > 0 or a null d_b with n_b > 0: PQHIP_EINVAL.  n_a + n_b == 0
 * writes d_off_out (all zeros; the offsets are not read) and launches no kernel.  Asynchronous on `stream`.
 */
#define PQHIP_LISTS_MERGE_MAX_ROW_BYTES 4096
#define PQHIP_LISTS_MERGE_MAX_LISTS 1048576
int32_t pqhip_lists_merge_dev(pqhip_codebook *cb, int32_t device_slot,
                              const int64_t *d_off_a, int64_t n_a,
                              const int64_t *d_off_b, int64_t n_b, int64_t n_lists,
                              int64_t row_bytes, const void *d_a, const void *d_b, void *d_out,
                              int64_t *d_off_out /* or NULL */, void *stream);

/*
 * Stable compaction of a row array under a row mask: the primitive under removing rows from a resident matrix, the twin
 * of pqhip_lists_merge_dev.  d_keep is a row mask in the format of the _masked searches and pqhip_pack_row_mask_dev:
 * ceil(n / 32) words, bit i & 31 of word i >> 5 set = row i is kept; bits of the last word at or beyond n are ignored,
 * whatever they hold, and no byte outside those words is read.  With K the set of kept rows, c = |K| and
 * s_0 < s_1 < .. < s_(c-1) its members: d_count[0] = c, always.  If c <= out_capacity_rows, row j of d_out is row s_j of
 * d_in, byte for byte, for j < c, and d_src_rows[j] = s_j if d_src_rows is given; no byte of d_out at or beyond
 * c row_bytes and no element of d_src_rows at or beyond c is written.  If c > out_capacity_rows, no byte of d_out or
 * d_src_rows is written and no flag is raised: the count is the answer, the caller allocates and calls again (the
 * capacity rule of the range searches: never write past the caller's buffers).  d_in == NULL together with
 * d_out == NULL moves no rows: the count, the offsets and the source rows only.  Rows are contiguous: the stride of both
 * arrays is row_bytes.  No base pointer needs any alignment (stores are 16 bytes wide on the 16-byte grid of the
 * destination address whatever it is; the source is read at the byte addresses it has).  d_out must not overlap d_in.
 * Bytes of rows that are not kept may be read -- they lie inside the input and are never interpreted; no byte outside
 * the n row_bytes input bytes is read.  cb supplies the device slot, the scratch and the stream's range flag, as for
 * pqhip_lists_merge_dev; its quantizer is not read.
 * List offsets.  With d_off_in given ([n_lists + 1], the list offsets of a list-ordered array), d_off_out[l] is the number
 * of kept rows i < off_in[l], for l in [0, n_lists]: compaction is stable in position order, so list l of the output is
 * exactly the kept rows of list l, in order.  The offsets are device memory and are NOT TRUSTED.  The array is
 * valid iff off[0] == 0, it is non-decreasing and off[n_lists] == n.  If it is invalid, no byte of d_out or d_src_rows is
 * written, no row is read, the stream's range flag is raised (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE) and d_count
 * and d_off_out are unspecified.  A mask can hold anything: every mask is valid.
 * Three kernels in stream order, none of which waits for another workgroup: every workgroup counts the kept rows of a
 * contiguous slice of source rows (a multiple of 1,024) and of each of its tiles of 1,024; one workgroup turns the
 * counts into each slice's first output row and the total, checks the offsets, computes d_off_out and decides whether
 * the mover runs (valid offsets, c <= out_capacity_rows); the mover walks the slices again.  The result is a function of
 * the input alone: it does not depend on the number of workgroups (chosen from the size and the CU count; option
 * "rows_compact_wgs" forces it).
 * Status codes, in the precedence of pqhip_lists_merge_dev: a null cb, n < 0, row_bytes < 1, out_capacity_rows < 0, a null
 * d_count, n_lists < 0, exactly one of d_in / d_out null, d_off_out given without d_off_in, a null d_keep with n > 0:
 * PQHIP_EINVAL; then the slot (PQHIP_ENODEV); row_bytes > PQHIP_ROWS_COMPACT_MAX_ROW_BYTES, n_lists >
 * PQHIP_LISTS_MERGE_MAX_LISTS, n > 2^49 or counts beyond the scratch limit (4 bytes per 1,024 rows): PQHIP_EUNSUPPORTED.
 * n == 0 writes d_count[0] = 0 and an all-zero d_off_out (the offsets are not read) and launches no kernel.
 * Asynchronous on `stream`; the counts live in the codebook's scratch.
 */
#define PQHIP_ROWS_COMPACT_MAX_ROW_BYTES 4096
int32_t pqhip_rows_compact_dev(pqhip_codebook *cb, int32_t device_slot,
                               const uint32_t *d_keep, int64_t n, int64_t row_bytes,
                               const void *d_in /* or NULL */, void *d_out /* or NULL */, int64_t out_capacity_rows,
                               const int64_t *d_off_in /* or NULL */, int64_t n_lists, int64_t *d_off_out /* or NULL */,
                               int64_t *d_src_rows /* or NULL */, int64_t *d_count, void *stream);

/*
 * Exact merge of the top-k results of several searches: the primitive under searching several resident matrices as one
 * (a main index plus a delta, more rows than one call takes, row shards on several devices gathered on one).
 * d_val is f32 [n_parts][n_queries][k_in] and d_idx int64 of the same shape, each with a part stride and a row stride in
 * elements and a column stride of one.  Row q of part p is what a search of part p returned for query q: first its real
 * entries in that search's order, then padding with index -1.  d_offsets is int64 [n_parts] in device memory or NULL; it
 * is added to every index >= 0 of its part.  largest is 0 for distances and 1 for scores.  d_out_val and d_out_idx are
 * [n_queries][k] with row strides; d_out_part is int32 [n_queries][k] with a row stride, or NULL, and receives the part
 * each result came from.
 * Definition.  An entry with index < 0 is absent, whatever its value holds.  The present entries of query q are ordered by
 * (key(v), part, rank within the part's row), ascending; with largest the key is key(-v).  key() is the order of every
 * search of the library: -0 == +0, every NaN equal to every other and after every number.  The output row is the first
 * min(k, count) of them; after them come index -1, value +Inf (largest: -Inf) and part -1.  Values come back as the
 * searches return them: bit for bit, a NaN as the canonical quiet NaN and a zero as +0.  No element of an output row at or
 * beyond k is written.
 * The merge is stable and never compares ids.
 *   - If the parts are consecutive row ranges of one matrix, given in order, and each row is a result of an exhaustive
 *     search (plain, masked, packed or re-ranked), the output is bit for bit that search on the whole matrix for every
 *     k <= k_in.
 *   - For any parts the values are those of the union.  Ties go to the earlier part.
 *   - A row whose present entries are not in that order gives an unspecified order, but nothing is read or written out
 *     of bounds.
 * k > n_parts k_in is allowed: the row is padded.  Only the first min(k_in, 64 L) entries of a part's row are read, with L
 * the smallest power of two with 64 L >= k: later entries cannot reach the output.
 * One kernel, one workgroup per query and one wave per part (at most eight waves; further parts go round): a wave reads a
 * part's row with consecutive lanes on consecutive entries, the waves' sorted lists of 32-bit (key, part << 10 | rank)
 * pairs are merged in a tree through at most 32 KB of LDS, and the id of each of the k winners is fetched once.  Queries
 * are taken grid-stride: the result does not depend on the number of workgroups (min(n_queries, 2^20); option
 * "topk_merge_wgs" forces it).  cb supplies the device slot and the stream's device, as for pqhip_rerank_f32_dev; its
 * quantizer is not read.  The call needs no scratch.
 * Status codes, in the precedence of pqhip_adc_search_f32_dev: a null cb, n_queries < 0, n_parts < 1, k < 1, k_in < 1, a
 * `largest` other than 0 or 1: PQHIP_EINVAL; then the slot (PQHIP_ENODEV); k or k_in > PQHIP_TOPK_MERGE_MAX_K, n_parts >
 * PQHIP_TOPK_MERGE_MAX_PARTS: PQHIP_EUNSUPPORTED; n_queries == 0 launches nothing; then a null d_val, d_idx, d_out_val or
 * d_out_idx: PQHIP_EINVAL; an input row stride < k_in or an output row stride < k: PQHIP_ESHAPE.  Part strides are not
 * constrained.  Asynchronous on `stream`.
 */
#define PQHIP_TOPK_MERGE_MAX_K 1024
#define PQHIP_TOPK_MERGE_MAX_PARTS 65536
int32_t pqhip_topk_merge_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                 const float *d_val, int64_t val_part_stride, int64_t val_row_stride,
                                 const int64_t *d_idx, int64_t idx_part_stride, int64_t idx_row_stride,
                                 int64_t n_parts, int64_t n_queries, int32_t k_in,
                                 const int64_t *d_offsets /* or NULL */, int32_t largest, int32_t k,
                                 float *d_out_val, int64_t out_val_row_stride, int64_t *d_out_idx, int64_t out_idx_row_stride,
                                 int32_t *d_out_part /* or NULL */, int64_t out_part_row_stride, void *stream);

/*
 * Building a partitioned index on the device: the layout of the lists, the residuals and the query-free row terms.
 *
 * pqhip_lists_layout_dev: d_assign is [n] list ids, signed integers of idx_bytes (4 or 8) bytes each.  With `ids` the
 * STABLE argsort of the assignments (positions inside a list ascend in row number) the outputs are
 *     d_list_off [n_lists + 1]   prefix sums of the list sizes (empty lists are legal)
 *     d_ids [n]                  ids[p] = the row at position p
 *     d_positions [n]            positions[ids[p]] = p
 *     d_lists [n] or NULL        lists[p] = assign[ids[p]]
 * all int64.  A counting sort in one pass over the ids: every workgroup counts a contiguous slice of rows, a scan gives
 * the offsets and each workgroup's first position in each list, and the workgroups walk their slices again in row
 * order.  The result is a function of the input alone: it does not depend on the number of workgroups (chosen from the
 * size, the number of lists and the CU count; option "lists_layout_wgs" forces it).  cb supplies the device slot, the
 * scratch (8 bytes per list and workgroup) and the stream's range flag, as for pqhip_lists_merge_dev; its quantizer is
 * not read.
 * The ids are device memory and are NOT TRUSTED.  If any id is negative or >= n_lists, no element of d_ids, d_positions
 * or d_lists is written, the stream's range flag is raised (pqhip_check_codes_dev -> PQHIP_ECODE_RANGE) and the
 * contents of d_list_off are unspecified: the counting pass validates, and the placing pass runs only behind a validity
 * word.
 * Status codes: a null cb, n < 0, n_lists < 1, idx_bytes other than 4 or 8, a null d_list_off, with n > 0 a null d_assign,
 * d_ids or d_positions: PQHIP_EINVAL; then the slot (PQHIP_ENODEV); n_lists > PQHIP_LISTS_LAYOUT_MAX_LISTS (the k-means
 * limit; it bounds the table of counts a workgroup keeps in LDS) or n > 2^49: PQHIP_EUNSUPPORTED, as is a table of counts
 * beyond the scratch limit (a workgroup takes at most 2^31 rows).  n == 0 writes an all-zero d_list_off and launches no
 * kernel.  Asynchronous on `stream`.
 *
 * pqhip_residuals_f32_dev: out[i][j] = x[i][j] - centroids[assign[i]][j] for i < n, j < d: one IEEE f32 subtraction per
 * element.  d_x and d_out are [n][d] with row strides in elements (>= d, PQHIP_ESHAPE otherwise), d_assign int64 [n],
 * d_centroids [n_lists][d] contiguous.  A list id outside [0, n_lists) writes a zero row and raises the range flag.  No
 * base or stride needs any alignment: loads and stores are 16 bytes wide where the three addresses allow it and single
 * elements elsewhere.  d_out must not overlap an input.  d <= PQHIP_RESIDUALS_MAX_D (PQHIP_EUNSUPPORTED).
 *
 * pqhip_residual_terms_f32_dev: the query-free term of a residual-encoded row (pqhip_adc_search_lists_residual_f32_dev:
 * row_terms) without a reconstruction.  cb is the residual quantizer (M subquantizers of K <= 256 centroids, sub-vectors
 * of ds floats), d_codes [n][M] one byte per code with a row stride (>= M, PQHIP_ESHAPE otherwise), d_assign int64 [n],
 * d_centroids [n_lists][M ds] contiguous, d_out f32 [n].  With r = quantizers[m][code[i][m]][e] and
 * c = centroids[assign[i]][m ds + e], both widened to f64:
 *     p[i][m] = the sequential f64 sum over e = 0 .. ds - 1, starting from +0, of (r r + 2 c r): both products are exact,
 *               their sum is one rounded addition, adding it to the running sum a second one; nothing is fused
 *     out[i]  = (float) of the sequential f64 sum over m = 0 .. M - 1, starting from +0, of p[i][m] (to nearest even)
 * A code >= K reads entry 0 and raises the range flag; a list id outside [0, n_lists) writes +0 and raises it.
 * A codebook WITH A PROJECTION is PQHIP_EUNSUPPORTED (its reconstruction includes the inverse rotation, which this call
 * does not apply), as are K > 256, M > PQHIP_RESIDUAL_TERMS_MAX_M and M ds > PQHIP_RESIDUALS_MAX_D.
 *
 * Status codes of the two residual calls: a null cb, n < 0, n_lists < 1 (d < 1): PQHIP_EINVAL; then the slot
 * (PQHIP_ENODEV); then PQHIP_EUNSUPPORTED as above; n == 0 is PQHIP_OK and launches nothing; then a null pointer
 * (PQHIP_EINVAL) and the strides (PQHIP_ESHAPE).  Asynchronous on `stream`.
 */
#define PQHIP_LISTS_LAYOUT_MAX_LISTS 16384
#define PQHIP_RESIDUALS_MAX_D 1048576
#define PQHIP_RESIDUAL_TERMS_MAX_M 8192
int32_t pqhip_lists_layout_dev(pqhip_codebook *cb, int32_t device_slot,
                               const void *d_assign, int32_t idx_bytes, int64_t n, int64_t n_lists,
                               int64_t *d_list_off, int64_t *d_ids, int64_t *d_positions,
                               int64_t *d_lists /* or NULL */, void *stream);
int32_t pqhip_residuals_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                const float *d_x, int64_t n, int64_t d, int64_t x_row_stride,
                                const int64_t *d_assign, const float *d_centroids, int64_t n_lists,
                                float *d_out, int64_t out_row_stride, void *stream);
int32_t pqhip_residual_terms_f32_dev(pqhip_codebook *cb, int32_t device_slot,
                                     const uint8_t *d_codes, int64_t n, int64_t codes_row_stride,
                                     const int64_t *d_assign, const float *d_centroids, int64_t n_lists,
                                     float *d_out, void *stream);

/* Reconstruct's range check is asynchronous on the device path: returns PQHIP_ECODE_RANGE if any
 * device call since the last query saw a code >= K (synchronises `stream`). */
int32_t pqhip_check_codes_dev(pqhip_codebook *cb, int32_t device_slot, void *stream);

/*
 * "Next" row of the hot path: the assignment step of k-means training,
 * `kmeans::cluster_assignments(centroids, instances, Axis(0))` (src/kmeans.rs:133-159, called from
 * kmeans.rs:319 and through primitives::quantize_batch::<_, usize, _> at opq.rs:180).  Same kernels
 * as PQ encode with one subquantizer; out[i] = index of the nearest of the K centroids [K][dim] for
 * row i of x, as out_bytes-wide unsigned integers (8 = usize).  Host buffers, element strides.
 */
int32_t pqhip_cluster_assignments_f32(pqhip_ctx *ctx, const float *centroids, int64_t n_centroids,
                                      int64_t dim, const float *x, int64_t n_rows,
                                      int64_t x_row_stride, int64_t x_col_stride, void *out,
                                      int32_t out_bytes);

/*
 * The whole k-means step of PQ/OPQ training, for all M subquantizers at once: `n_iterations` times
 * `kmeans_iteration` (src/kmeans.rs:308-327 = cluster_assignments :133-159, update_centroids
 * :166-198, mean_squared_error :329-360) on every subquantizer's column block of x.  It replaces
 *   - `sq_instances.kmeans_with_centroids(Axis(0), quantizer, NIterationsCondition(n_iterations))`
 *     (src/pq/pq.rs:176; kmeans.rs:270-279) for every subquantizer of `train_pq_using`
 *     (pq.rs:214-241), with the initial centroids of pq.rs:166-172 passed in;
 *   - `Opq::update_subquantizers` (src/pq/opq.rs:227-245) with n_iterations = 1 and loss = NULL
 *     (x = the rotated instances);
 *   - a plain `kmeans_iteration` / `kmeans_with_centroids` with M = 1, dsub = dim.
 * quantizers [M][K][dsub] (host, C order) holds the initial centroids and receives the updated
 * ones; loss (host, [M], may be NULL) receives the LAST iteration's mean squared error of every
 * subquantizer.  Results are bit-identical to the reference's sequential f32 arithmetic (sums in
 * row order, f32 counts, IEEE division, one sequential fold for the loss); empty clusters become
 * zero vectors as in kmeans.rs:180-197.  The instances stay resident on one device for all
 * iterations (host entry point: the first device of the context).  Limits: K <= 16384,
 * n_rows <= 2^31; sub-vectors wider than 256 floats use the slow anchor kernel for the assignment
 * step.  Both calls return synchronised.
 */
int32_t pqhip_kmeans_iterations_f32(pqhip_ctx *ctx, float *quantizers, int64_t n_subquantizers,
                                    int64_t n_centroids, int64_t sub_dim, const float *x,
                                    int64_t n_rows, int64_t x_row_stride, int64_t x_col_stride,
                                    int32_t n_iterations, float *loss);

/* same, instances already in HBM on `device_slot` (unit column stride) */
int32_t pqhip_kmeans_iterations_f32_dev(pqhip_ctx *ctx, int32_t device_slot, float *quantizers,
                                        int64_t n_subquantizers, int64_t n_centroids,
                                        int64_t sub_dim, const float *d_x, int64_t n_rows,
                                        int64_t x_row_stride, int32_t n_iterations, float *loss,
                                        void *stream);

/*
 * Resident instance matrices for the training entry points (which iterate over the same rows many
 * times): a row-major copy [n_rows][n_cols] of a host matrix (any element strides) in the HBM of
 * `device_slot`.  pqhip_matrix_device_ptr() is what the *_dev entry points take as d_x (row stride
 * n_cols).  A caller that has no device-memory management of its own (the Rust binding) uploads
 * once per training run.
 */
typedef struct pqhip_matrix pqhip_matrix;
int32_t pqhip_matrix_upload_f32(pqhip_ctx *ctx, int32_t device_slot, const float *x, int64_t n_rows,
                                int64_t n_cols, int64_t x_row_stride, int64_t x_col_stride,
                                pqhip_matrix **out);
const float *pqhip_matrix_device_ptr(const pqhip_matrix *m);
int64_t pqhip_matrix_rows(const pqhip_matrix *m);
void pqhip_matrix_destroy(pqhip_matrix *m);

/*
 * The device part of `Opq::train_iteration` (src/pq/opq.rs:156-195), i.e. everything of an OPQ
 * training iteration except its LAPACK call:
 *   rx = instances.dot(&projection)                                   (opq.rs:167)
 *   update_subquantizers(centroids, rx)   -- one kmeans_iteration per subquantizer  (:168, :227-245)
 *   quantized = quantize_batch::<usize>(centroids, rx); reconstruct_batch_into(centroids, quantized, rx)
 *                                                                     (:176-182, no projection)
 *   cross = instances.t().dot(&reconstructed)                         (first half of :191)
 * quantizers [M][K][dsub] (host, in/out), projection [d][d] (host, in), instances d_x [n][d] resident
 * in HBM on `device_slot`; cross [d][d] (host, out).  The caller finishes the iteration with
 * `(u, _, vt) = cross.svd(); projection = u.dot(vt)` (opq.rs:191-192).  Every step follows the
 * arithmetic rules of DESIGN.md section 3 (the cross product is rule 2 with k over the rows: chains
 * restart every 256 rows, block results added in row order), so quantizers and cross are
 * bit-identical to the reference's default build for the same projection.  Returns synchronised.
 */
int32_t pqhip_opq_train_step_f32_dev(pqhip_ctx *ctx, int32_t device_slot, float *quantizers,
                                     int64_t n_subquantizers, int64_t n_centroids, int64_t sub_dim,
                                     const float *projection, const float *d_x, int64_t n_rows,
                                     int64_t x_row_stride, float *cross, void *stream);

/* d_out [n][d] = d_x [n][d] . projection [d][d] (host) on the device with rule-2 arithmetic:
 * `instances.dot(&projection)` of the training paths (opq.rs:62, gaussian_opq.rs:55).  Returns synchronised. */
int32_t pqhip_rotate_f32_dev(pqhip_ctx *ctx, int32_t device_slot, const float *d_x, int64_t n_rows,
                             int64_t x_row_stride, int64_t d, const float *projection, float *d_out,
                             int64_t out_row_stride, void *stream);

/* out [da][db] (host) = a^T . b for device-resident a [n][da], b [n][db] (unit column strides) with
 * the same rule-2 arithmetic: `a.t().dot(&b)` of ndarray (opq.rs:191). */
int32_t pqhip_at_dot_b_f32_dev(pqhip_ctx *ctx, int32_t device_slot, const float *d_a,
                               int64_t a_row_stride, int64_t da, const float *d_b,
                               int64_t b_row_stride, int64_t db, int64_t n_rows, float *out,
                               void *stream);

/* ---- knobs used by the test-suite and the bench (not part of the reference surface) --------
 * The library reads three environment variables (PQHIP_PACK_THREADS, PQHIP_HOST_ZERO_COPY, PQHIP_FUSED2_OPQ: all
 * about the host path / deployment); every other switch is an explicit call below.
 *
 * pqhip_set_encode_variant: force an encode kernel family on one codebook (PQHIP_EUNSUPPORTED from the next
 * quantize call when the family has no instantiation for the shape).  Codebooks with sub-vectors of more than 128 floats or
 * K > 256 have one matrix-core form, through 64-bit keys: every variant other than 1 and 8 takes it where it applies.
 *   0  auto
 *   1  scalar anchor kernel (exact by construction, any shape)
 *   2  MFMA 32x32x2 with a lane-local (VALU) argmin          auto for sub-vectors of <= 2 floats
 *   4  MFMA 32x32x2, LDS-atomic argmin, fragments in LDS     auto wherever 9 is not taken; K > 256; k-means
 *   6  VALU kernel for small codebooks (K <= 64, u8 codes)   auto for K <= 16, sub-vectors of <= 8 floats where 10 does not fit
 *   7  two subquantizers per matrix tile (K <= 16)           auto for 2 floats, and 4 floats from 48 subquantizers on
 *   8  OPQ only: rotation + encode in one kernel             auto where instantiated (opq_fused2_launch.h)
 *   9  MFMA 16x16x4, LDS-atomic argmin, four waves per SIMD  auto for K > 128 and sub-vectors of 12 .. 24 floats;
 *      256 centroids of 20 floats: a bf16 16x16x32 screen, undecided rows resolved exactly (same codes)
 *  10  MFMA 16x16x4 for small codebooks (K <= 32, 4 / 8 / 12 / 16 / 20 / 24 / 32 floats, u8 codes, 16-byte aligned rows)   auto wherever it fits
 *  11  1- and 2-float sub-vectors, K <= 256: per-cell candidate lists (Pq handles with finite, in-range centroids)
 *      auto for K > 16, and for every K at 1 float
 *   (3 and 5 named kernels that rounds 1-2 shipped; PQHIP_EINVAL since round 4)                                  */
int32_t pqhip_set_encode_variant(pqhip_codebook *cb, int32_t variant);
/* process-wide: the P-block rotation kernel where both exist (16-byte aligned rows, d % 4 == 0):
 *   0  auto: k_rotate_pblock9 (16x16x4) for the gather form (OPQ reconstruct), for d > 640, and for plain rotation
 *      where 64-column blocks would execute >= 10 % more columns than 16-column tiles (d = 96, 144, 272, 400 ..);
 *      k_rotate_pblock8 (32x32x2) otherwise
 *   8 / 9  force one of them                                                                                    */
int32_t pqhip_set_rotation_variant(int32_t variant);
/* per-context options (value >= 0; PQHIP_EINVAL for an unknown name):
 *   "kmeans_window_rows"   rows per window of the k-means iteration (0 = default, 512 K)
 *   "kmeans_lane_form"     1 = lane-per-chain update walk for every shape
 *   "kmeans_no_graph"      1 = never replay small training sets as a captured hipGraph
 *   "opq_scratch_rows"     rows per chunk of the two-kernel OPQ paths (0 = whole rounds of the rotation grid)
 *   "opq_fused"            0 = OPQ encode as rotation -> scratch -> encode (default 1; PQHIP_FUSED2_OPQ=0 presets 0)
 *   "opq_gather_rotation"  0 = OPQ reconstruct as gather -> scratch -> rotation (default 1)
 *   "adc_single_query"     1 = one scan pass per query (default 0: 8 / 4 queries share a pass)
 *   "adc_lists_wgs_per_query"  workgroups that share one query of the list searches (0 = chosen from the shape; at most 4096)
 *   "adc_among_wgs_per_query"  workgroups that share one query of the searches among given rows (0 = chosen from the
 *                          mean number of ids per query; at most 4096)
 *   "adc_range_wgs"        producer workgroups of the exhaustive range searches (0 = chosen from the shape; at most 8192,
 *                          so that the one-workgroup prefix scan of a pass sums at most 2^20 counts)
 *   "adc_range_wgs_per_query"  workgroups that share one query of the list range searches (0 = chosen from the shape; at
 *                          most 4096, as "adc_lists_wgs_per_query")
 *   "adc_search_wgs"       producer workgroups of the exhaustive searches over 1- and 4-byte codes, masked or not (0 = one
 *                          per CU with at least 4,096 rows; at most 65536; rows per workgroup stay a multiple of 1,024)
 *   "adc_packed4_wgs"      producer workgroups of the exhaustive searches over 4-bit packed codes (0 = chosen from the shape,
 *                          as for the u8 searches; at most 65536; rows per workgroup stay a multiple of 1,024)
 *   "lists_merge_wgs"      workgroups of the mover of pqhip_lists_merge_dev (0 = chosen from the size and the CU count; at
 *                          most 2^20, and never more than one per 1,024 16-byte chunks of output)
 *   "lists_layout_wgs"     workgroups (row slices) of pqhip_lists_layout_dev (0 = chosen from the size, the number of lists and
 *                          the CU count; at most 65536, never more than one per 1,024 rows; the result does not depend on it)
 *   "rows_compact_wgs"     workgroups (row slices) of pqhip_rows_compact_dev (0 = chosen from the size and the CU count; at most
 *                          2^20, never more than one per 1,024 rows; the result does not depend on it)
 *   "topk_merge_wgs"       workgroups of pqhip_topk_merge_f32_dev (0 = one per query up to 2^20; at most 2^20, never more than
 *                          one per query; the result does not depend on it)
 *   "rerank_wgs_per_query" workgroups that share one query in the distance stage of pqhip_rerank_f32_dev (0 = chosen from the
 *                          shape; at most 1024)
 *   "flat_search_wgs"      producer workgroups of pqhip_flat_search_f32_dev (0 = one per CU; at most 65536; rows per workgroup
 *                          stay a multiple of 1,024; the result does not depend on it)
 *   "flat_lists_wgs_per_query"  workgroups that share one query of pqhip_flat_search_lists_f32_dev (0 = chosen from the
 *                          expected probed bytes; at most 4096; the result does not depend on it)
 *   "flat_range_wgs"       producer workgroups of pqhip_flat_range_f32_dev (0 = one per CU; at most 16384, so that the
 *                          one-workgroup prefix scan of a pass of 4 queries sums at most 2^20 counts; rows per workgroup
 *                          stay a multiple of 1,024; the result does not depend on it)
 *   "flat_range_wgs_per_query"  workgroups that share one query of pqhip_flat_range_lists_f32_dev (0 = chosen from the
 *                          expected probed bytes; at most 4096; the result does not depend on it)
 *   "flat_among_wgs_per_query"  workgroups that share one query of pqhip_flat_among_f32_dev (0 = chosen from the mean
 *                          number of ids per query and the row bytes; at most 4096; the result does not depend on it)
 *   "flat_range_among_wgs_per_query"  the same for pqhip_flat_range_among_f32_dev
 *   "flat_screen_wgs"      producer workgroups of pqhip_flat_screen_f32_dev (0 = two per CU; at most 2048, so that the
 *                          prefix scan of a pass of 64 queries sums at most 2^20 counts; rows per workgroup stay a
 *                          multiple of 256; the result does not depend on it)
 *   "cross_product_exact" 0 = X^T.R of the OPQ training step / pqhip_at_dot_b_f32_dev as a plain split-K product:
 *                          within 1e-5 relative of the exact rule-2 result, no per-block partial matrices (default 1)
 *   "cross_product_group_bytes"  workspace of partial matrices per launch group (0 = 4 GiB)
 *   "lookup_two_pass"      row lookups (pqhip_reconstruct_rows*): 0 = one kernel, 1 = select the code rows into a compact
 *                          staging area first, 2 (default) = two passes when the resident matrix exceeds 256 MB
 *   "candidate_tables"     1 (default): pqhip_codebook_create builds the per-cell candidate tables of the 1- / 2-float sub-vector
 *                          encode kernel on the host (M = 150, K = 256: about 2.4 s on 8 cores, 34 ms at M = 10, K = 128 -- it pays
 *                          for itself after some 5e8 / 2.6e8 encoded rows); 0: handles created from now on get no tables and
 *                          encode on the kernels that evaluate every centroid (same codes)                                  */
int32_t pqhip_ctx_set_option(pqhip_ctx *ctx, const char *name, int64_t value);
/* Launch log of the calling thread: every kernel the library launches is noted by name; pqhip_launch_log() renders
 * "k_a + k_b x3 + ..." (distinct names in first-launch order with counts; valid until the thread's next call of
 * it), pqhip_launch_log_reset() clears it.  bench.py reports roofline.kernel from it.                            */
const char *pqhip_launch_log(void);
void pqhip_launch_log_reset(void);
/* Host only (no GPU needed): the candidate tables k_encode_vor2 uses for a codebook of 1- or 2-float sub-vectors, as built at
 * codebook creation (layout and the argument why the winner is always on a cell's list: reductive_amd/csrc/vor2_prep.h).
 * quantizers [M][K][dsub], dsub 1 or 2.  *n_words receives the number of 32-bit words; words_out (capacity words_cap, may be NULL to ask
 * for the size) the regions back to back, region_off_out [M + 1] their word offsets.  PQHIP_EUNSUPPORTED when the codebook
 * is not eligible (K > 256, non-finite or extreme centroids).  The CPU test-suite checks the tables against the oracle. */
int32_t pqhip_vor2_tables_host(const float *quantizers, int64_t M, int64_t K, int64_t dsub, uint32_t *words_out,
                               int64_t words_cap, uint32_t *region_off_out, int64_t *n_words);
/* name of the encode kernel the last device call on this codebook launched ("" if none)        */
const char *pqhip_last_encode_kernel(const pqhip_codebook *cb);

/* Self-test of the hardware property the MFMA path rests on: v_mfma_f32_32x32x2_f32 must equal
 * a k-ordered fmaf chain bit for bit.  Runs n_trials random 32x32xk tiles on device_slot;
 * *out_mismatches receives the number of differing elements. */
int32_t pqhip_selftest_mfma_chain(pqhip_ctx *ctx, int32_t device_slot, int32_t k, int32_t n_trials,
                                  uint64_t seed, int64_t *out_mismatches);

#ifdef __cplusplus
}
#endif
#endif /* PQHIP_H */
