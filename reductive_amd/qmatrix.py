"""A quantized embedding matrix kept resident in HBM: SURVEY.md 8f rank 3 (file / wire format -> direct
device upload) feeding rank 2 (lookup) and rank 4 (ADC scan).

The consumer of reductive's `Pq` -- finalfusion's quantized embedding storage -- is NOT in
/root/reference; its chunk layout is restated here from memory of finalfusion's public format
description, so this reader is UNPINNED by construction: no reference-held fixture exists for it and
none can be produced in this image (no Rust toolchain).  What is pinned is the in-tree surface it feeds
(`Pq::new` pq.rs:38-61, `projection()` :108-110, `subquantizers()` :191-193, `n_quantizer_centroids()`
:103-105) and the round trip through our own writer.

Storage chunk, little endian:
    u32 chunk identifier (4 = QuantizedArray; 3 is BucketSubwordVocab)     u64 chunk length in bytes (of what follows)
    u32 projection (0/1)   u32 norms (0/1)   u32 quantized_len M   u32 reconstructed_len d
    u32 n_centroids K      u64 n_embeddings N
    u32 quantized type id (1 = u8)   u32 reconstructed type id (10 = f32)
    zero padding up to a multiple of 4 bytes of the ABSOLUTE position in the file (the chunk follows the magic,
    the header chunk and usually a vocabulary chunk, so its start is not aligned in general: writer and reader take the
    position from f.tell(), or from `stream_offset` for streams that cannot tell)
    [d x d] f32 projection (if flagged)    [M x K x d/M] f32 quantizers
    [N] f32 norms (if flagged)             [N x M] u8 quantized embeddings
"""
import io
import struct

import numpy as np

from . import pq as _pq
from .pq import Pq, PanicError

CHUNK_QUANTIZED_ARRAY = 4
TYPE_U8, TYPE_F32 = 1, 10


class FormatError(ValueError):
    pass


def _position(f, stream_offset):
    """absolute position of the next byte of `f` in its file (f.tell() when the stream supports it)"""
    if stream_offset is not None:
        return stream_offset
    try:
        return f.tell()
    except (OSError, AttributeError, io.UnsupportedOperation):
        return 0


def write_chunk(f, pq, codes, norms=None, stream_offset=None):
    """Serialise (pq, codes [N, M] u8, norms [N] f32 or None) as one storage chunk at the stream's current position."""
    stream_offset = _position(f, stream_offset)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    M, K, dsub = pq.subquantizers().shape
    if codes.ndim != 2 or codes.shape[1] != M:
        raise PanicError("Quantization length does not match number of subquantizers")
    if norms is not None:
        norms = np.ascontiguousarray(norms, dtype=np.float32)
        if norms.shape != (codes.shape[0],):
            raise FormatError("one norm per embedding expected")
    P = pq.projection()
    head = struct.pack("<IIIIIQII", int(P is not None), int(norms is not None), M, M * dsub, K, codes.shape[0],
                       TYPE_U8, TYPE_F32)
    pad = (-(stream_offset + 12 + len(head))) % 4
    body = [head, b"\0" * pad]
    if P is not None:
        body.append(np.ascontiguousarray(P, dtype="<f4").tobytes())
    body.append(np.ascontiguousarray(pq.subquantizers(), dtype="<f4").tobytes())
    if norms is not None:
        body.append(norms.astype("<f4").tobytes())
    body.append(codes.tobytes())
    payload = b"".join(body)
    f.write(struct.pack("<IQ", CHUNK_QUANTIZED_ARRAY, len(payload)))
    f.write(payload)


def read_chunk(f, stream_offset=None, ctx=None):
    """Parse the storage chunk that starts at the stream's current position -> (Pq, codes [N, M] u8, norms [N] f32 or
    None); host arrays."""
    stream_offset = _position(f, stream_offset)
    def take(n):
        b = f.read(n)
        if len(b) != n:
            raise FormatError("truncated quantized-array chunk")
        return b
    ident, length = struct.unpack("<IQ", take(12))
    if ident != CHUNK_QUANTIZED_ARRAY:
        raise FormatError("not a quantized-array chunk (identifier %d)" % ident)
    proj, has_norms, M, d, K, N, qt, rt = struct.unpack("<IIIIIQII", take(36))
    if qt != TYPE_U8 or rt != TYPE_F32:
        raise FormatError("unsupported element types (%d, %d): u8 codes and f32 reconstructions only" % (qt, rt))
    if M == 0 or d == 0 or K == 0 or d % M != 0 or K > 256:
        raise FormatError("inconsistent quantizer shape M=%d d=%d K=%d" % (M, d, K))
    pad = (-(stream_offset + 12 + 36)) % 4
    take(pad)
    need = (d * d * 4 if proj else 0) + M * K * (d // M) * 4 + (N * 4 if has_norms else 0) + N * M
    if length != 36 + pad + need:
        raise FormatError("chunk length %d does not match its header (%d)" % (length, 36 + pad + need))
    P = np.frombuffer(take(d * d * 4), "<f4").reshape(d, d).astype(np.float32) if proj else None
    q = np.frombuffer(take(M * K * (d // M) * 4), "<f4").reshape(M, K, d // M).astype(np.float32)
    norms = np.frombuffer(take(N * 4), "<f4").astype(np.float32) if has_norms else None
    codes = np.frombuffer(take(N * M), np.uint8).reshape(N, M).copy()
    return Pq(P, q, ctx=ctx), codes, norms


def sort_ranges(lims, val, idx, descending=False):
    """Order every segment of a CSR range result by value: lims [nq + 1], val / idx flat (torch tensors, CPU or CUDA)
    -> (val, idx) with segment q, entries lims[q]:lims[q + 1], ascending in val (descending=True: descending); equal
    values keep the order they came in.  Two stable sorts: by value over all entries, then by segment."""
    import torch
    counts = lims[1:] - lims[:-1]
    seg = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=val.device), counts.to(val.device))
    by_val = torch.sort(val, stable=True, descending=descending).indices
    order = by_val[torch.sort(seg[by_val], stable=True).indices]
    return val[order], idx[order]


def _on_device(a, dev, dtype=None, host_dtype=None):
    """a host array (anything numpy converts, read as host_dtype) or a torch tensor -> a contiguous tensor on `dev`, of
    `dtype` if given"""
    import torch
    if not hasattr(a, "is_cuda"):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=host_dtype))
    return (a.to(dev) if dtype is None else a.to(dev, dtype)).contiguous()


def _positions(ids):
    """ids [N] (ids[p] = the original row stored at position p) -> positions [N], positions[ids[p]] = p"""
    import torch
    positions = torch.empty_like(ids)
    positions[ids] = torch.arange(ids.shape[0], dtype=torch.int64, device=ids.device)
    return positions


def _chunks(n, chunk=1 << 20):
    """the row ranges (r0, r1) the build steps work through: [0, n) in pieces of at most 2^20 rows"""
    return ((r0, min(n, r0 + chunk)) for r0 in range(0, n, chunk))


def _clone(matrix, names=None):
    """a new matrix of the class of `matrix` that shares its attributes: all it has set, or those of `names` it has set"""
    new = object.__new__(type(matrix))
    have = vars(matrix)
    new.__dict__.update(have if names is None else {name: have[name] for name in names if name in have})
    return new


def _device_rows(vectors, width, dev, what="vectors"):
    """vectors [B, width] (numpy or torch, any float dtype torch converts) -> float32 [B, width] on `dev`, contiguous"""
    import torch
    if len(vectors.shape) != 2 or vectors.shape[1] != width:
        raise PanicError("%s must be [B, %d]" % (what, width))
    return _on_device(vectors, dev, torch.float32, np.float32)


def _batch_norms(norms, has_norms, B, dev):
    """the norms= of an add(): required iff the matrix has norms -> float32 [B] on `dev`, or None"""
    import torch
    if (norms is not None) != has_norms:
        raise PanicError("norms are required for a matrix with norms and forbidden for one without")
    if norms is None:
        return None
    norms = _on_device(norms, dev, torch.float32, np.float32)
    if tuple(norms.shape) != (B,):
        raise PanicError("one norm per added vector expected")
    return norms


def _residual_codes_terms(residual_pq, rows, c, codes_out):
    """What a residual matrix stores for `rows` [n, d] f32 of the lists whose centroids are `c` [n, d] (device tensors):
    the codes of rows - c go to codes_out [n, M]; returns the query-free terms t_i = sum_j (r^_ij^2 + 2 c_ij r^_ij),
    accumulated in float64 and rounded once to f32.  The default route of _encode_residuals."""
    residual_pq.quantize_batch_device(rows - c, out=codes_out)
    r = residual_pq.reconstruct_batch_device(codes_out).double()
    return (r * r + 2.0 * c.double() * r).sum(1).float()


def _residual_codes_terms_device(residual_pq, rows, lists, centroids, codes_out, terms_out, buf):
    """_residual_codes_terms on the device route: `lists` int64 [n] and `centroids` [n_lists, d] on the device in the
    place of the gathered centroids.  The residuals go through residuals_device into buf[:n] (bit for bit rows - c), the
    codes to codes_out, and the terms come from residual_terms_device -- defined by its own fixed f64 order, not by
    torch's reduction -- into terms_out [n].  A quantizer with a projection keeps the torch tail, so its terms are
    those of _residual_codes_terms."""
    resid = residual_pq.residuals_device(rows, lists, centroids, out=buf[:rows.shape[0]])
    residual_pq.quantize_batch_device(resid, out=codes_out)
    if residual_pq.projection() is None:
        residual_pq.residual_terms_device(codes_out, lists, centroids, out=terms_out)
    else:
        r = residual_pq.reconstruct_batch_device(codes_out).double()
        terms_out.copy_((r * r + 2.0 * centroids[lists].double() * r).sum(1).float())


def _assign_device(coarse, n, rows_of_range, dev):
    """the nearest centroid of n rows -> int64 [n] on `dev`: the encode kernels of the one-subquantizer codebook
    `coarse` with a 4-byte index, in chunks of 2^20 rows; rows_of_range(r0, r1) gives the float32 device rows [r0, r1)"""
    import torch
    out = torch.empty((n, 1), dtype=torch.int32, device=dev)
    for r0, r1 in _chunks(n):
        coarse.quantize_batch_device(rows_of_range(r0, r1), out=out[r0:r1])
    return out[:, 0].long()


def _encode_residuals(residual_pq, n, rows_of_range, lists, centroids, device_terms):
    """What a residual matrix stores for n rows, in chunks of 2^20 rows -> (codes u8 [n, M], row terms f32 [n]) on the
    device: rows_of_range(r0, r1) gives the float32 device rows [r0, r1), `lists` int64 [n] the list of each row and
    `centroids` [n_lists, d] the device centroids; device_terms chooses _residual_codes_terms_device (through one
    residual buffer of a chunk's size) over _residual_codes_terms.  The loop of partition_residual and of encode()."""
    import torch
    dev = centroids.device
    codes = torch.empty((n, residual_pq.quantized_len()), dtype=torch.uint8, device=dev)
    terms = torch.empty(n, dtype=torch.float32, device=dev)
    buf = None
    if device_terms and n:
        buf = torch.empty((min(1 << 20, n), centroids.shape[1]), dtype=torch.float32, device=dev)
    for r0, r1 in _chunks(n):
        rows = rows_of_range(r0, r1)
        if device_terms:
            _residual_codes_terms_device(residual_pq, rows, lists[r0:r1], centroids, codes[r0:r1], terms[r0:r1], buf)
        else:
            terms[r0:r1] = _residual_codes_terms(residual_pq, rows, centroids[lists[r0:r1]], codes[r0:r1])
    return codes, terms


class _Refine:
    """Exact re-ranking against the original vectors, for all three matrix classes: `vectors` is an [N, d] device copy
    in ORIGINAL row order (None until attach_vectors), so the row numbers a search returns address it as they are."""

    vectors = None

    def attach_vectors(self, vectors, dtype=None):
        """Keep the original vectors ([N, d], numpy or torch, row i belonging to row i of the matrix this one was built
        from) on the device as `dtype` (torch.float32, the default, or torch.float16: half the memory and half the
        bytes a refinement reads, the elements rounded once here).  Enables `refine=` of nearest() / most_similar().
        Returns self."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float16):
            raise PanicError("vectors are kept as float32 or float16")
        if tuple(vectors.shape) != (len(self), self.pq.reconstructed_len()):
            raise PanicError("vectors must be [%d, %d]" % (len(self), self.pq.reconstructed_len()))
        self.vectors = _on_device(vectors, self.codes.device, dtype)
        return self

    def _check_refine(self, k, refine):
        if self.vectors is None:
            raise PanicError("refine needs the original vectors: call attach_vectors first")
        if not k <= int(refine) <= 1024:
            raise PanicError("refine must lie between k and 1024, was %d (k = %d)" % (refine, k))
        return int(refine)

    def _refined(self, queries, rows, k, ip):
        """rows: the original row numbers of the candidates ([R] or [nq, R], -1 = padding), on the device"""
        return self.pq.rerank_device(queries, self.vectors, rows, k, ip=ip)

    def _exact_words(self, allow):
        """`allow=` of an exact search -> the mask words in ORIGINAL row order (the order of `vectors`) or None"""
        import torch
        if allow is None:
            return None
        if isinstance(allow, RowFilter):
            if allow.matrix is not self:
                raise PanicError("the row filter was built for another matrix")
            if getattr(self, "ids", None) is not None:
                raise PanicError("the row filter of a partitioned matrix is in position order: give the flags of all rows")
            return allow.words
        allow = _on_device(allow, self.vectors.device)
        if allow.dtype != torch.bool or tuple(allow.shape) != (len(self),):
            raise PanicError("allow must be a bool array with one flag per row (%d)" % len(self))
        return self.pq.pack_row_mask_device(allow.view(torch.uint8))

    _max_abs = None           # (key of the vectors it was taken from, their largest |element|)

    def _screen_x_exp(self):
        """x_exp of the matrix-core screen for `vectors` (pq.flat_screen_x_exp of their largest |element|, which is
        reduced once and kept until the tensor is replaced or written)"""
        v = self.vectors
        key = (v.data_ptr(), tuple(v.shape), v.dtype, v._version)
        if self._max_abs is None or self._max_abs[0] != key:
            self._max_abs = (key, _pq._matrix_max_abs(v))
        return _pq.flat_screen_x_exp(self._max_abs[1])

    def _screens(self, screen):
        """screen=True takes the batch route where the screen serves the width; wider vectors keep the plain call"""
        return bool(screen) and self.vectors.shape[1] <= _pq.FLAT_SCREEN_MAX_D

    def _flat_topk(self, q, k, ip, words, screen):
        if self._screens(screen):
            return self.pq.flat_search_batch_device(q, self.vectors, k, ip=ip, allow=words, x_exp=self._screen_x_exp())
        return self.pq.flat_search_device(q, self.vectors, k, ip=ip, allow=words)

    def _flat_range(self, q, threshold, ip, words, screen):
        if self._screens(screen):
            return self.pq.flat_range_batch_device(q, self.vectors, threshold, ip=ip, allow=words, x_exp=self._screen_x_exp())
        return self.pq.flat_range_device(q, self.vectors, threshold, ip=ip, allow=words)

    def _exact(self, ip, queries, k, allow, screen=False):
        import torch
        if self.vectors is None:
            raise PanicError("refine needs the original vectors: call attach_vectors first")
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        return self._flat_topk(q, k, ip, self._exact_words(allow), screen)

    def exact_nearest(self, queries, k, allow=None, screen=False):
        """The true k nearest rows: the exhaustive top-k of ALL attached vectors by their exact squared distance
        (Pq.flat_search_device), in original row numbers, ties to the smaller row -> (dist, idx) [k] or [nq, k].  The
        codes are not read: this is the ground truth the quantized searches are measured against, and dist are the
        values refine= returns.  allow: None, bool flags [N] in original row order, or (QuantizedMatrix) a RowFilter of
        this matrix; a partitioned matrix's RowFilter is in position order and is refused.  screen=True: the route for
        query batches (Pq.flat_search_batch_device: matrix-core screen, exact resolve), the same result bit for bit;
        vectors wider than 2,048 elements keep the plain call."""
        return self._exact(False, queries, k, allow, screen)

    def exact_most_similar(self, queries, k, allow=None, screen=False):
        """The true k rows of largest inner product with the attached vectors as they are, largest first -> (score, idx),
        as exact_nearest()."""
        return self._exact(True, queries, k, allow, screen)

    def _exact_range(self, ip, queries, threshold, allow, sort, screen=False):
        import torch
        if self.vectors is None:
            raise PanicError("refine needs the original vectors: call attach_vectors first")
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        lims, val, rows = self._flat_range(q, threshold, ip, self._exact_words(allow), screen)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows

    def exact_within(self, queries, radius, allow=None, sort=False, screen=False):
        """The true answer of within(): EVERY attached vector whose exact squared distance to the query is <= radius (a
        scalar or one value per query) -> (lims, dist, idx), CSR over the queries in ascending original row number
        (Pq.flat_range_device); sort=True: ascending in distance, ties in row order.  The codes are not read: this is
        what the recall of within() is measured against, and the one way to true distances for a radius query (refine=
        stops at 1,024 candidates).  allow: as for exact_nearest().  screen=True: the route for query batches
        (Pq.flat_range_batch_device), the same result bit for bit."""
        return self._exact_range(False, queries, radius, allow, sort, screen)

    def exact_similar_above(self, queries, threshold, allow=None, sort=False, screen=False):
        """Every attached vector whose exact inner product with the query is >= threshold -> (lims, score, idx), as
        exact_within(); sort=True: descending in score."""
        return self._exact_range(True, queries, threshold, allow, sort, screen)

    def _exact_among(self, ip, queries, rows, k):
        import torch
        if self.vectors is None:
            raise PanicError("refine needs the original vectors: call attach_vectors first")
        lims, rows = _Among._among_rows(self, rows)
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        return self.pq.flat_among_device(q, self.vectors, rows, k, lims=lims, ip=ip)

    def exact_nearest_among(self, queries, rows, k):
        """exact_nearest() among the rows that `rows` names and no others -- what nearest_among() takes: a vector of
        ORIGINAL row numbers shared by all queries, or the pair (lims, rows) that within() / similar_above() return ->
        (dist, idx) [k] or [nq, k]: the k nearest of them by their exact squared distance to the attached vectors, in
        original row numbers on every class, ties to the smaller row, index -1 and +Inf past the last
        (Pq.flat_among_device).  Any number of rows per query: this is the re-ranking of a shortlist longer than the 1,024
        candidates of refine=, e.g. m.exact_nearest_among(q, m.within(q, r)[::2], k).  -1 is padding, any other number
        outside [0, N) is skipped; a row named twice may come back twice.  For distinct rows the result is
        exact_nearest(queries, k, allow=<flags of the rows>) at the cost of the named rows alone."""
        return self._exact_among(False, queries, rows, k)

    def exact_most_similar_among(self, queries, rows, k):
        """exact_most_similar() among the rows that `rows` names -> (score, idx), largest first, as
        exact_nearest_among()."""
        return self._exact_among(True, queries, rows, k)

    def _exact_range_among(self, ip, queries, rows, threshold, sort):
        import torch
        if self.vectors is None:
            raise PanicError("refine needs the original vectors: call attach_vectors first")
        lims, rows = _Among._among_rows(self, rows)
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        lims, val, rows = self.pq.flat_range_among_device(q, self.vectors, rows, threshold, lims=lims, ip=ip)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows

    def exact_within_among(self, queries, rows, radius, sort=False):
        """exact_within() among the rows that `rows` names (as for exact_nearest_among) -> (lims, dist, idx): of every
        query's rows those whose exact squared distance is <= radius (a scalar or one value per query), in the order in
        which they were named, in original row numbers on every class (Pq.flat_range_among_device); sort=True: ascending
        in distance.  It verifies a radius query over the codes against the stored vectors at the cost of the rows
        that query returned:
            m.exact_within_among(q, m.within(q, r + slack)[::2], r)
        is exact_within(q, r) restricted to the rows within(q, r + slack) found.  A row named twice is returned twice."""
        return self._exact_range_among(False, queries, rows, radius, sort)

    def exact_similar_above_among(self, queries, rows, threshold, sort=False):
        """exact_similar_above() among the rows that `rows` names -> (lims, score, idx), as exact_within_among():
            m.exact_similar_above_among(q, m.similar_above(q, t - slack)[::2], t)
        sort=True: descending in score."""
        return self._exact_range_among(True, queries, rows, threshold, sort)


class RowFilter:
    """The set of rows a search may return, packed for one matrix: `words` is the device mask of the searches' `allow=`
    (int32 [ceil(N / 32)], bit p of the matrix's own row order -- position order for a partitioned matrix), `matrix` the
    matrix it was built for (row_filter of that matrix; using it on another raises PanicError), `n_allowed` the number of
    allowed rows.  A filter is rebuilt from its N flags; there are no in-place updates."""

    def __init__(self, matrix, words, n_allowed):
        self.matrix = matrix
        self.words = words
        self.n_allowed = n_allowed


class _Filter:
    """Row filters for all three matrix classes.  Flags are given in ORIGINAL row order; a partitioned matrix packs them
    through its permutation, bit p = allow[ids[p]] (Pq.pack_row_mask_device with perm = ids)."""

    def row_filter(self, allow=None, rows=None, allowed=True):
        """allow: bool [N] (numpy or torch), True = the row may be returned, in original row order; or rows=: original
        row numbers with allowed=True (only these rows may be returned) or allowed=False (these rows are excluded --
        deleted rows, a skip set -- and every other row may be returned) -> RowFilter for `allow=` of nearest() /
        most_similar() of THIS matrix.  partition() / partition_residual() do not carry filters over: build the filter
        from the same flags on the partitioned matrix."""
        import torch
        N, dev = len(self), self.codes.device
        if (allow is None) == (rows is None):
            raise PanicError("give either the flags of all rows or a list of row numbers")
        if rows is not None:
            r = _on_device(rows, dev, torch.int64, np.int64).reshape(-1)
            if r.numel() and (int(r.min()) < 0 or int(r.max()) >= N):
                raise PanicError("row numbers must lie in [0, %d)" % N)
            flags = torch.full((N,), 0 if allowed else 1, dtype=torch.uint8, device=dev)
            flags[r] = 1 if allowed else 0
        else:
            allow = _on_device(allow, dev)
            if allow.dtype != torch.bool or tuple(allow.shape) != (N,):
                raise PanicError("allow must be a bool array with one flag per row (%d)" % N)
            flags = allow.view(torch.uint8)
        words = self.pq.pack_row_mask_device(flags, perm=getattr(self, "ids", None))
        return RowFilter(self, words, int(flags.count_nonzero()))

    def _allow_words(self, allow):
        """`allow=` of a search -> the mask words or None: a RowFilter of this matrix, or flags packed on the spot"""
        if allow is None:
            return None
        if isinstance(allow, RowFilter):
            if allow.matrix is not self:
                raise PanicError("the row filter was built for another matrix")
            return allow.words
        return self.row_filter(allow).words


def _compact_arrays(pq, words, n, arrays, list_off=None, want_src_rows=False):
    """The kept rows of each of `arrays` (device tensors of n rows, or None) under the mask words `words`, through
    Pq.compact_rows_device: one plan-only call for the count (the offsets of the compacted lists, the numbers of the kept
    rows), then one moving call per array into exactly that many rows -> (outs, list_off_out or None, src_rows or None)"""
    _, off, src, c = pq.compact_rows_device(words, None, list_off=list_off, want_src_rows=want_src_rows, n=n, check=True)
    outs = [None if a is None else pq.compact_rows_device(words, a, capacity=c)[0] for a in arrays]
    return outs, off, src


class _Compact:
    """Removing rows, for all three matrix classes: compact() / remove() return a NEW matrix that holds the kept rows
    alone -- tensor for tensor what the class's constructor builds from them in their original order -- and the old
    row number of every new row.  Every per-row array is compacted on the device (Pq.compact_rows_device); nothing of
    length N goes to the host or through a sort.  Row filters are not carried over: `kept` is what a caller needs to
    rebuild one.  self and its filters stay as they are.  A packed matrix moves its packed rows as they are."""

    def _keep_words(self, allow):
        words = self._allow_words(allow)
        if words is None:
            raise PanicError("compact() takes a row filter of this matrix or the flags of all rows")
        return words

    def _compact_vectors(self, words, kept):
        """the attached vectors (original row order) under the original-order mask, in their dtype"""
        v = self.vectors
        if v is None:
            return None
        if v.shape[1] * v.element_size() > 4096:
            return v[kept].contiguous()
        return self.pq.compact_rows_device(words, v, capacity=kept.shape[0])[0]

    def remove(self, rows):
        """compact() of the filter that excludes the ORIGINAL row numbers `rows` (numpy or torch; a number outside
        [0, N) raises PanicError, as row_filter(rows=.., allowed=False) does) -> (new_matrix, kept)."""
        return self.compact(self.row_filter(rows=rows, allowed=False))


class _Packed4:
    """4-bit packed codes for all three matrix classes (quantizers of at most 16 centroids): pack4() gives a matrix of
    the same class whose `codes` hold two codes per byte, [N, ceil(M / 2)] (include/pqhip.h, "4-bit packed codes"), at
    half the bytes in HBM and per search.  nearest() and most_similar() with every option, embeddings(), row_filter(),
    attach_vectors() and growth work on it and return exactly what the unpacked matrix returns; the range searches, the
    full scans and the partitioning do not read packed codes and raise PanicError: call unpack4() first."""

    packed4 = False

    def _with_codes(self, codes, packed4):
        new = _clone(self)      # norms, ids, positions, lists, row terms, centroids, vectors: shared
        new.codes = codes
        new.packed4 = packed4
        return new

    def pack4(self):
        """The same matrix with 4-bit packed codes -> a NEW matrix of this class (self if it is packed already) that
        shares every other tensor with self; row filters are not carried over (row_filter on the result).  PanicError
        for a quantizer of more than 16 centroids."""
        if self.packed4:
            return self
        return self._with_codes(self.pq.pack_codes4_device(self.codes), True)

    def unpack4(self):
        """The inverse of pack4(): one byte per code again -> a NEW matrix (self if it is not packed)."""
        if not self.packed4:
            return self
        return self._with_codes(self.pq.unpack_codes4_device(self.codes), False)

    def _unpacked_only(self, what):
        if self.packed4:
            raise PanicError("%s() does not read 4-bit packed codes: call unpack4() first" % what)

    def _stored_codes(self, codes):
        """the codes of a batch ([B, M] u8) as this matrix stores them"""
        return self.pq.pack_codes4_device(codes) if self.packed4 else codes

    def _reconstruct_rows(self, pos, scales=None, out=None):
        """reconstruct_rows_device of the stored rows `pos`; a packed matrix unpacks the selected rows first"""
        import torch
        if not self.packed4:
            return self.pq.reconstruct_rows_device(self.codes, pos, scales=scales, out=out)
        if pos.shape[0] == 0:
            return out if out is not None else torch.empty((0, self.pq.reconstructed_len()), dtype=torch.float32, device=pos.device)
        codes = self.pq.unpack_codes4_device(self.codes, rows=pos, check=True)
        sel = torch.arange(pos.shape[0], dtype=torch.int64, device=pos.device)
        return self.pq.reconstruct_rows_device(codes, sel, scales=None if scales is None else scales[pos].contiguous(), out=out)


class _Search:
    """The top-k and the range search of all three matrix classes: one body each.  A class says what is its own in one
    hook, _search_terms(ip, ranged, queries, nprobe) -> (the Pq method that serves the call, the tables it reads, the
    arguments it takes between the tables and k or the threshold: none, the lists and probes, or those with the bias
    of every probe and the row terms), and in _original_rows, which turns what the kernel returns into row numbers."""

    def _tables(self, ip, queries):
        return self.pq.adc_ip_tables_device(queries) if ip else self.pq.adc_tables_device(queries)

    def _original_rows(self, pos):
        """the unpartitioned matrix stores rows under their numbers"""
        return pos

    def _topk(self, ip, queries, k, nprobe, use_norms, refine, allow):
        R = k if refine is None else self._check_refine(k, refine)
        fn, tables, more = self._search_terms(ip, False, queries, nprobe)
        kw = {"scales": self.norms if use_norms else None} if ip else {}
        val, pos = fn(self.codes, tables, *more, R, allow=self._allow_words(allow), packed4=self.packed4, **kw)
        rows = self._original_rows(pos)
        return (val, rows) if refine is None else self._refined(queries, rows, k, ip)

    def _range(self, ip, queries, threshold, nprobe, use_norms, allow, sort):
        self._unpacked_only("similar_above" if ip else "within")
        fn, tables, more = self._search_terms(ip, True, queries, nprobe)
        kw = {"scales": self.norms if use_norms else None} if ip else {}
        lims, val, pos = fn(self.codes, tables, *more, threshold, allow=self._allow_words(allow), **kw)
        rows = self._original_rows(pos)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows


class _Among:
    """Searches among given rows for all three matrix classes: nearest_among() / most_similar_among() rank exactly the
    rows the caller names (Pq.adc_among_device / adc_ip_among_device) -- a tenant's rows, the result of a range search,
    a shortlist from another index -- and read no other row.  Not served on a packed matrix: unpack4() first."""

    def _among_rows(self, rows):
        """rows= -> (lims or None, row numbers): one int64 vector shared by all queries, or the pair (lims, rows) that
        within() / similar_above() return; numpy or torch, brought to the device of the codes"""
        import torch
        dev = self.codes.device

        def vector(t, what):
            host = not hasattr(t, "is_cuda")
            if host:
                t = np.asarray(t)
                if t.dtype.kind not in "iu":
                    raise PanicError("%s must be integers" % what)
            if len(t.shape) != 1 or not host and (t.is_floating_point() or t.dtype == torch.bool):
                raise PanicError("%s must be a vector of integers" % what)
            return _on_device(t, dev, torch.int64, np.int64)

        if isinstance(rows, tuple):
            if len(rows) != 2:
                raise PanicError("rows must be a vector of row numbers or the pair (lims, rows)")
            return vector(rows[0], "lims"), vector(rows[1], "rows")
        return None, vector(rows, "rows")

    def _among_ids(self, rows):
        """original row numbers -> what the kernel is given; the unpartitioned matrix stores rows under their numbers"""
        return rows

    def _among_terms(self, ip, queries):
        """-> (tables, the keyword arguments that place a row in a list); the residual class names its lists here"""
        return self._tables(ip, queries), {}

    def _among(self, ip, queries, rows, k, use_norms, refine, check):
        self._unpacked_only("most_similar_among" if ip else "nearest_among")
        R = k if refine is None else self._check_refine(k, refine)
        lims, rows = self._among_rows(rows)
        tables, kw = self._among_terms(ip, queries)
        if ip:
            kw["scales"] = self.norms if use_norms else None
        fn = self.pq.adc_ip_among_device if ip else self.pq.adc_among_device
        val, pos = fn(self.codes, tables, self._among_ids(rows), R, lims=lims, check=check, **kw)
        rows = self._original_rows(pos)
        return (val, rows) if refine is None else self._refined(queries, rows, k, ip)

    def nearest_among(self, queries, rows, k, refine=None, check=False):
        """nearest() among the rows that `rows` names and no others: a vector of ORIGINAL row numbers shared by all
        queries, or the pair (lims, rows) -- the rows of query q are rows[lims[q]:lims[q + 1]], exactly what within() /
        similar_above() return -> (dist, idx) [k] or [nq, k], the k nearest of them, ties to the smaller row (a
        partitioned matrix: to the smaller position in list order), index -1 and +Inf past the last.  -1 is padding; any
        other number outside [0, N) is skipped (check=True: the reference's index panic); a row named twice may come
        back twice.  For distinct rows the result is nearest(queries, k, allow=<flags of the rows>) -- with all lists
        probed on a partitioned matrix -- at the cost of the named rows alone.  refine=R: as for nearest()."""
        return self._among(False, queries, rows, k, True, refine, check)

    def most_similar_among(self, queries, rows, k, use_norms=True, refine=None, check=False):
        """most_similar() among the rows that `rows` names (as for nearest_among) -> (score, idx), largest first."""
        return self._among(True, queries, rows, k, use_norms, refine, check)


class QuantizedMatrix(_Refine, _Filter, _Packed4, _Search, _Among, _Compact):
    """Codes (+ norms) resident in HBM next to the device codebook: the lookup, scan and similarity-search consumer."""

    def __init__(self, pq, codes, norms=None, device="cuda:0"):
        import torch
        self.pq = pq
        self.codes = torch.as_tensor(np.ascontiguousarray(codes, dtype=np.uint8)).to(device)
        self.norms = None if norms is None else torch.as_tensor(np.ascontiguousarray(norms, dtype=np.float32)).to(device)
        if self.codes.dim() != 2 or self.codes.shape[1] != pq.quantized_len():
            raise PanicError("Quantization length does not match number of subquantizers")

    @classmethod
    def load(cls, path_or_file, device="cuda:0", ctx=None):
        """file -> device: header on the host, the three payload arrays straight into device tensors."""
        f = open(path_or_file, "rb") if isinstance(path_or_file, str) else path_or_file
        try:
            pq, codes, norms = read_chunk(f, ctx=ctx)
        finally:
            if isinstance(path_or_file, str):
                f.close()
        return cls(pq, codes, norms, device=device)

    def __len__(self):
        return self.codes.shape[0]

    def embeddings(self, rows, out=None):
        """`reconstruct_batch(codes.select(Axis(0), rows)) * norms.select(rows)` in one pass over HBM."""
        import torch
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.codes.device)
        return self._reconstruct_rows(rows, scales=self.norms, out=out)

    def distances(self, queries):
        """asymmetric squared distances of the query vector(s) to every (un-normalised) code row.  Not served on a
        packed matrix: unpack4() first."""
        self._unpacked_only("distances")
        return self.pq.adc_scan_device(self.codes, self.pq.adc_tables_device(queries))

    def inner_products(self, queries, use_norms=True):
        """inner products of the query vector(s) with every row: the scan over the inner-product tables, times the
        stored norms when use_norms (and the matrix has them) -> [n] or [nq, n].  Not served on a packed matrix:
        unpack4() first."""
        self._unpacked_only("inner_products")
        ip = self.pq.adc_scan_device(self.codes, self.pq.adc_ip_tables_device(queries))
        if use_norms and self.norms is not None:
            ip = ip * self.norms
        return ip

    def _search_terms(self, ip, ranged, queries, nprobe):
        pq = self.pq
        if ip:
            fn = pq.adc_ip_range_device if ranged else pq.adc_ip_search_device
        else:
            fn = pq.adc_range_device if ranged else pq.adc_search_device
        return fn, self._tables(ip, queries), ()

    def nearest(self, queries, k, refine=None, allow=None):
        """the k rows of smallest asymmetric squared distance (adc_search_device over all rows), ties to the smaller
        row -> (dist, idx) [k] or [nq, k].  refine=R (k <= R <= 1024, vectors attached): the R nearest rows by that
        estimate are re-ranked by their exact squared distance to the attached vectors (Pq.rerank_device) on the
        device; dist are then the exact distances.  allow: None, a RowFilter of this matrix (row_filter) or a bool
        array [N] packed on the spot -- only allowed rows are ranked, exactly as if the others were not stored (index
        -1 past the last allowed row); with refine= the shortlist holds allowed rows only."""
        return self._topk(False, queries, k, None, True, refine, allow)

    def most_similar(self, queries, k, use_norms=True, refine=None, allow=None):
        """the k rows of largest inner product with what embeddings() returns (the stored vectors, unscaled, with
        use_norms=False or without norms), largest first, ties to the smaller row -> (score, idx) [k] or [nq, k].
        refine=R (k <= R <= 1024, vectors attached): the R most similar rows by that estimate are re-ranked by their
        exact inner product with the attached vectors as they are; use_norms then only affects the candidate stage.
        allow: as for nearest()."""
        return self._topk(True, queries, k, None, use_norms, refine, allow)

    def within(self, queries, radius, allow=None, sort=False):
        """EVERY row whose asymmetric squared distance to the query is <= radius (a scalar or one value per query) ->
        (lims, dist, idx): CSR over the queries, lims int64 [nq + 1] ([2] for one query), the rows of query q at
        lims[q]:lims[q + 1] in ascending row number (Pq.adc_range_device; the result is allocated to its size, after one
        read of the count).  sort=True: each query's rows ascending in distance instead, ties in row order
        (sort_ranges).  allow: as for nearest().  There is no refine=: re-ranking is defined for at most 1,024
        candidates per query, and a range result has no such bound.  Not served on a packed matrix: unpack4() first."""
        return self._range(False, queries, radius, None, True, allow, sort)

    def similar_above(self, queries, threshold, use_norms=True, allow=None, sort=False):
        """Every row whose inner product with the query, as most_similar() scores it, is >= threshold (a scalar or one
        value per query) -> (lims, score, idx), CSR as for within() (Pq.adc_ip_range_device).  sort=True: each query's
        rows descending in score, ties in row order.  No refine=, as for within().  Not served on a packed matrix:
        unpack4() first."""
        return self._range(True, queries, threshold, None, use_norms, allow, sort)

    def add(self, vectors, norms=None):
        """The matrix with the rows of `vectors` ([B, d] float32, numpy or CUDA) appended as rows len(self) .. len(self) +
        B - 1 -> a NEW QuantizedMatrix; self is left as it is (and so are the row filters built for it, which the new
        matrix refuses).  The codes are quantize_batch_device of the vectors; norms [B] is required iff the matrix has
        norms.  Attached vectors are extended by the new ones in the attached dtype.  A packed matrix packs the new codes:
        m.pack4().add(x) is m.add(x).pack4()."""
        import torch
        dev = self.codes.device
        x = _device_rows(vectors, self.pq.reconstructed_len(), dev)
        nb = _batch_norms(norms, self.norms is not None, x.shape[0], dev)
        new = _clone(self, ("pq", "packed4"))
        codes = self._stored_codes(self.pq.quantize_batch_device(x)) if x.shape[0] else self.codes[:0]
        if codes.dtype != self.codes.dtype:
            raise PanicError("the matrix holds 1-byte codes")
        new.codes = torch.cat([self.codes, codes])
        new.norms = None if nb is None else torch.cat([self.norms, nb])
        if self.vectors is not None:
            new.vectors = torch.cat([self.vectors, x.to(self.vectors.dtype)])
        return new

    def compact(self, allow):
        """The matrix of the rows that `allow` keeps (a RowFilter of this matrix, or a bool array [N]) -> (new_matrix,
        kept): a NEW QuantizedMatrix with codes[kept] and norms[kept], and kept, int64 [N'] on the device, the old row
        number of new row i, ascending.  Attached vectors are compacted in their dtype.  For any search S,
        new.S(q, ..) is self.S(q, .., allow=allow) with the indices mapped through kept."""
        words = self._keep_words(allow)
        new = _clone(self, ("pq", "packed4"))
        (new.codes, new.norms), _, kept = _compact_arrays(self.pq, words, len(self), (self.codes, self.norms), want_src_rows=True)
        if self.vectors is not None:
            new.vectors = self._compact_vectors(words, kept)
        return new, kept

    def partition(self, n_lists, n_iterations=10, vectors=None, train_rows=None, rng=None, on_device=False):
        """Partition the rows with a coarse k-means quantizer of n_lists centroids -> PartitionedMatrix (IVFADC without
        residual encoding: the codes stay the codes of the vectors themselves).

        The coarse quantizer is trained on `vectors` ([N, d] float32, numpy or CUDA, row i belonging to code row i) if
        given, else on the reconstructions of the stored codes (reconstruct_batch_device, without the norms), so a
        matrix loaded from a storage chunk can be partitioned without the original embeddings.  train_rows: train on
        that many distinct rows drawn with `rng` instead of all of them (every row is assigned either way).  Initial
        centroids are n_lists distinct training rows drawn with the numpy Generator `rng`, as train_pq draws them;
        training is kmeans_iterations with one subquantizer, assignment is cluster_assignments.  Both take the slow
        anchor kernel for sub-vectors wider than 256 floats: accepted for a build step.  1 <= n_lists <= 16384 (the
        k-means limit) and n_lists <= number of training rows.  Row filters are not carried over: a RowFilter belongs
        to the matrix that built it (call row_filter on the result).  Not served on a packed matrix: unpack4() first.

        on_device=True: the same training and the same draws from `rng`, but the rows are assigned by the coarse
        codebook's quantize_batch_device (as _Lists.assign does) and laid out by Pq.lists_layout_device: no array of
        length N goes to the host.  The result equals that of the default route tensor for tensor (ids, list_off,
        positions, codes, norms, centroids)."""
        self._unpacked_only("partition")
        rng = rng or np.random.default_rng(0)
        centroids, assign, _, _ = self._coarse_partition(n_lists, n_iterations, vectors, train_rows, rng, on_device)
        out = PartitionedMatrix(self, centroids, assign)
        out.vectors = self.vectors           # attached vectors stay in original row order: handed on as they are
        return out

    def _coarse_partition(self, n_lists, n_iterations, vectors, train_rows, rng, on_device=False):
        """The part partition() and partition_residual() share: trains the coarse quantizer and assigns every row ->
        (centroids [n_lists, d] f32, assign [N] int64, rows_of, train_sel): rows_of(sel) gives the float32 device rows
        the partition is built from, train_sel the training rows (a slice or sorted row numbers).  Draws from rng:
        the training rows (if fewer than all), then the initial centroids.  assign is a numpy array, or with on_device
        a device tensor (_assign_device: the rows never leave the device)."""
        import torch
        from .pq import ReductiveError, cluster_assignments, kmeans_iterations
        N, d = len(self), self.pq.reconstructed_len()
        if not 1 <= n_lists <= 16384:
            raise ReductiveError("The number of lists must be between 1 and 16384, was %d" % n_lists)
        if on_device and not self.codes.is_cuda:
            raise PanicError("on_device=True needs a matrix that is resident on a GPU")

        def rows_of(sel):
            """float32 [len(sel), d] on the device: the given vectors or the reconstructions of the code rows `sel`"""
            if vectors is None:
                if not isinstance(sel, slice):
                    sel = torch.as_tensor(sel, dtype=torch.int64, device=self.codes.device)
                return self.pq.reconstruct_batch_device(self.codes[sel])
            return _on_device(vectors[sel], self.codes.device, torch.float32, np.float32)

        if vectors is not None and tuple(vectors.shape) != (N, d):
            raise PanicError("vectors must be [%d, %d]" % (N, d))
        n_train = N if train_rows is None else min(int(train_rows), N)
        if n_lists > n_train:
            raise ReductiveError("The number of lists (%d) exceeds the number of training rows (%d)" % (n_lists, n_train))
        train_sel = slice(0, N) if n_train == N else np.sort(rng.choice(N, n_train, replace=False))
        train = rows_of(train_sel)
        init = train[torch.as_tensor(rng.choice(n_train, n_lists, replace=False), device=train.device)].cpu().numpy()
        centroids, _ = kmeans_iterations(init[None], train, n_iterations, want_loss=False, ctx=self.pq._ctx)
        centroids = np.ascontiguousarray(centroids[0])
        del train
        if on_device:
            coarse = Pq(None, centroids[None], ctx=self.pq._ctx)
            assign = _assign_device(coarse, N, lambda r0, r1: rows_of(slice(r0, r1)), self.codes.device)
            return centroids, assign, rows_of, train_sel
        assign = np.empty(N, np.int64)
        for r0, r1 in _chunks(N):
            assign[r0:r1] = cluster_assignments(centroids, rows_of(slice(r0, r1)).cpu().numpy(), ctx=self.pq._ctx)
        return centroids, assign, rows_of, train_sel

    def partition_residual(self, n_lists, n_subquantizers=None, n_subquantizer_bits=None, n_iterations=10,
                           pq_iterations=10, n_attempts=1, vectors=None, train_rows=None, residual_pq=None, rng=None,
                           on_device=False):
        """Partition the rows as partition() does (the same coarse training, the same draws from `rng`, the same
        assignment) and re-encode them as residuals -> ResidualPartitionedMatrix (IVFADC with residual encoding).

        Row i of list l is stored as the code of vectors[i] - centroids[l], formed on the device in f32; `vectors`
        defaults to the reconstructions of the stored codes, as in partition().  The residual quantizer is trained with
        train_pq (pq_iterations, n_attempts, draws from `rng` after the coarse ones) on the residuals of the training
        rows; n_subquantizers and n_subquantizer_bits default to those of self.pq (at most 8 bits: the list searches
        read 1-byte codes); a given `residual_pq` (a Pq of the same width, OPQ allowed) skips the training.  All
        residuals are encoded with quantize_batch_device, in chunks, and every row gets its query-free term
        t_i = sum_j (r^_ij^2 + 2 c_lj r^_ij), r^ = reconstruct_batch_device of the residual quantizer, accumulated in
        float64 on the device and rounded once to f32.  The norms are kept as they are.  Row filters are not carried
        over (row_filter on the result builds one from the same flags).  Not served on a packed matrix: unpack4() first.

        on_device=True: assignment and layout as partition(on_device=True); the residuals are formed by
        Pq.residuals_device (bit for bit rows - centroids[assign]) and the row terms by Pq.residual_terms_device, which
        reads the codebook entries instead of a reconstruction.  Only the training rows go to the host (train_pq).  The
        result equals that of the default route in everything except row_terms: the device terms are defined by the
        fixed f64 order of pqhip_residual_terms_f32_dev, not by torch's reduction, and agree with the default route's
        within 2^-23 |t| + 2^-40 sum_j (r^2 + |2 c r|); searches over the two may differ where two rows tie to the
        last bit.  A residual quantizer with a projection keeps the torch tail (its terms then equal the default
        route's).  The matrix carries device_terms = True, so add() / encode() compute the terms of new rows the same way."""
        import torch
        from .pq import ReductiveError, train_pq
        self._unpacked_only("partition_residual")
        rng = rng or np.random.default_rng(0)
        N, d = len(self), self.pq.reconstructed_len()
        M = self.pq.quantized_len() if n_subquantizers is None else int(n_subquantizers)
        bits = n_subquantizer_bits
        if bits is None:
            bits = max(1, int(self.pq.n_quantizer_centroids() - 1).bit_length())
        if residual_pq is None and bits > 8:
            raise ReductiveError("The residual codes are 1-byte codes: at most 8 subquantizer bits, was %d" % bits)
        if residual_pq is not None and (residual_pq.reconstructed_len() != d or residual_pq.n_quantizer_centroids() > 256):
            raise PanicError("the residual quantizer must reconstruct %d columns from 1-byte codes" % d)
        centroids, assign, rows_of, train_sel = self._coarse_partition(n_lists, n_iterations, vectors, train_rows, rng,
                                                                       on_device)
        dev = self.codes.device
        cd = torch.from_numpy(centroids).to(dev)
        ad = assign if on_device else torch.from_numpy(assign).to(dev)
        if residual_pq is None:
            sel = train_sel if isinstance(train_sel, slice) else torch.from_numpy(train_sel).to(dev)
            if on_device:
                resid = self.pq.residuals_device(rows_of(train_sel), ad[sel].contiguous(), cd)
            else:
                resid = rows_of(train_sel) - cd[ad[sel]]
            residual_pq = train_pq(M, int(bits), pq_iterations, n_attempts, resid.cpu().numpy(), rng=rng, ctx=self.pq._ctx)
            del resid
        codes, terms = _encode_residuals(residual_pq, N, lambda r0, r1: rows_of(slice(r0, r1)), ad, cd, on_device)
        out = ResidualPartitionedMatrix(residual_pq, codes, self.norms, terms, centroids, assign)
        out.device_terms = bool(on_device)
        out.vectors = self.vectors
        return out


def ivf_layout(assign, n_lists):
    """assign [N] list id per row -> (perm, list_off): perm = the stable argsort of the assignments, so list l is
    positions [list_off[l], list_off[l + 1]) of the permuted rows and positions inside a list ascend in original row
    number; list_off [n_lists + 1] = prefix sums of the list sizes (empty lists are legal).  Pure numpy."""
    a = np.asarray(assign)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("assign must be a vector of integer list ids")
    if n_lists < 0 or (a.size and (int(a.min()) < 0 or int(a.max()) >= n_lists)):
        raise ValueError("list ids must lie in [0, %d)" % n_lists)
    perm = np.argsort(a, kind="stable").astype(np.int64)
    list_off = np.zeros(n_lists + 1, np.int64)
    np.cumsum(np.bincount(a.astype(np.int64), minlength=n_lists), out=list_off[1:])
    return perm, list_off


def _ivf_layout_device(assign, n_lists):
    """ivf_layout of an int64 device tensor of list ids, in torch -> (perm, list_off) on its device: a stable sort of the
    list ids, bincount and cumsum (a batch that is being added; a whole matrix goes through Pq.lists_layout_device)"""
    import torch
    list_off = torch.zeros(n_lists + 1, dtype=torch.int64, device=assign.device)
    list_off[1:] = torch.cumsum(torch.bincount(assign, minlength=n_lists), 0)
    return torch.sort(assign, stable=True).indices, list_off


class _ListLayout:
    """What every partitioned class shares, over codes or over the vectors themselves: the list layout, the coarse
    quantizer, the probe selection and the assignment of new rows.  `codes` is what the class stores per row, in list
    order (it lends its device and its length)."""

    def _init_lists(self, centroids, assign, n_rows, dev, ctx, want_lists=False):
        """The layout of the lists from `assign`: a numpy array of list ids (ivf_layout on the host) or an int64 CUDA
        tensor (Pq.lists_layout_device: nothing of length N touches the host) -> with want_lists the list of every
        position (device int64 [N]; device route only), else None."""
        import torch
        self.centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        self.n_lists = self.centroids.shape[0]
        on_device = hasattr(assign, "is_cuda")
        if on_device:
            if not assign.is_cuda or assign.dtype != torch.int64 or assign.device != torch.device(dev):
                raise PanicError("a device assignment must be an int64 CUDA tensor on the device of the codes")
            if tuple(assign.shape) != (n_rows,):
                raise PanicError("one list id per row expected")
        else:
            perm, list_off = ivf_layout(assign, self.n_lists)
            if perm.size != n_rows:
                raise PanicError("one list id per row expected")
        # the coarse quantizer as a codebook of one subquantizer: its distance tables order the lists
        self.coarse = Pq(None, self.centroids[None], ctx=ctx)
        self._list_ids = torch.arange(self.n_lists, dtype=torch.int32, device=dev)[:, None].contiguous()
        if on_device:
            laid = self.coarse.lists_layout_device(assign.contiguous(), self.n_lists, want_lists=want_lists, check=True)
            self.ids, self.list_off, self.positions = laid[:3]
            return laid[3] if want_lists else None
        self.ids, self.list_off = torch.from_numpy(perm).to(dev), torch.from_numpy(list_off).to(dev)
        self.positions = _positions(self.ids)

    def __len__(self):
        return self.codes.shape[0]

    def _probes_and_dists(self, queries, nprobe):
        """(list ids, their coarse distances) as probes() defines them; on the all-lists route beyond 1,024 probes the
        distances are the coarse table rows themselves"""
        import torch
        nprobe = min(int(nprobe), self.n_lists)
        if nprobe < 1:
            raise PanicError("nprobe must be at least 1")
        single = queries.dim() == 1
        tables = self.coarse.adc_tables_device(queries)
        if nprobe > 1024:
            if nprobe < self.n_lists:
                raise PanicError("more than 1024 probes are served only as all %d lists" % self.n_lists)
            nq = 1 if single else queries.shape[0]
            pr = torch.arange(self.n_lists, dtype=torch.int64, device=self.codes.device)
            if single:
                return pr, tables[0]
            return pr[None].expand(nq, -1).contiguous(), tables[:, 0, :].contiguous()
        d, pr = self.coarse.adc_search_device(self._list_ids, tables, nprobe)
        return pr, d

    def probes(self, queries, nprobe):
        """list ids [nq, nprobe] int64 ([nprobe] for one query): the nprobe first lists in the order (key(dist), list
        id), dist the squared distance of the query to the coarse centroids as adc_tables_device of the one-subquantizer
        codebook defines it, key the first-minimum order (NaN last).  nprobe is cut to n_lists; beyond 1,024 only
        nprobe >= n_lists is served, by all list ids in ascending order (every list is read, no selection needed)."""
        return self._probes_and_dists(queries, nprobe)[0]

    def _original_rows(self, pos):
        import torch
        return torch.where(pos < 0, pos, self.ids[pos.clamp(min=0)])

    def _among_ids(self, rows):
        """original row numbers -> positions, without an index out of bounds on the device: the gather is clamped, -1
        stays -1 and any other number outside [0, N) becomes N, which the kernel skips and flags"""
        import torch
        n = len(self)
        inside = (rows >= 0) & (rows < n)
        pos = self.positions[rows.clamp(0, n - 1)] if n else torch.zeros_like(rows)
        return torch.where(inside, pos, torch.where(rows == -1, rows, torch.full_like(rows, n))).contiguous()

    def assign(self, vectors):
        """the list of each vector ([B, d] float32, numpy or CUDA) -> int64 [B] on the device: the nearest centroid, as
        cluster_assignments(self.centroids, vectors) gives it row for row (the encode kernels of the one-subquantizer
        coarse codebook with a 4-byte index, entirely on the device)"""
        x = _device_rows(vectors, self.centroids.shape[1], self.codes.device)
        return _assign_device(self.coarse, x.shape[0], lambda r0, r1: x[r0:r1], x.device)

    def _kept_flags(self, allow, words):
        """what compact() keeps, as uint8 flags [N] in ORIGINAL row order: from the flags themselves, or from a
        RowFilter's words (bit p = position p is kept) through ids"""
        import torch
        N, dev = len(self), self.codes.device
        if isinstance(allow, RowFilter):             # the filter keeps the words only: bit p = position p is kept
            shifts = torch.arange(32, dtype=torch.int32, device=dev)
            kept_pos = ((words[:, None] >> shifts) & 1).reshape(-1)[:N].to(torch.uint8)
            flags = torch.empty(N, dtype=torch.uint8, device=dev)
            flags[self.ids] = kept_pos
            return flags
        return _on_device(allow, dev).view(torch.uint8)      # the flags themselves (row_filter has checked them)


class _Lists(_ListLayout, _Refine, _Filter, _Packed4, _Search, _Among, _Compact):
    """What both partitioned forms over codes share beside the layout: growth and compaction of the stored arrays."""

    device_terms = False        # ResidualPartitionedMatrix: the row terms come from Pq.residual_terms_device

    # ---- growth: every method returns a NEW matrix and leaves self (and the row filters built for it) untouched ----
    _ROW_ARRAYS = ("codes", "norms")          # what a matrix stores per row, in list order, beside ids

    def _shell(self):
        """a matrix of this class that shares what growth does not change: quantizers, centroids, probe selection"""
        return _clone(self, ("pq", "centroids", "n_lists", "coarse", "_list_ids", "_centroids_dev", "packed4", "device_terms"))

    def _piece(self, assign, vectors, **row_arrays):
        """A batch laid out as a matrix of this class over the same lists: `assign` int64 [B] on the device, row_arrays
        the per-row arrays in batch order (None where the matrix has none).  B-sized torch operations only."""
        p = self._shell()
        p.ids, p.list_off = _ivf_layout_device(assign, self.n_lists)
        p.positions = _positions(p.ids)
        for name, t in row_arrays.items():
            setattr(p, name, None if t is None else t[p.ids].contiguous())
        p.vectors = vectors
        return p

    def extend(self, other):
        """The matrix that holds the rows of self followed by the rows of `other`, a matrix of the same class over the
        same lists (equal pq, equal centroids, norms in both or in neither; PanicError otherwise) -> a NEW matrix; the
        rows of other are renumbered from len(self).  List l of the result is list l of self followed by list l of
        other, which is what the constructor builds from the concatenated rows and assignments: every stored array is
        merged on the device (Pq.merge_lists_device), positions are rebuilt by a scatter, and nothing of length N
        goes to the host or through a sort.  Attached vectors are concatenated, in the dtype of self, if both
        matrices have them, and dropped otherwise.  Row filters are not carried over.  Both matrices hold 4-bit packed
        codes or neither does (PanicError otherwise: pack4() or unpack4() one of them); the merge moves the packed rows."""
        import torch
        if type(other) is not type(self):
            raise PanicError("only a matrix of the same class can be merged")
        if other.packed4 != self.packed4:
            raise PanicError("a packed and an unpacked matrix cannot be merged: call pack4() or unpack4() on one of them")
        if other.device_terms != self.device_terms:
            raise PanicError("the row terms of the two matrices come from different routes (device_terms differs)")
        if not (other.pq == self.pq) or not np.array_equal(other.centroids, self.centroids):
            raise PanicError("the matrices must share the quantizer and the centroids of the lists")
        if (other.norms is None) != (self.norms is None):
            raise PanicError("either both matrices have norms or neither")
        if other.codes.device != self.codes.device or other.codes.dtype != self.codes.dtype:
            raise PanicError("the matrices must live on one device and hold codes of one width")
        new = self._shell()
        merge = self.pq.merge_lists_device
        new.ids, new.list_off = merge(self.list_off, self.ids, other.list_off, other.ids + len(self))
        for name in self._ROW_ARRAYS:
            mine = getattr(self, name)
            setattr(new, name, None if mine is None else merge(self.list_off, mine, other.list_off, getattr(other, name))[0])
        new.positions = _positions(new.ids)
        if self.vectors is not None and other.vectors is not None:
            new.vectors = torch.cat([self.vectors, other.vectors.to(self.vectors.device, self.vectors.dtype)])
        return new

    def compact(self, allow):
        """The matrix of the rows that `allow` keeps (a RowFilter of this matrix, or a bool array [N] in ORIGINAL row
        order) -> (new_matrix, kept): a NEW matrix of this class over the same lists, and kept, int64 [N'] on the
        device, the old row number of new row i, ascending; the kept rows are renumbered 0 .. N' - 1 in that order.
        Compaction is stable in position order, so list l of the result is the kept rows of list l, in order -- what
        the constructor builds from the kept rows and their assignments: every stored array is compacted under the
        position-order mask (Pq.compact_rows_device, which also gives list_off), ids[p'] = rank[ids[p]] with rank the
        running count of the original-order flags, positions are rebuilt by a scatter.  Attached vectors are compacted
        under the original-order mask.  Centroids, coarse codebook, packed4 and device_terms are shared or carried."""
        import torch
        words = self._keep_words(allow)
        N = len(self)
        flags = self._kept_flags(allow, words)
        rank = torch.cumsum(flags, 0, dtype=torch.int64) - 1
        names = ("ids",) + self._ROW_ARRAYS
        outs, list_off, _ = _compact_arrays(self.pq, words, N, [getattr(self, name) for name in names], list_off=self.list_off)
        new = self._shell()
        for name, t in zip(names, outs):
            setattr(new, name, t)
        new.ids = rank[new.ids]
        new.list_off = list_off
        new.positions = _positions(new.ids)
        words_orig = self.pq.pack_row_mask_device(flags)
        kept = self.pq.compact_rows_device(words_orig, None, want_src_rows=True, n=N)[2]
        if self.vectors is not None:
            new.vectors = self._compact_vectors(words_orig, kept)
        return new, kept

    def _add_encoded(self, x, norms, assign, **row_arrays):
        """add() of both classes: extend() applied to the batch laid out as a piece"""
        nb = _batch_norms(norms, self.norms is not None, x.shape[0], x.device)
        return self.extend(self._piece(assign, x if self.vectors is not None else None, norms=nb, **row_arrays))


class PartitionedMatrix(_Lists):
    """A QuantizedMatrix whose rows are grouped by a coarse quantizer: list l holds the rows nearest to centroid l,
    stored contiguously, and a search reads only the `nprobe` lists nearest to the query.  The codes are those of the
    vectors themselves, so a search is the exhaustive search restricted to the rows of the probed lists, bit for bit;
    with nprobe = n_lists it is the exhaustive search.  Row numbers given and returned are those of the matrix it was
    built from.

    centroids [n_lists, d] float32 (host); list_off [n_lists + 1] and ids [N] int64 on the device (ids[p] = original row
    of position p); codes / norms in list order."""

    def __init__(self, qm, centroids, assign):
        self.pq = qm.pq
        self._init_lists(centroids, assign, len(qm), qm.codes.device, self.pq._ctx)
        self.codes = qm.codes[self.ids].contiguous()
        self.norms = None if qm.norms is None else qm.norms[self.ids].contiguous()

    def _search_terms(self, ip, ranged, queries, nprobe):
        pq = self.pq
        if ip:
            fn = pq.adc_ip_range_lists_device if ranged else pq.adc_ip_search_lists_device
        else:
            fn = pq.adc_range_lists_device if ranged else pq.adc_search_lists_device
        return fn, self._tables(ip, queries), (self.list_off, self.probes(queries, nprobe))

    def nearest(self, queries, k, nprobe, refine=None, allow=None):
        """the k rows of smallest asymmetric squared distance among the rows of the nprobe nearest lists, ties to the
        smaller position in list order -> (dist, idx) [k] or [nq, k]; idx are original row numbers, -1 past the last
        probed row (distance +Inf).  refine=R (k <= R <= 1024, vectors attached): the R first rows of that search are
        re-ranked by their exact squared distance to the attached vectors (Pq.rerank_device), ties to the smaller
        original row number; dist are then the exact distances.  allow: None, a RowFilter of this matrix or a bool array
        [N] in ORIGINAL row order -- only allowed rows of the probed lists are ranked, as if the others were not stored."""
        return self._topk(False, queries, k, nprobe, True, refine, allow)

    def most_similar(self, queries, k, nprobe, use_norms=True, refine=None, allow=None):
        """QuantizedMatrix.most_similar among the rows of the nprobe nearest lists -> (score, idx), idx original row
        numbers, -1 past the last probed row (score -Inf).  refine=R: the R first rows are re-ranked by their exact
        inner product with the attached vectors as they are; use_norms then only affects the candidate stage.
        allow: as for nearest()."""
        return self._topk(True, queries, k, nprobe, use_norms, refine, allow)

    def within(self, queries, radius, nprobe, allow=None, sort=False):
        """QuantizedMatrix.within among the rows of the nprobe nearest lists -> (lims, dist, idx), idx original row
        numbers; the rows of a query come list by list in probe order, inside a list in ascending original row number
        (Pq.adc_range_lists_device).  sort=True: ascending in distance, ties in that order.  No refine=: re-ranking is
        defined for at most 1,024 candidates per query.  Not served on a packed matrix: unpack4() first."""
        return self._range(False, queries, radius, nprobe, True, allow, sort)

    def similar_above(self, queries, threshold, nprobe, use_norms=True, allow=None, sort=False):
        """QuantizedMatrix.similar_above among the rows of the nprobe nearest lists -> (lims, score, idx), idx original
        row numbers, order as for within() (Pq.adc_ip_range_lists_device).  sort=True: descending in score.  Not served
        on a packed matrix: unpack4() first."""
        return self._range(True, queries, threshold, nprobe, use_norms, allow, sort)

    def add(self, vectors, norms=None):
        """The matrix with `vectors` ([B, d] float32, numpy or CUDA) added as rows len(self) .. len(self) + B - 1 -> a NEW
        PartitionedMatrix: each vector goes to the end of the list assign() names, stored as quantize_batch_device
        encodes it.  The result is, tensor for tensor, the matrix the constructor builds from all rows in row order.
        norms [B] is required iff the matrix has norms.  Attached vectors are extended in the attached dtype."""
        x = _device_rows(vectors, self.pq.reconstructed_len(), self.codes.device)
        codes = self._stored_codes(self.pq.quantize_batch_device(x)) if x.shape[0] else self.codes[:0]
        return self._add_encoded(x, norms, self.assign(x), codes=codes)

    def embeddings(self, rows, out=None):
        """QuantizedMatrix.embeddings of the original row numbers `rows`."""
        import torch
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.codes.device)
        return self._reconstruct_rows(self.positions[rows], scales=self.norms, out=out)


class ResidualPartitionedMatrix(_Lists):
    """A partitioned matrix whose codes encode the residual of each row against its list's centroid (IVFADC with
    residual encoding, built by QuantizedMatrix.partition_residual): row i of list l stands for c_l + r^_i, r^_i the
    reconstruction of its code by `pq`, the quantizer of the residuals.  A search keeps one table per query -- the
    inner-product table of the residual quantizer -- plus one bias per probed list and, for distances, the stored
    query-free term of each row (include/pqhip.h: pqhip_adc_search_lists_residual_f32_dev):
        |q - c_l - r^_i|^2 = |q - c_l|^2 + row_terms[i] - 2 <q, r^_i>          <q, c_l + r^_i> = <q, c_l> + <q, r^_i>
    Row numbers given and returned are those of the matrix it was built from.

    pq: the residual quantizer; coarse: the one-subquantizer codebook of the centroids [n_lists, d] (host float32);
    list_off [n_lists + 1], ids [N], positions [N] and lists [N] (the list of each position) int64 on the device; codes
    [N, M] u8, norms [N] f32 or None and row_terms [N] f32 in list order.
    Reading or writing such a matrix as a storage chunk is not provided: finalfusion has no chunk for residual codes."""

    def __init__(self, pq, codes, norms, row_terms, centroids, assign):
        """codes / norms / row_terms in original row order (device tensors); assign [N] the list of each row: a numpy
        array, or an int64 CUDA tensor, which is laid out on the device (`lists` is then the kernel's fourth output)."""
        import torch
        dev = codes.device
        self.pq = pq
        lists = self._init_lists(centroids, assign, codes.shape[0], dev, pq._ctx, want_lists=True)
        self.codes = codes[self.ids].contiguous()
        self.norms = None if norms is None else norms[self.ids].contiguous()
        self.row_terms = row_terms[self.ids].contiguous()
        if lists is None:
            lists = torch.from_numpy(np.asarray(assign, dtype=np.int64)).to(dev)[self.ids].contiguous()
        self.lists = lists
        self._centroids_dev = torch.from_numpy(self.centroids).to(dev)

    def _search_terms(self, ip, ranged, queries, nprobe):
        """the probes with the bias of each -- |q - c_l|^2 for distances, <q, c_l> for inner products -- then the one
        table per query, which is the inner-product table for both"""
        pq = self.pq
        pr, bias = self._probes_and_ips(queries, nprobe) if ip else self._probes_and_dists(queries, nprobe)
        if ip:
            fn = pq.adc_ip_range_lists_residual_device if ranged else pq.adc_ip_search_lists_residual_device
        else:
            fn = pq.adc_range_lists_residual_device if ranged else pq.adc_search_lists_residual_device
        return fn, pq.adc_ip_tables_device(queries), (self.list_off, pr, bias) + (() if ip else (self.row_terms,))

    def nearest(self, queries, k, nprobe, refine=None, allow=None):
        """the k rows of smallest dist = fl(fl(bias + row_term) - fl(s + s)) among the rows of the nprobe nearest lists:
        s the row sum over the query's inner-product table, bias the coarse distance of the row's list as
        coarse.adc_search_device returns it beside the probed ids (the coarse table row when more than 1,024 lists are
        all probed) -> (dist, idx) [k] or [nq, k]; idx are original row numbers, -1 past the last probed row (+Inf).
        refine=R (k <= R <= 1024, vectors attached): the R first rows of that search are re-ranked by their exact
        squared distance to the attached vectors (Pq.rerank_device); dist are then the exact distances.  allow: as for
        PartitionedMatrix.nearest."""
        return self._topk(False, queries, k, nprobe, True, refine, allow)

    def _probes_and_ips(self, queries, nprobe):
        """(list ids as probes() defines them, <q, c_l> of each: the entry of the coarse inner-product table at the list;
        at a padded id the entry of list 0, which no result reads)"""
        import torch
        pr = self.probes(queries, nprobe)
        ipt = self.coarse.adc_ip_tables_device(queries)
        ipt = ipt[0] if queries.dim() == 1 else ipt[:, 0, :]
        return pr, torch.gather(ipt, -1, pr.clamp(min=0)).contiguous()

    def most_similar(self, queries, k, nprobe, use_norms=True, refine=None, allow=None):
        """the k rows of largest score = fl(fl(bias + s) * norm) (fl(bias + s) with use_norms=False or without norms)
        among the rows of the nprobe nearest lists, bias the entry of coarse.adc_ip_tables_device(queries)[:, 0, :] at
        the row's list, i.e. <q, c_l> -> (score, idx), idx original row numbers, -1 past the last probed row (-Inf).
        refine=R: the R first rows are re-ranked by their exact inner product with the attached vectors as they are;
        use_norms then only affects the candidate stage.  allow: as for PartitionedMatrix.nearest."""
        return self._topk(True, queries, k, nprobe, use_norms, refine, allow)

    def within(self, queries, radius, nprobe, allow=None, sort=False):
        """every row of the nprobe nearest lists with dist = fl(fl(bias + row_term) - fl(s + s)) <= radius, bias obtained
        exactly as nearest() obtains it -> (lims, dist, idx), idx original row numbers, rows list by list in probe order
        (Pq.adc_range_lists_residual_device).  sort=True: ascending in distance.  No refine=: re-ranking is defined for
        at most 1,024 candidates per query.  Not served on a packed matrix: unpack4() first."""
        return self._range(False, queries, radius, nprobe, True, allow, sort)

    def similar_above(self, queries, threshold, nprobe, use_norms=True, allow=None, sort=False):
        """every row of the nprobe nearest lists with score = fl(fl(bias + s) * norm) >= threshold (fl(bias + s) with
        use_norms=False or without norms), bias obtained exactly as most_similar() obtains it -> (lims, score, idx)
        (Pq.adc_ip_range_lists_residual_device).  sort=True: descending in score.  Not served on a packed matrix:
        unpack4() first."""
        return self._range(True, queries, threshold, nprobe, use_norms, allow, sort)

    _ROW_ARRAYS = ("codes", "norms", "row_terms", "lists")

    def _among_terms(self, ip, queries):
        """the residual forms: the list of every position, the row terms and, as the bias of every list, the full row
        of the coarse table -- |q - c_l|^2 resp. <q, c_l> -- so a candidate need not lie in a probed list"""
        ct = self.coarse.adc_ip_tables_device(queries) if ip else self.coarse.adc_tables_device(queries)
        kw = {"row_list": self.lists, "list_bias": ct[0] if queries.dim() == 1 else ct[:, 0, :]}
        if not ip:
            kw["row_terms"] = self.row_terms
        return self.pq.adc_ip_tables_device(queries), kw

    def encode(self, vectors):
        """What the matrix would store for `vectors` ([B, d] float32, numpy or CUDA) -> (lists int64 [B], codes u8 [B, M],
        row_terms f32 [B]) on the device: the list assign() names, the code of the f32 residual against that list's
        centroid, and the row's query-free term -- the loop body of partition_residual, on the route the matrix was
        built by (device_terms: Pq.residuals_device and Pq.residual_terms_device), so add() stays the constructor
        applied to the concatenation."""
        x = _device_rows(vectors, self.pq.reconstructed_len(), self.codes.device)
        lists = self.assign(x)
        codes, terms = _encode_residuals(self.pq, x.shape[0], lambda r0, r1: x[r0:r1], lists, self._centroids_dev,
                                         self.device_terms)
        return lists, codes, terms

    def add(self, vectors, norms=None):
        """The matrix with `vectors` ([B, d] float32, numpy or CUDA) added as rows len(self) .. len(self) + B - 1 -> a NEW
        ResidualPartitionedMatrix: each vector goes to the end of its list, stored as encode() gives it.  The result
        is, tensor for tensor, the matrix the constructor builds from all rows in row order.  norms [B] is required
        iff the matrix has norms.  Attached vectors are extended in the attached dtype.  Neither quantizer is
        re-trained."""
        x = _device_rows(vectors, self.pq.reconstructed_len(), self.codes.device)
        lists, codes, terms = self.encode(x)
        return self._add_encoded(x, norms, lists, codes=self._stored_codes(codes), row_terms=terms, lists=lists)

    def embeddings(self, rows):
        """fl(fl(r^ + c_l) * norm) of the original row numbers `rows` (fl(r^ + c_l) without norms) -> [len(rows), d]."""
        import torch
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.codes.device)
        pos = self.positions[rows]
        e = self._reconstruct_rows(pos) + self._centroids_dev[self.lists[pos]]
        return e if self.norms is None else e * self.norms[pos][:, None]


class FlatMatrix(_Refine, _Filter, _Compact):
    """Rows kept as they are, f32 or f16, and searched exactly: no quantizer, no codes.  Every search is the exhaustive
    top-k by the true squared distance or inner product (Pq.flat_search_device), so rows are searchable the moment
    they are added -- the delta of a MatrixGroup before it is encoded -- and a small collection needs no training.  Its
    values are those `refine=` returns on the other classes.  within() / similar_above() return every row inside a
    radius by the same values (Pq.flat_range_device).  `vectors` is the [N, d] device tensor; `pq` is a
    one-centroid placeholder of width d that only lends its device slot and scratch to the calls."""

    def __init__(self, vectors, device="cuda:0", dtype=None, ctx=None):
        import torch
        if len(vectors.shape) != 2 or vectors.shape[1] < 1:
            raise PanicError("vectors must be [N, d]")
        if dtype is None:
            dtype = torch.float16 if str(vectors.dtype) in ("float16", "torch.float16") else torch.float32
        if dtype not in (torch.float32, torch.float16):
            raise PanicError("vectors are kept as float32 or float16")
        self.vectors = _on_device(vectors, device, dtype)
        self.pq = Pq(None, np.zeros((1, 1, vectors.shape[1]), np.float32), ctx=ctx)

    @property
    def codes(self):
        """what the shared row-filter and compaction code asks for its device: the stored rows take the codes' place"""
        return self.vectors

    def __len__(self):
        return self.vectors.shape[0]

    def attach_vectors(self, vectors, dtype=None):
        raise PanicError("a FlatMatrix holds its vectors already")

    def _topk(self, ip, queries, k, refine, allow, screen=False):
        import torch
        if refine is not None:
            self._check_refine(k, refine)       # the estimate is exact already: refine changes nothing
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        return self._flat_topk(q, k, ip, self._allow_words(allow), screen)

    def nearest(self, queries, k, refine=None, allow=None, screen=False):
        """the k rows of smallest exact squared distance, ties to the smaller row -> (dist, idx) [k] or [nq, k]; index -1
        and +Inf past the last (allowed) row.  refine is accepted and changes nothing; allow: None, a RowFilter of this
        matrix or a bool array [N].  screen=True: the route for query batches (Pq.flat_search_batch_device: matrix-core
        screen, exact resolve), the same result bit for bit; vectors wider than 2,048 elements keep the plain call."""
        return self._topk(False, queries, k, refine, allow, screen)

    def most_similar(self, queries, k, use_norms=True, refine=None, allow=None, screen=False):
        """the k rows of largest exact inner product, largest first -> (score, idx); use_norms is accepted and ignored
        (the rows are stored unscaled), refine and allow as for nearest()."""
        return self._topk(True, queries, k, refine, allow, screen)

    def _range(self, ip, queries, threshold, allow, sort, screen=False):
        import torch
        q = _on_device(queries, self.vectors.device, torch.float32, np.float32)
        lims, val, rows = self._flat_range(q, threshold, ip, self._allow_words(allow), screen)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows

    def within(self, queries, radius, allow=None, sort=False, screen=False):
        """EVERY row whose exact squared distance to the query is <= radius (a scalar or one value per query) -> (lims,
        dist, idx): CSR over the queries, lims int64 [nq + 1] ([2] for one query), the rows of query q at
        lims[q]:lims[q + 1] in ascending row number, dist the value nearest() returns for the row (Pq.flat_range_device;
        the result is allocated to its size, after one read of the count).  sort=True: each query's rows ascending in
        distance instead, ties in row order (sort_ranges).  allow: as for nearest().  screen=True: the route for query
        batches (Pq.flat_range_batch_device), the same result bit for bit."""
        return self._range(False, queries, radius, allow, sort, screen)

    def similar_above(self, queries, threshold, use_norms=True, allow=None, sort=False, screen=False):
        """Every row whose exact inner product with the query is >= threshold (a scalar or one value per query) ->
        (lims, score, idx), CSR as for within(); sort=True: each query's rows descending in score, ties in row order.
        use_norms is accepted and ignored, as in most_similar(); screen as for within()."""
        return self._range(True, queries, threshold, allow, sort, screen)

    def nearest_among(self, queries, rows, k):
        """nearest() among the rows that `rows` names and no others: a vector of row numbers shared by all queries, or the
        pair (lims, rows) -- the rows of query q are rows[lims[q]:lims[q + 1]], what within() returns -> (dist, idx) [k]
        or [nq, k], ties to the smaller row, index -1 and +Inf past the last (Pq.flat_among_device).  -1 is padding, any
        other number outside [0, N) is skipped; a row named twice may come back twice.  For distinct rows the result is
        nearest(queries, k, allow=<flags of the rows>) at the cost of the named rows alone."""
        return self._exact_among(False, queries, rows, k)

    def most_similar_among(self, queries, rows, k):
        """most_similar() among the rows that `rows` names (as for nearest_among) -> (score, idx), largest first."""
        return self._exact_among(True, queries, rows, k)

    def within_among(self, queries, rows, radius, sort=False):
        """within() among the rows that `rows` names (as for nearest_among) -> (lims, dist, idx): of every query's rows
        those whose exact squared distance is <= radius, in the order in which they were named
        (Pq.flat_range_among_device); sort=True: ascending in distance.  A row named twice is returned twice."""
        return self._exact_range_among(False, queries, rows, radius, sort)

    def similar_above_among(self, queries, rows, threshold, sort=False):
        """similar_above() among the rows that `rows` names -> (lims, score, idx), as within_among(); sort=True:
        descending in score."""
        return self._exact_range_among(True, queries, rows, threshold, sort)

    def embeddings(self, rows):
        """the stored rows `rows` as float32 [len(rows), d]"""
        import torch
        rows = _on_device(rows, self.vectors.device, torch.int64, np.int64).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= len(self)):
            raise PanicError("row numbers must lie in [0, %d)" % len(self))
        return self.vectors[rows].to(torch.float32)

    def add(self, vectors):
        """The matrix with the rows of `vectors` ([B, d]) appended, rounded to the stored dtype -> a NEW FlatMatrix; self
        and its row filters stay as they are."""
        import torch
        x = _device_rows(vectors, self.vectors.shape[1], self.vectors.device)
        new = _clone(self, ("pq",))
        new.vectors = torch.cat([self.vectors, x.to(self.vectors.dtype)])
        return new

    def compact(self, allow):
        """The matrix of the rows that `allow` keeps (a RowFilter of this matrix, or a bool array [N]) -> (new_matrix,
        kept), kept the old row number of new row i, ascending (Pq.compact_rows_device)."""
        words = self._keep_words(allow)
        _, _, kept = _compact_arrays(self.pq, words, len(self), (), want_src_rows=True)
        new = _clone(self, ("pq",))
        new.vectors = self._compact_vectors(words, kept)
        return new, kept

    # the coarse training and assignment of QuantizedMatrix.partition: it asks self for pq (width, context), codes
    # (device) and len alone, which this class has, and reads the rows from the `vectors` it is given
    _coarse_partition = QuantizedMatrix._coarse_partition

    def partition(self, n_lists, n_iterations=10, train_rows=None, rng=None):
        """Partition the rows with a coarse k-means quantizer of n_lists centroids -> PartitionedFlatMatrix (IVF-Flat:
        the rows stay the vectors themselves, a search reads the probed lists only).  The quantizer is trained on the
        stored rows (f16 rows converted to f32), on train_rows distinct rows drawn with `rng` if given, from n_lists
        distinct training rows as initial centroids: the training and the draws from `rng` of QuantizedMatrix.partition
        with these rows as `vectors`.  Every row is assigned by the coarse codebook's quantize_batch_device and laid out
        by Pq.lists_layout_device: nothing of length N goes to the host.  Row filters are not carried over."""
        rng = rng or np.random.default_rng(0)
        centroids, assign, _, _ = self._coarse_partition(n_lists, n_iterations, self.vectors, train_rows, rng, on_device=True)
        return PartitionedFlatMatrix(self.vectors, centroids, assign, device=self.vectors.device, dtype=self.vectors.dtype,
                                     ctx=self.pq._ctx)


class PartitionedFlatMatrix(_ListLayout, _Filter, _Compact):
    """A FlatMatrix whose rows are grouped by a coarse quantizer (IVF-Flat): list l holds the rows nearest to centroid l,
    stored contiguously, and a search reads only the `nprobe` lists nearest to the query -- by the exact value of
    FlatMatrix, so a search is FlatMatrix's restricted to the rows of the probed lists, bit for bit; with nprobe = n_lists
    it returns FlatMatrix's values.  Ties go to the smaller position in list order.  Row numbers given and returned are
    those of `vectors` as it was given.

    rows [N, d] f32 or f16 in list order; ids [N] (ids[p] = original row of position p), positions [N] and list_off
    [n_lists + 1] int64 on the device; centroids [n_lists, d] float32 (host); coarse (also `pq`): the one-subquantizer
    codebook of the centroids, which orders the lists, assigns new rows and lends its device slot and scratch."""

    vectors = None              # nothing is attached: the rows are the vectors

    def __init__(self, vectors, centroids, assign, device="cuda:0", dtype=None, ctx=None):
        """vectors [N, d] (numpy or torch), centroids [n_lists, d], assign [N] the list of every row: a numpy array of
        list ids or an int64 CUDA tensor on `device` (then nothing of length N touches the host)."""
        import torch
        if len(vectors.shape) != 2 or vectors.shape[1] < 1:
            raise PanicError("vectors must be [N, d]")
        if dtype is None:
            dtype = torch.float16 if str(vectors.dtype) in ("float16", "torch.float16") else torch.float32
        if dtype not in (torch.float32, torch.float16):
            raise PanicError("vectors are kept as float32 or float16")
        if len(np.shape(centroids)) != 2 or np.shape(centroids)[1] != vectors.shape[1]:
            raise PanicError("centroids must be [n_lists, %d]" % vectors.shape[1])
        v = _on_device(vectors, device, dtype)
        self._init_lists(centroids, assign, v.shape[0], v.device, ctx)
        self.pq = self.coarse
        self.rows = v[self.ids].contiguous()

    @property
    def codes(self):
        """what the shared layout, row-filter and compaction code asks for its device: the stored rows take the codes' place"""
        return self.rows

    def _shell(self):
        """a matrix of this class that shares what growth and compaction do not change"""
        return _clone(self, ("pq", "centroids", "n_lists", "coarse", "_list_ids"))

    def _wide(self):
        """rows beyond the 4,096 bytes that the device mover and the device compaction take: they go through torch"""
        return self.rows.shape[1] * self.rows.element_size() > 4096

    # ---- searches -------------------------------------------------------------------------------------------------------
    def _check_refine(self, k, refine):
        if not k <= int(refine) <= 1024:
            raise PanicError("refine must lie between k and 1024, was %d (k = %d)" % (refine, k))
        return int(refine)

    def _refined(self, queries, rows, k, ip):
        """the re-ranking a MatrixGroup asks of a part: the candidates' exact values against the stored rows, which are
        the values the search itself returns; ties to the smaller position"""
        val, pos = self.pq.rerank_device(queries, self.rows, self._among_ids(rows), k, ip=ip)
        return val, self._original_rows(pos)

    def _topk(self, ip, queries, k, nprobe, refine, allow):
        import torch
        if refine is not None:
            self._check_refine(k, refine)       # the values are exact already: refine changes nothing
        q = _on_device(queries, self.rows.device, torch.float32, np.float32)
        val, pos = self.pq.flat_search_lists_device(q, self.rows, self.list_off, self.probes(q, nprobe), k, ip=ip,
                                                    allow=self._allow_words(allow))
        return val, self._original_rows(pos)

    def nearest(self, queries, k, nprobe, refine=None, allow=None):
        """the k rows of smallest exact squared distance among the rows of the nprobe nearest lists, ties to the smaller
        position in list order -> (dist, idx) [k] or [nq, k]; idx are original row numbers, -1 past the last probed
        (allowed) row (distance +Inf).  refine is accepted and changes nothing; allow: None, a RowFilter of this matrix
        or a bool array [N] in ORIGINAL row order (Pq.flat_search_lists_device)."""
        return self._topk(False, queries, k, nprobe, refine, allow)

    def most_similar(self, queries, k, nprobe, use_norms=True, refine=None, allow=None):
        """the k rows of largest exact inner product among the rows of the nprobe nearest lists, largest first ->
        (score, idx), -1 and -Inf past the last probed row; use_norms is accepted and ignored (the rows are stored
        unscaled), the rest as for nearest().  The lists are chosen by distance to the centroids, as for nearest()."""
        return self._topk(True, queries, k, nprobe, refine, allow)

    def _range(self, ip, queries, threshold, nprobe, allow, sort):
        import torch
        q = _on_device(queries, self.rows.device, torch.float32, np.float32)
        lims, val, pos = self.pq.flat_range_lists_device(q, self.rows, self.list_off, self.probes(q, nprobe), threshold, ip=ip,
                                                         allow=self._allow_words(allow))
        rows = self._original_rows(pos)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows

    def within(self, queries, radius, nprobe, allow=None, sort=False):
        """EVERY row of the nprobe nearest lists whose exact squared distance to the query is <= radius (a scalar or one
        value per query) -> (lims, dist, idx), CSR over the queries; idx are original row numbers and the rows of a query
        come list by list in probe order, inside a list in its stored order (Pq.flat_range_lists_device).  The values
        are FlatMatrix.within()'s: with nprobe = n_lists the result is the same set.  sort=True: ascending in distance,
        ties in that order.  allow: as for nearest()."""
        return self._range(False, queries, radius, nprobe, allow, sort)

    def similar_above(self, queries, threshold, nprobe, use_norms=True, allow=None, sort=False):
        """Every row of the nprobe nearest lists whose exact inner product with the query is >= threshold -> (lims,
        score, idx), as within(); sort=True: descending in score.  use_norms is accepted and ignored, as in
        most_similar()."""
        return self._range(True, queries, threshold, nprobe, allow, sort)

    def _among(self, ip, queries, rows, k):
        import torch
        lims, rows = _Among._among_rows(self, rows)
        q = _on_device(queries, self.rows.device, torch.float32, np.float32)
        val, pos = self.pq.flat_among_device(q, self.rows, self._among_ids(rows), k, lims=lims, ip=ip)
        return val, self._original_rows(pos)

    def nearest_among(self, queries, rows, k):
        """nearest() among the rows that `rows` names and no others, whatever their lists: a vector of ORIGINAL row
        numbers shared by all queries, or the pair (lims, rows) that within() returns -> (dist, idx) [k] or [nq, k] in
        original row numbers, index -1 and +Inf past the last (Pq.flat_among_device).  The rows are mapped to positions
        and back; like the quantized partitioned classes this one breaks ties by POSITION in list order, not by row
        number.  -1 is padding, any other number outside [0, N) is skipped; a row named twice may come back twice.
        For distinct rows the result is nearest(queries, k, n_lists, allow=<flags of the rows>) at the cost of the named
        rows alone."""
        return self._among(False, queries, rows, k)

    def most_similar_among(self, queries, rows, k):
        """most_similar() among the rows that `rows` names (as for nearest_among, ties by position) -> (score, idx),
        largest first."""
        return self._among(True, queries, rows, k)

    def _range_among(self, ip, queries, rows, threshold, sort):
        import torch
        lims, rows = _Among._among_rows(self, rows)
        q = _on_device(queries, self.rows.device, torch.float32, np.float32)
        lims, val, pos = self.pq.flat_range_among_device(q, self.rows, self._among_ids(rows), threshold, lims=lims, ip=ip)
        rows = self._original_rows(pos)
        if sort:
            val, rows = sort_ranges(lims, val, rows, ip)
        return lims, val, rows

    def within_among(self, queries, rows, radius, sort=False):
        """within() among the rows that `rows` names (as for nearest_among), whatever their lists -> (lims, dist, idx): of
        every query's rows those whose exact squared distance is <= radius, in the order in which they were named, in
        original row numbers (Pq.flat_range_among_device); sort=True: ascending in distance, ties in that order.  A row
        named twice is returned twice."""
        return self._range_among(False, queries, rows, radius, sort)

    def similar_above_among(self, queries, rows, threshold, sort=False):
        """similar_above() among the rows that `rows` names -> (lims, score, idx), as within_among(); sort=True:
        descending in score."""
        return self._range_among(True, queries, rows, threshold, sort)

    def embeddings(self, rows):
        """the stored rows of the original row numbers `rows` as float32 [len(rows), d]"""
        import torch
        rows = _on_device(rows, self.rows.device, torch.int64, np.int64).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= len(self)):
            raise PanicError("row numbers must lie in [0, %d)" % len(self))
        return self.rows[self.positions[rows]].to(torch.float32)

    # ---- growth and removal: every method returns a NEW matrix and leaves self and its row filters untouched ----------
    def add(self, vectors):
        """The matrix with `vectors` ([B, d], numpy or CUDA) added as rows len(self) .. len(self) + B - 1, rounded to the
        stored dtype -> a NEW PartitionedFlatMatrix: each vector goes to the end of the list assign() names.  ids and
        rows are merged list by list on the device (Pq.merge_lists_device; rows wider than 4,096 bytes are gathered by
        torch instead).  The result is, tensor for tensor, the matrix the constructor builds from all rows in row order."""
        import torch
        N = len(self)
        x = _device_rows(vectors, self.rows.shape[1], self.rows.device)
        ids_b, off_b = _ivf_layout_device(self.assign(x), self.n_lists)
        rows_b = x.to(self.rows.dtype)[ids_b].contiguous()
        new = self._shell()
        merge = self.pq.merge_lists_device
        new.ids, new.list_off = merge(self.list_off, self.ids, off_b, ids_b + N)
        if self._wide():
            # where original row r is stored in [self.rows; rows_b], gathered in the merged order
            stored = torch.cat([self.positions, _positions(ids_b) + N])
            new.rows = torch.cat([self.rows, rows_b])[stored[new.ids]]
        else:
            new.rows = merge(self.list_off, self.rows, off_b, rows_b)[0]
        new.positions = _positions(new.ids)
        return new

    def compact(self, allow):
        """The matrix of the rows that `allow` keeps (a RowFilter of this matrix, or a bool array [N] in ORIGINAL row
        order) -> (new_matrix, kept): a NEW PartitionedFlatMatrix over the same lists and kept, int64 [N'] on the device,
        the old row number of new row i, ascending; the kept rows are renumbered 0 .. N' - 1 in that order.  Compaction
        is stable in position order, so list l of the result is the kept rows of list l, in order -- tensor for tensor
        what the constructor builds from the kept rows and their assignments (Pq.compact_rows_device under the
        position-order mask; rows wider than 4,096 bytes are selected by torch instead)."""
        import torch
        words = self._keep_words(allow)
        N = len(self)
        flags = self._kept_flags(allow, words)
        rank = torch.cumsum(flags, 0, dtype=torch.int64) - 1
        wide = self._wide()
        outs, list_off, _ = _compact_arrays(self.pq, words, N, [self.ids, None if wide else self.rows], list_off=self.list_off)
        new = self._shell()
        new.rows = self.rows[flags[self.ids].bool()] if wide else outs[1]
        new.ids = rank[outs[0]]
        new.list_off = list_off
        new.positions = _positions(new.ids)
        kept = self.pq.compact_rows_device(self.pq.pack_row_mask_device(flags), None, want_src_rows=True, n=N)[2]
        return new, kept


class GroupFilter:
    """The set of rows a search of a MatrixGroup may return: one RowFilter per part (None for a part without rows), built
    from flags or row numbers in GLOBAL row numbering (MatrixGroup.row_filter); `n_allowed` counts the allowed rows."""

    def __init__(self, group, filters, n_allowed):
        self.group = group
        self.filters = filters
        self.n_allowed = n_allowed


class MatrixGroup:
    """Several resident matrices searched as one.  `parts` is a sequence of QuantizedMatrix, PartitionedMatrix or
    ResidualPartitionedMatrix -- of mixed classes, packed or not, on one device or several.  Global row = bases[p] + the
    part's own row number, bases the running sum of len(part) (int64 [P] on the group's device: `device`, by default the
    first part's).  Results come back on that device.

    A top-k search sends the queries to every part's device, runs the part's own method, gathers the parts' rows into
    one stacked buffer on the group's device and merges them there in one call of Pq.merge_topk_device with
    offsets=bases: the order is (value, part, rank in the part's result), so ties go to the earlier part and ids are
    never compared.  For parts that are consecutive row ranges of one QuantizedMatrix, in order, every search of the
    group is that matrix's search bit for bit.  For partitioned parts (which break ties by position, not by row) it
    is the merge of the parts' own results under that order.  With refine=R the R best rows of the GROUP by the
    estimate are the shortlist -- as one matrix would form it -- and each part re-ranks its members of the shortlist
    against its own attached vectors; the parts' exact results are merged again.

    A range search joins the parts' CSR results per query in part order, ids plus base (Pq.merge_lists_device over
    lims): ascending global row for exhaustive parts in row order, part-major and then each part's stated order for
    list parts; sort=True applies sort_ranges afterwards.

    A FlatMatrix part (rows that are not encoded: a fresh delta) contributes its exact values to a top-k search and to
    the shortlist of refine=R, and re-ranks its members against its own rows, which gives the same numbers; a range
    search of a group with a flat part raises PanicError (the flat classes have within() / similar_above() of their own;
    joining them in here is a follow-up, because it changes what a group does today).  A PartitionedFlatMatrix part (a delta grown large enough to be
    worth lists) does the same over the lists that `nprobe` names.

    add, compact, remove, the *_among searches, persistence and any folding of a small part into a large one stay with
    the parts: MatrixGroup(new_parts) over a replaced part is the way to a changed group."""

    def __init__(self, parts, device=None):
        import torch
        self.parts = list(parts)
        if not self.parts:
            raise PanicError("a group needs at least one part")
        for part in self.parts:
            if not isinstance(part, (QuantizedMatrix, _Lists, FlatMatrix, PartitionedFlatMatrix)):
                raise PanicError("a part must be a QuantizedMatrix, PartitionedMatrix, ResidualPartitionedMatrix, FlatMatrix "
                                 "or PartitionedFlatMatrix")
        if len({part.pq.reconstructed_len() for part in self.parts}) != 1:
            raise PanicError("the parts of a group must hold vectors of one length")
        self.device = self.parts[0].codes.device if device is None else torch.device(device)
        self._bounds = [0]
        for part in self.parts:
            self._bounds.append(self._bounds[-1] + len(part))
        self.bases = torch.tensor(self._bounds[:-1], dtype=torch.int64, device=self.device)
        self._pq = self.parts[0].pq              # its quantizer is not used: the handle the group's own calls run on

    def __len__(self):
        return self._bounds[-1]

    def locate(self, rows):
        """global row numbers (numpy or torch) -> (part, local_row), int64 tensors on the group's device"""
        import torch
        rows = _on_device(rows, self.device, torch.int64, np.int64)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= len(self)):
            raise PanicError("row numbers must lie in [0, %d)" % len(self))
        part = torch.bucketize(rows, self.bases, right=True) - 1
        return part, rows - self.bases[part]

    # ---- filters --------------------------------------------------------------------------------------------------------
    def row_filter(self, allow=None, rows=None, allowed=True):
        """allow: bool [len(self)] in global row numbering, True = the row may be returned; or rows=: global row numbers
        with allowed=True (only these) or allowed=False (all but these) -> GroupFilter for `allow=` of the group's
        searches: one row_filter per part, from the flags or rows split at `bases`."""
        import torch
        if (allow is None) == (rows is None):
            raise PanicError("give either the flags of all rows or a list of row numbers")
        filters, n_allowed = [], 0
        if rows is not None:
            part, local = self.locate(_on_device(rows, self.device, torch.int64, np.int64).reshape(-1))
        else:
            allow = _on_device(allow, self.device)
            if allow.dtype != torch.bool or tuple(allow.shape) != (len(self),):
                raise PanicError("allow must be a bool array with one flag per row (%d)" % len(self))
        for p, m in enumerate(self.parts):
            if len(m) == 0:
                filters.append(None)
                continue
            if rows is not None:
                f = m.row_filter(rows=local[part == p], allowed=allowed)
            else:
                f = m.row_filter(allow[self._bounds[p]:self._bounds[p + 1]])
            filters.append(f)
            n_allowed += f.n_allowed
        return GroupFilter(self, filters, n_allowed)

    def _part_filters(self, allow):
        if allow is None:
            return [None] * len(self.parts)
        if isinstance(allow, GroupFilter):
            if allow.group is not self:
                raise PanicError("the row filter was built for another group")
            return allow.filters
        return self.row_filter(allow).filters

    # ---- searches -------------------------------------------------------------------------------------------------------
    @staticmethod
    def _more(part, nprobe):
        """the arguments a part's search takes besides the group's: nprobe for the classes that have lists"""
        if not isinstance(part, _ListLayout):
            return {}
        if nprobe is None:
            raise PanicError("a group with a partitioned part needs nprobe")
        return {"nprobe": nprobe}

    def _queries(self, queries):
        import torch
        q = _on_device(queries, self.device, torch.float32, np.float32)
        if q.dim() not in (1, 2):
            raise PanicError("queries must be [d] or [nq, d]")
        return q.dim() == 1, (q[None] if q.dim() == 1 else q)

    def _gather(self, width, per_part):
        """per_part(p, part) -> (val, rows) [nq, width] on the part's device, or None for nothing; stacks them on the
        group's device ([P, nq, width], absent = index -1)"""
        import torch
        vals = ids = None
        for p, part in enumerate(self.parts):
            got = per_part(p, part) if len(part) else None
            if vals is None and got is not None:
                nq = got[0].shape[0]
                vals = torch.empty((len(self.parts), nq, width), dtype=torch.float32, device=self.device)
                ids = torch.full((len(self.parts), nq, width), -1, dtype=torch.int64, device=self.device)
            if got is not None:
                vals[p].copy_(got[0])            # torch orders the streams of a copy between devices
                ids[p].copy_(got[1])
        return vals, ids

    def _topk(self, ip, queries, k, nprobe, use_norms, refine, allow):
        import torch
        single, q = self._queries(queries)
        k = int(k)
        filters = self._part_filters(allow)
        R = k
        if refine is not None:
            R = max([part._check_refine(k, refine) for part in self.parts if len(part)], default=int(refine))
        kw = {"use_norms": use_norms} if ip else {}
        qs = [q.to(part.codes.device) for part in self.parts]

        def estimate(p, part):
            fn = part.most_similar if ip else part.nearest
            return fn(qs[p], R, allow=filters[p], **self._more(part, nprobe), **kw)

        vals, ids = self._gather(R, estimate)
        if vals is None:                         # no part holds a row
            val = torch.full((q.shape[0], k), float("-inf") if ip else float("inf"), dtype=torch.float32, device=self.device)
            idx = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=self.device)
            return (val[0], idx[0]) if single else (val, idx)
        if refine is None:
            val, idx = self._pq.merge_topk_device(vals, ids, k, largest=ip, offsets=self.bases)
        else:
            # the group's shortlist, as one matrix forms it; each part re-ranks its members against its own vectors
            _, short, src = self._pq.merge_topk_device(vals, ids, R, largest=ip, offsets=self.bases, want_parts=True)

            def exact(p, part):
                cand = torch.where(src == p, short - self._bounds[p], torch.full_like(short, -1))
                return part._refined(qs[p], cand.to(part.codes.device), k, ip)

            vals, ids = self._gather(k, exact)
            val, idx = self._pq.merge_topk_device(vals, ids, k, largest=ip, offsets=self.bases)
        return (val[0], idx[0]) if single else (val, idx)

    def nearest(self, queries, k, nprobe=None, refine=None, allow=None):
        """the k rows of smallest asymmetric squared distance over all parts -> (dist, idx) [k] or [nq, k], idx global row
        numbers, -1 past the last row (distance +Inf).  nprobe goes to the partitioned parts (required if there is one);
        refine=R needs vectors attached to every part; allow: None, a GroupFilter of this group or a bool array
        [len(self)] in global row numbering."""
        return self._topk(False, queries, k, nprobe, True, refine, allow)

    def most_similar(self, queries, k, nprobe=None, use_norms=True, refine=None, allow=None):
        """the k rows of largest inner product over all parts, largest first -> (score, idx), as nearest()."""
        return self._topk(True, queries, k, nprobe, use_norms, refine, allow)

    def _range(self, ip, queries, threshold, nprobe, use_norms, allow, sort):
        """A group with a flat part still raises: FlatMatrix / PartitionedFlatMatrix have within() / similar_above() now,
        but serving them here changes what the group does today and is left to a follow-up."""
        import torch
        if any(isinstance(part, (FlatMatrix, PartitionedFlatMatrix)) for part in self.parts):
            raise PanicError("a range search over the raw vectors of a FlatMatrix part is not served")
        _, q = self._queries(queries)
        filters = self._part_filters(allow)
        kw = {"use_norms": use_norms} if ip else {}
        lims = val = idx = None
        for p, part in enumerate(self.parts):
            if len(part) == 0:
                continue
            dev = part.codes.device
            thr = threshold.to(dev) if hasattr(threshold, "is_cuda") else threshold
            fn = part.similar_above if ip else part.within
            l, v, r = fn(q.to(dev), thr, allow=filters[p], sort=False, **self._more(part, nprobe), **kw)
            l, v, r = l.to(self.device), v.to(self.device), (r.to(self.device) + self._bounds[p])
            if lims is None:
                lims, val, idx = l, v, r
            else:                                # the queries as lists: rows of query q so far, then this part's
                val, _ = self._pq.merge_lists_device(lims, val.contiguous(), l, v.contiguous())
                idx, lims = self._pq.merge_lists_device(lims, idx.contiguous(), l, r.contiguous())
        if lims is None:
            return (torch.zeros(q.shape[0] + 1, dtype=torch.int64, device=self.device),
                    torch.empty(0, dtype=torch.float32, device=self.device), torch.empty(0, dtype=torch.int64, device=self.device))
        if sort:
            val, idx = sort_ranges(lims, val, idx, ip)
        return lims, val, idx

    def within(self, queries, radius, nprobe=None, allow=None, sort=False):
        """every row of every part within `radius` (a scalar or one value per query) -> (lims, dist, idx), CSR over the
        queries: the rows of a query part by part, inside a part in the part's own order (ascending row for a
        QuantizedMatrix), idx global row numbers.  sort=True: ascending in distance, ties in that order."""
        return self._range(False, queries, radius, nprobe, True, allow, sort)

    def similar_above(self, queries, threshold, nprobe=None, use_norms=True, allow=None, sort=False):
        """every row of every part whose inner product with the query is >= threshold -> (lims, score, idx), as within();
        sort=True: descending in score."""
        return self._range(True, queries, threshold, nprobe, use_norms, allow, sort)

    # ---- lookups --------------------------------------------------------------------------------------------------------
    def embeddings(self, rows):
        """the embeddings of the global row numbers `rows`, in request order -> float32 [len(rows), d] on the group's
        device: the rows are bucketed by part, looked up by each part and scattered back."""
        import torch
        part, local = self.locate(_on_device(rows, self.device, torch.int64, np.int64).reshape(-1))
        out = torch.empty((part.shape[0], self.parts[0].pq.reconstructed_len()), dtype=torch.float32, device=self.device)
        for p, m in enumerate(self.parts):
            sel = torch.nonzero(part == p).reshape(-1)
            if sel.numel():
                out[sel] = m.embeddings(local[sel].to(m.codes.device)).to(self.device)
        return out


def dumps(pq, codes, norms=None):
    b = io.BytesIO()
    write_chunk(b, pq, codes, norms)
    return b.getvalue()
