"""Host-side mirror of reductive's `Pq<f32>` (src/pq/pq.rs:28-348, src/pq/traits.rs:75-156).

Same names, argument meaning and error behaviour as the reference's `QuantizeVector` /
`Reconstruct` traits; the batch methods -- the hot path -- dispatch to libpqhip.so through the
C ABI (include/pqhip.h).  The reference panics on shape errors; here a panic is `PanicError`
carrying the reference's message.  There is no CPU fallback for the batch methods: without the
HIP library or a gfx950 device they raise.

The single-vector methods (`quantize_vector`, `reconstruct`) are the reference's latency path
(pq.rs:285-298, 329-343) and stay on the host, as in the Rust integration.
"""
import ctypes
import threading

import numpy as np

from . import _lib, _marshal
from ._lib import PanicError
from ._marshal import ptr_or_none, row_stride

_INDEX_TYPES = (np.uint8, np.uint16, np.uint32, np.uint64)


class ReductiveError(ValueError):
    """`ReductiveError` (src/error.rs:6-41): invalid training hyper-parameters."""


_default_ctx = None
_ctx_lock = threading.Lock()


class _Ctx:
    def __init__(self, devices=None):
        h = ctypes.c_void_p()
        arr = (ctypes.c_int32 * len(devices))(*devices) if devices else None
        _marshal.run("pqhip_ctx_create", arr, len(devices) if devices else 0, ctypes.byref(h))
        self.handle = h
        self.devices = list(devices) if devices else None
        self.n_devices = _lib.lib().pqhip_ctx_n_devices(h)

    def close(self):
        if self.handle:
            _lib.lib().pqhip_ctx_destroy(self.handle)
            self.handle = None

    def set_option(self, name, value):
        """test / A-B knob (include/pqhip.h: pqhip_ctx_set_option), e.g. ("opq_fused", 0), ("kmeans_window_rows", 64)."""
        rc = _lib.lib().pqhip_ctx_set_option(self.handle, name.encode(), int(value))
        if rc != _lib.OK:
            raise _lib.PqHipError(rc, "pqhip_ctx_set_option(%s)" % name)


def set_option(name, value, ctx=None):
    """pqhip_ctx_set_option on `ctx` (default: the process-wide context)."""
    (ctx or default_ctx()).set_option(name, value)


def launch_log(reset=False):
    """Kernels the library launched from this thread since the last reset ("k_a + k_b x3"; include/pqhip.h)."""
    L = _lib.lib()
    text = L.pqhip_launch_log().decode()
    if reset:
        L.pqhip_launch_log_reset()
    return text


def vor2_tables(quantizers):
    """The candidate tables of the 2-float sub-vector encode kernel for `quantizers` [M][K][2] (or [M][K][1]), built on the host exactly as
    at codebook creation (include/pqhip.h: pqhip_vor2_tables_host; layout: csrc/vor2_prep.h).  Returns (words uint32[],
    region_off uint32[M + 1]) or None when the codebook is not eligible.  Needs no GPU."""
    q = np.ascontiguousarray(quantizers, dtype=np.float32)
    if q.ndim != 3 or q.shape[2] not in (1, 2):
        raise ReductiveError("vor2_tables: quantizers must be [M][K][1] or [M][K][2]")
    L = _lib.lib()
    M, K, dsub = q.shape
    n = ctypes.c_int64(0)
    off = np.zeros(M + 1, dtype=np.uint32)
    rc = L.pqhip_vor2_tables_host(q.ctypes.data, M, K, dsub, None, 0, None, ctypes.byref(n))
    if rc == _lib.EUNSUPPORTED:
        return None
    if rc != _lib.OK:
        raise _lib.PqHipError(rc, "pqhip_vor2_tables_host")
    words = np.zeros(n.value, dtype=np.uint32)
    _marshal.run("pqhip_vor2_tables_host", q.ctypes.data, M, K, dsub, words.ctypes.data, words.size, off.ctypes.data,
                 ctypes.byref(n))
    return words, off


def default_ctx():
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            _default_ctx = _Ctx()
        return _default_ctx


def _estrides(a):
    return [s // a.itemsize for s in a.strides]


def _unrolled_dot_rows(a, b):
    """ndarray numeric_util::unrolled_dot of every row of a [r, n] with b ([n] or [r, n]);
    float32 with separately rounded multiply and add (numpy never fuses)."""
    prod = (a * (b if b.ndim == 2 else b[None, :])).astype(np.float32)
    n = a.shape[1]
    nf = (n // 8) * 8
    p = np.zeros((a.shape[0], 8), np.float32)
    for i in range(0, nf, 8):
        p = p + prod[:, i:i + 8]
    s = np.zeros(a.shape[0], np.float32)
    s = s + (p[:, 0] + p[:, 4])
    s = s + (p[:, 1] + p[:, 5])
    s = s + (p[:, 2] + p[:, 6])
    s = s + (p[:, 3] + p[:, 7])
    for i in range(nf, n):
        s = s + prod[:, i]
    return s


def _first_min(d):
    """kmeans.rs:119-125: first minimum under ordered-float (NaN greatest, -0 == +0)."""
    ok = ~np.isnan(d)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (d == d[ok].min()))[0])


def cluster_assignments(centroids, instances, dtype=np.uint64, ctx=None):
    """`kmeans::cluster_assignments(centroids, instances, Axis(0))` (src/kmeans.rs:133-159) on the
    GPU: index of the nearest centroid [K, dim] for every row of `instances` [n, dim]."""
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    x = np.asarray(instances, dtype=np.float32)
    if centroids.ndim != 2 or x.ndim != 2 or x.shape[1] != centroids.shape[1]:
        raise PanicError("Cannot compute (squared) euclidean distance of matrices with different "
                         "numbers of columns.")                                  # linalg.rs:161-165
    out = np.zeros(x.shape[0], dtype=dtype)
    if x.shape[0] == 0:
        return out
    if any(s < 0 for s in x.strides) or any(s % 4 for s in x.strides):
        x = np.ascontiguousarray(x)
    rs, cs = _estrides(x)
    ctx = ctx or default_ctx()
    fp = ctypes.POINTER(ctypes.c_float)
    _marshal.run("pqhip_cluster_assignments_f32", ctx.handle, centroids.ctypes.data_as(fp), centroids.shape[0],
                 centroids.shape[1], x.ctypes.data, x.shape[0], rs, cs, out.ctypes.data, out.itemsize)
    return out


def kmeans_iterations(quantizers, instances, n_iterations=1, want_loss=True, ctx=None):
    """`n_iterations` x `kmeans_iteration` (src/kmeans.rs:308-327) on every subquantizer's column
    block, on the GPU: the body of `kmeans_with_centroids(.., NIterationsCondition(n))` at
    pq.rs:176 for all subquantizers of `train_pq_using`, and of `Opq::update_subquantizers`
    (opq.rs:227-245) when n_iterations == 1.  quantizers [M, K, dsub] are the initial centroids;
    returns (updated quantizers, last mean squared error per subquantizer or None).
    `instances` may be a numpy array [n, d] or a CUDA float32 torch tensor (kept in HBM)."""
    q = np.array(quantizers, dtype=np.float32, order="C", copy=True)
    if q.ndim == 2:
        q = q[None]
    if not hasattr(instances, "is_cuda"):
        instances = np.asarray(instances, dtype=np.float32)
    if q.ndim != 3 or q.shape[1] == 0:
        raise PanicError("Cannot cluster instances with zero centroids.")        # kmeans.rs:260-263
    M, K, dsub = q.shape
    if instances.ndim != 2 or instances.shape[1] != M * dsub:
        raise PanicError("Centroid and instance lengths differ.")                # kmeans.rs:264-268
    ctx = ctx or default_ctx()
    loss = np.zeros(M, np.float32) if want_loss else None
    fp = ctypes.POINTER(ctypes.c_float)
    lp = loss.ctypes.data_as(fp) if want_loss else None
    L = _lib.lib()
    if hasattr(instances, "is_cuda"):
        import torch
        x = instances
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
        if x.shape[1] != M * dsub:
            raise PanicError("Centroid and instance lengths differ.")            # kmeans.rs:264-268
        if x.stride(1) != 1:
            x = x.contiguous()
        dev = x.device.index or 0
        slot = dev if ctx.devices is None else ctx.devices.index(dev)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rs = row_stride(x, x.shape[0], x.shape[1])
        rc = L.pqhip_kmeans_iterations_f32_dev(ctx.handle, slot, q.ctypes.data_as(fp), M, K, dsub,
                                               x.data_ptr(), x.shape[0], rs, n_iterations, lp,
                                               ctypes.c_void_p(stream))
    else:
        x = np.asarray(instances, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != M * dsub:
            raise PanicError("Centroid and instance lengths differ.")            # kmeans.rs:264-268
        if any(s < 0 for s in x.strides) or any(s % 4 for s in x.strides):
            x = np.ascontiguousarray(x)
        rs, cs = _estrides(x) if x.size else (x.shape[1], 1)
        rc = L.pqhip_kmeans_iterations_f32(ctx.handle, q.ctypes.data_as(fp), M, K, dsub, x.ctypes.data,
                                           x.shape[0], rs, cs, n_iterations, lp)
    if rc != _lib.OK:
        raise _lib.PqHipError(rc, "pqhip_kmeans_iterations_f32")
    return q, loss


def train_pq(n_subquantizers, n_subquantizer_bits, n_iterations, n_attempts, instances, rng=None, ctx=None):
    """`Pq::train_pq_using` (src/pq/pq.rs:214-241 -> train_subquantizer pq.rs:144-188) with the
    k-means iterations on the GPU.  Initial centroids are K distinct random instances per
    subquantizer (RandomInstanceCentroids, pq.rs:166-172); the draw uses numpy's generator, not the
    reference's XorShift stream, so trained codebooks agree with the reference statistically, not
    bit for bit.  The best of `n_attempts` (lowest final loss, first on ties) is kept per subquantizer."""
    x = np.asarray(instances, dtype=np.float32)
    n, d = x.shape
    K = 1 << n_subquantizer_bits
    # check_quantizer_invariants (pq.rs:63-100), same order, messages of error.rs:6-41
    if n_subquantizers == 0 or n_subquantizers > d:
        raise ReductiveError("The number of subquantizers must be between 1 and %d, was %d" % (d, n_subquantizers))
    max_bits = int(np.trunc(np.log2(float(n)))) if n > 0 else 0
    if n_subquantizer_bits == 0 or n_subquantizer_bits > max_bits:
        raise ReductiveError("The number of subquantizers bits must be between 1 and %d" % max_bits)
    if d % n_subquantizers != 0:
        # (the reference's format string swaps the two numbers, error.rs:19-23; kept as is)
        raise ReductiveError("The number of columns (%d) is not exactly dividable by the number of "
                             "subquantizers (%d)" % (n_subquantizers, d))
    if n_iterations == 0:
        raise ReductiveError("The number of quantization iterations must be >= 1")
    if n_attempts == 0:
        raise ReductiveError("The number of quantization attempts per iteration must be >= 1")
    rng = rng or np.random.default_rng(0)
    M, dsub = n_subquantizers, d // n_subquantizers
    best_q, best_loss = None, None
    for _ in range(n_attempts):
        init = np.stack([x[rng.choice(n, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)])
        q, loss = kmeans_iterations(init, x, n_iterations, want_loss=True, ctx=ctx)
        if best_q is None:
            best_q, best_loss = q, loss
        else:
            better = np.array([(not np.isnan(l)) and (np.isnan(b) or l < b) for l, b in zip(loss, best_loss)])
            best_q[better] = q[better]
            best_loss[better] = loss[better]
    return Pq(None, best_q, ctx=ctx)


def at_dot_b(a, b, ctx=None):
    """`a.t().dot(&b)` (opq.rs:191) for CUDA float32 tensors a [n, da], b [n, db] on the GPU with the
    reference's summation order over the rows; returns a numpy [da, db] array."""
    import torch
    assert a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32
    assert a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.stride(1) == 1 and b.stride(1) == 1
    ctx = ctx or default_ctx()
    dev = a.device.index or 0
    slot = dev if ctx.devices is None else ctx.devices.index(dev)
    out = np.zeros((a.shape[1], b.shape[1]), np.float32)
    rs = lambda t: row_stride(t, t.shape[0], t.shape[1])
    _marshal.run("pqhip_at_dot_b_f32_dev", ctx.handle, slot, a.data_ptr(), rs(a), a.shape[1], b.data_ptr(), rs(b),
                 b.shape[1], a.shape[0], out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                 ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream))
    return out


def opq_train_step(quantizers, projection, instances, ctx=None):
    """The device part of `Opq::train_iteration` (opq.rs:156-195): rotation, one k-means iteration
    per subquantizer, the quantize -> reconstruct round trip and `instances.t().dot(&reconstructed)`.
    instances: CUDA float32 tensor [n, d].  Returns (updated quantizers, cross [d, d]); the caller
    finishes with `u, _, vt = svd(cross); projection = u @ vt` (opq.rs:191-192)."""
    import torch
    q = np.array(quantizers, dtype=np.float32, order="C", copy=True)
    if q.ndim != 3 or q.size == 0:
        raise PanicError("Cannot cluster instances with zero centroids.")
    M, K, dsub = q.shape
    d = M * dsub
    P = np.ascontiguousarray(projection, dtype=np.float32)
    if list(P.shape) != [d, d]:
        raise PanicError("Incorrect projection matrix shape, was: %s, should be [%d, %d]" % (list(P.shape), d, d))
    x = instances
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    if x.shape[1] != d:
        raise PanicError("Centroid and instance lengths differ.")
    if x.stride(1) != 1:
        x = x.contiguous()
    ctx = ctx or default_ctx()
    dev = x.device.index or 0
    slot = dev if ctx.devices is None else ctx.devices.index(dev)
    cross = np.zeros((d, d), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    _marshal.run("pqhip_opq_train_step_f32_dev", ctx.handle, slot, q.ctypes.data_as(fp), M, K, dsub, P.ctypes.data_as(fp),
                 x.data_ptr(), x.shape[0], row_stride(x, x.shape[0], d), cross.ctypes.data_as(fp),
                 ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    return q, cross


def bucket_eigenvalues(eigenvalues, n_buckets):
    """`bucket_eigenvalues` (opq.rs:198-273): eigenvalue allocation of Ge et al. 2013 -- largest
    first, each to the non-full bucket whose product (sum of shifted logs) is smallest."""
    ev = np.asarray(eigenvalues, dtype=np.float32)
    if n_buckets <= 0:
        raise PanicError("Cannot distribute eigenvalues over zero buckets.")
    if ev.shape[0] < n_buckets:
        raise PanicError("At least one eigenvalue is required per bucket")
    if ev.shape[0] % n_buckets != 0:
        raise PanicError("The number of eigenvalues should be a multiple of the number of buckets.")
    order = sorted(range(ev.shape[0]), key=lambda i: (np.isnan(ev[i]), ev[i]))     # ascending, NaN last
    eps = np.finfo(np.float32).eps
    if not ev[order[0]] >= -eps:
        raise PanicError("Bucketing is only supported for positive eigenvalues.")
    logs = np.log(ev + eps).astype(np.float32)
    logs = (logs - logs.min()).astype(np.float32)
    assignments = [[] for _ in range(n_buckets)]
    products = [np.float32(0)] * n_buckets
    cap = ev.shape[0] // n_buckets
    while order:
        i = order.pop()
        open_buckets = [b for b in range(n_buckets) if len(assignments[b]) < cap]
        b = min(open_buckets, key=lambda k: (products[k], k))                          # first minimum
        assignments[b].append(i)
        products[b] = np.float32(products[b] + logs[i])
    return assignments


def create_projection_matrix(instances, n_subquantizers):
    """`Opq::create_projection_matrix` (opq.rs:101-137): eigenvectors of the covariance matrix
    (linalg.rs:23-44, LAPACK `eigh`, upper triangle), columns ordered by `bucket_eigenvalues`."""
    x = np.asarray(instances, dtype=np.float32)
    n, d = x.shape
    if n == 0:
        raise PanicError("Cannot compute a covariance from zero observations")
    centered = x - x.mean(axis=0, dtype=np.float32)
    cov = (centered.T @ (centered / np.float32(n - 1))).astype(np.float32)
    evals, evecs = np.linalg.eigh(cov, UPLO="U")
    P = np.zeros((d, d), np.float32)
    for col, direction in enumerate(i for b in bucket_eigenvalues(evals, n_subquantizers) for i in b):
        P[:, col] = evecs[:, direction]
    return P


def set_rotation_variant(variant):
    """test knob (include/pqhip.h: pqhip_set_rotation_variant), process-wide: 0 auto, 8 / 9 force that rotation kernel."""
    _marshal.run("pqhip_set_rotation_variant", variant)


def rotate(instances, projection, ctx=None):
    """`instances.dot(&projection)` (opq.rs:62, gaussian_opq.rs:55) on the GPU with the reference's
    summation order; CUDA float32 tensor [n, d] in, CUDA tensor out."""
    import torch
    x = instances
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
    if x.stride(1) != 1:
        x = x.contiguous()
    d = x.shape[1]
    P = np.ascontiguousarray(projection, dtype=np.float32)
    if list(P.shape) != [d, d]:
        raise PanicError("Incorrect projection matrix shape, was: %s, should be [%d, %d]" % (list(P.shape), d, d))
    ctx = ctx or default_ctx()
    dev = x.device.index or 0
    slot = dev if ctx.devices is None else ctx.devices.index(dev)
    out = torch.empty((x.shape[0], d), dtype=torch.float32, device=x.device)
    _marshal.run("pqhip_rotate_f32_dev", ctx.handle, slot, x.data_ptr(), x.shape[0], row_stride(x, x.shape[0], d), d,
                 P.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.data_ptr(), d,
                 ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    return out


def train_gaussian_opq(n_subquantizers, n_subquantizer_bits, n_iterations, n_attempts, instances, rng=None, ctx=None):
    """`GaussianOpq::train_pq_using` (gaussian_opq.rs:33-68): the PCA / eigenvalue-allocation
    projection of `create_projection_matrix`, then a plain PQ trained on the rotated instances
    (rotation and k-means on the GPU)."""
    import torch
    x = np.asarray(instances, dtype=np.float32)
    if x.ndim != 2 or n_subquantizers == 0 or n_subquantizers > x.shape[1]:
        raise ReductiveError("The number of subquantizers must be between 1 and %d, was %d"
                             % (x.shape[1] if x.ndim == 2 else 0, n_subquantizers))
    if x.shape[1] % n_subquantizers != 0:
        raise ReductiveError("The number of columns (%d) is not exactly dividable by the number of "
                             "subquantizers (%d)" % (n_subquantizers, x.shape[1]))
    P = create_projection_matrix(x, n_subquantizers)
    ctx = ctx or default_ctx()
    dev = torch.device("cuda", (ctx.devices[0] if ctx.devices else 0))
    rx = rotate(torch.from_numpy(np.ascontiguousarray(x)).to(dev), P, ctx=ctx).cpu().numpy()
    pq = train_pq(n_subquantizers, n_subquantizer_bits, n_iterations, n_attempts, rx, rng=rng, ctx=ctx)
    return Pq(P, pq.subquantizers(), ctx=ctx)


def train_opq(n_subquantizers, n_subquantizer_bits, n_iterations, n_attempts, instances, rng=None, ctx=None):
    """`Opq::train_pq_using` (opq.rs:44-99) with every data-sized step on the GPU: the iteration's
    rotation, k-means update, quantize -> reconstruct round trip and cross product run in
    `opq_train_step`; what stays on the host is LAPACK (covariance eigen-decomposition for the
    initial projection, opq.rs:101-137; one d x d SVD per iteration, opq.rs:191-192) and the
    random draw of the initial centroids (numpy's generator, not the reference's stream).
    `n_attempts` has no effect, as in the reference (opq.rs:34-36)."""
    import torch
    x = np.asarray(instances, dtype=np.float32)
    n, d = x.shape
    M, K = n_subquantizers, 1 << n_subquantizer_bits
    if M == 0 or M > d:
        raise ReductiveError("The number of subquantizers must be between 1 and %d, was %d" % (d, M))
    max_bits = int(np.trunc(np.log2(float(n)))) if n > 0 else 0
    if n_subquantizer_bits == 0 or n_subquantizer_bits > max_bits:
        raise ReductiveError("The number of subquantizers bits must be between 1 and %d" % max_bits)
    if d % M != 0:
        raise ReductiveError("The number of columns (%d) is not exactly dividable by the number of "
                             "subquantizers (%d)" % (M, d))
    if n_iterations == 0:
        raise ReductiveError("The number of quantization iterations must be >= 1")
    rng = rng or np.random.default_rng(0)
    dsub = d // M
    P = create_projection_matrix(x, M)
    # initial centroids: K distinct rows of rx per subquantizer (opq.rs:139-158)
    q = np.stack([(x[rng.choice(n, K, replace=False)] @ P)[:, m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    ctx = ctx or default_ctx()
    dev = torch.device("cuda", (ctx.devices[0] if ctx.devices else 0))
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for _ in range(n_iterations):
        q, cross = opq_train_step(q, P, xd, ctx=ctx)
        u, _, vt = np.linalg.svd(cross)                                                   # opq.rs:191
        P = (u @ vt).astype(np.float32)                                                   # opq.rs:192
    return Pq(P, q, ctx=ctx)


def pack_codes4(codes, n_centroids=16):
    """codes: integer array [n, M] (or [M]) of a quantizer with n_centroids <= 16 -> the 4-bit packed rows, uint8
    [n, ceil(M / 2)]: code m lives in byte m >> 1, even m in the low nibble and odd m in the high nibble; the high nibble
    of the last byte of an odd M is 0 (include/pqhip.h, "4-bit packed codes").  Raises on a code >= n_centroids."""
    if n_centroids > 16:
        raise PanicError("4-bit packed codes need a quantizer of at most 16 centroids")
    c = np.asarray(codes)
    single = c.ndim == 1
    c = np.atleast_2d(c)
    if c.ndim != 2 or c.dtype.kind not in "ui":
        raise PanicError("codes must be an integer array [n, n_subquantizers]")
    if c.size and (int(c.min()) < 0 or int(c.max()) >= n_centroids):
        raise PanicError("ndarray: index out of bounds")
    n, M = c.shape
    even = np.zeros((n, (M + 1) // 2), dtype=np.uint8)
    odd = np.zeros_like(even)
    even[:, :] = c[:, 0::2]
    odd[:, :M // 2] = c[:, 1::2]
    out = even | (odd << 4)
    return out[0] if single else out


def unpack_codes4(packed, n_subquantizers):
    """The inverse of pack_codes4: uint8 [n, ceil(M / 2)] (or [ceil(M / 2)]) -> uint8 [n, M].  The pad nibble of an odd M
    is ignored whatever it holds."""
    p = np.asarray(packed)
    single = p.ndim == 1
    p = np.atleast_2d(p)
    M = int(n_subquantizers)
    if p.ndim != 2 or p.dtype != np.uint8 or p.shape[1] != (M + 1) // 2:
        raise PanicError("4-bit packed codes must be uint8 [n, ceil(n_subquantizers / 2)]")
    out = np.empty((p.shape[0], M), dtype=np.uint8)
    out[:, 0::2] = p & 0xf
    out[:, 1::2] = (p >> 4)[:, :M // 2]
    return out[0] if single else out


# ---- exact search for query batches: the pure rules of Pq.flat_search_batch_device ------------------------------------
FLAT_SCREEN_MAX_D = 2048                 # pqhip_flat_screen_f32_dev serves d <= 2048
FLAT_SCREEN_MAX_EXP = 40                 # |x_exp| the screen's proof covers
FLAT_SCREEN_ELEMENT_TOP = 13             # the largest scaled |element| lands in [2^13, 2^14): a factor 2 below the 2^15 of the contract
FLAT_BATCH_FALLBACK_FRACTION = 1.0 / 16  # candidates of a chunk beyond this share of n nq: the plain call
FLAT_BATCH_CHUNK = 256                   # queries per screen call of the batch search


def flat_screen_x_exp(max_abs):
    """x_exp for a matrix whose largest |element| is max_abs: 2^x_exp max_abs in [2^13, 2^14), clamped to +-40; 0 for a
    zero, NaN or infinite maximum (the screen is sound under any x_exp; this choice keeps it tight)."""
    m = float(max_abs)
    if not (m > 0.0) or m == float("inf"):
        return 0
    import math
    e = FLAT_SCREEN_ELEMENT_TOP - (math.frexp(m)[1] - 1)        # frexp: m = f 2^e, f in [0.5, 1)
    return max(-FLAT_SCREEN_MAX_EXP, min(FLAT_SCREEN_MAX_EXP, e))


def flat_batch_sample(n, k):
    """(S, t): the sample of the batch search is rows 0, t, 2 t, .. -- about S = 2 sqrt(n k) of them (at least 4 k, at
    most n), which balances the sample's cost (nq S rows) against the resolve's (about nq n k / S rows)."""
    import math
    n, k = int(n), int(k)
    if n <= 0:
        return 0, 1
    S = min(n, max(4 * k, int(math.ceil(2.0 * math.sqrt(float(n) * k)))))
    t = max(1, n // S)
    return (n + t - 1) // t, t


def flat_batch_capacity(n, nq, k, S):
    """ids allocated for one screen call of the batch search: the fallback limit -- a larger result falls back anyway,
    so the call is never repeated."""
    return int(FLAT_BATCH_FALLBACK_FRACTION * n * nq) + 1


def flat_batch_falls_back(total, n, nq):
    """a chunk of nq queries with `total` candidates takes the plain call when they exceed the stated share of n nq"""
    return total > FLAT_BATCH_FALLBACK_FRACTION * n * nq


def _matrix_max_abs(vectors):
    """largest finite |element| of a CUDA matrix as a float (two reductions without a temporary and one
    synchronisation; a matrix with NaN or infinite elements is reduced again in row chunks over its finite elements)"""
    import torch
    if vectors.numel() == 0:
        return 0.0
    lo, hi = torch.aminmax(vectors)
    m = max(-float(lo), float(hi))
    if m == m and m != float("inf"):
        return m
    m = 0.0
    for r0 in range(0, vectors.shape[0], 1 << 18):
        a = vectors[r0:r0 + (1 << 18)].abs()
        m = max(m, float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max()))
    return m


class Pq:
    """Product quantizer (Jegou et al., 2011) -- mirror of `reductive::pq::Pq<f32>`."""

    def __init__(self, projection, quantizers, ctx=None):
        """`Pq::new(projection, quantizers)` (pq.rs:38-61)."""
        quantizers = np.ascontiguousarray(quantizers, dtype=np.float32)
        if quantizers.ndim != 3 or quantizers.size == 0:
            raise PanicError("Attempted to construct a product quantizer without quantizers.")
        rl = quantizers.shape[0] * quantizers.shape[2]
        if projection is not None:
            projection = np.ascontiguousarray(projection, dtype=np.float32)
            if list(projection.shape) != [rl, rl]:
                raise PanicError("Incorrect projection matrix shape, was: %s, should be [%d, %d]"
                                 % (list(projection.shape), rl, rl))
        self._projection = projection
        self._quantizers = quantizers
        self._ctx = ctx
        self._handle = None
        self._lock = threading.Lock()

    # ---- accessors (pq.rs:103-110, 191-193) -------------------------------------------------
    def n_quantizer_centroids(self):
        return self._quantizers.shape[1]

    def projection(self):
        return self._projection

    def subquantizers(self):
        return self._quantizers

    def quantized_len(self):
        return self._quantizers.shape[0]

    def reconstructed_len(self):
        return self._quantizers.shape[0] * self._quantizers.shape[2]

    def __eq__(self, other):  # #[derive(PartialEq)] pq.rs:28 -- value equality, handle excluded
        if not isinstance(other, Pq):
            return NotImplemented
        pe = (self._projection is None) == (other._projection is None)
        if pe and self._projection is not None:
            pe = np.array_equal(self._projection, other._projection)
        return pe and np.array_equal(self._quantizers, other._quantizers)

    # ---- device handle (created lazily, cached; SURVEY.md section 8b "Ownership") -------------
    def _cb(self):
        with self._lock:
            if self._handle is None:
                ctx = self._ctx or default_ctx()
                M, K, dsub = self._quantizers.shape
                fp = ctypes.POINTER(ctypes.c_float)
                h = ctypes.c_void_p()
                proj = self._projection.ctypes.data_as(fp) if self._projection is not None else None
                _marshal.run("pqhip_codebook_create", ctx.handle, self._quantizers.ctypes.data_as(fp), M, K, dsub, proj,
                             ctypes.byref(h))
                self._handle = h
                self._ctx = ctx
            return self._handle

    def close(self):
        with self._lock:
            if self._handle is not None:
                _lib.lib().pqhip_codebook_destroy(self._handle)
                self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_encode_variant(self, variant):
        """test/bench knob: force an encode kernel family on this handle (0 = auto); the variants are described at
        pqhip_set_encode_variant in include/pqhip.h."""
        rc = _lib.lib().pqhip_set_encode_variant(self._cb(), variant)
        if rc != _lib.OK:
            raise _lib.PqHipError(rc)

    def last_encode_kernel(self):
        return _lib.lib().pqhip_last_encode_kernel(self._cb()).decode()

    # ---- QuantizeVector (traits.rs:75-99) -----------------------------------------------------
    def quantize_batch(self, x, dtype=np.uint8):
        """`quantize_batch::<I, _>(x)` (pq.rs:256-265); `dtype` plays the role of `I`."""
        x = np.asarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise PanicError("quantize_batch expects a matrix")
        quantized = np.zeros((x.shape[0], self.quantized_len()), dtype=dtype)
        self.quantize_batch_into(x, quantized)
        return quantized

    def quantize_batch_into(self, x, quantized):
        """`quantize_batch_into` (pq.rs:268-283 -> primitives.rs:64-104) on the GPU."""
        x = np.asarray(x, dtype=np.float32)
        if quantized.dtype.type not in _INDEX_TYPES:
            raise TypeError("index type must be one of u8/u16/u32/u64")
        if x.ndim != 2 or x.shape[1] != self.reconstructed_len():
            raise PanicError("Quantizer and vector length mismatch")            # primitives.rs:74-78
        if quantized.shape != (x.shape[0], self.quantized_len()):
            raise PanicError("Quantized matrix has incorrect shape, expected: (%d, %d), got: (%d, %d)"
                             % (x.shape[0], self.quantized_len(), quantized.shape[0],
                                quantized.shape[1] if quantized.ndim > 1 else 0))  # primitives.rs:80-87
        if x.shape[0] == 0:
            return
        if any(s < 0 for s in x.strides) or any(s % 4 for s in x.strides):
            x = np.ascontiguousarray(x)
        if any(s < 0 for s in quantized.strides):
            raise ValueError("negative output strides are not supported")
        rs, cs = _estrides(x)
        ors, ocs = _estrides(quantized)
        rc = _lib.lib().pqhip_quantize_batch_f32(self._cb(), x.ctypes.data, x.shape[0], rs, cs,
                                                quantized.ctypes.data, quantized.itemsize, ors, ocs)
        if rc == _lib.EINDEX_WIDTH:
            # the batch path of the reference has no such assert (it silently wraps,
            # primitives.rs:98-100); the GPU entry point refuses instead -- see DESIGN.md
            raise PanicError("Cannot store centroids in quantizer index type")
        if rc != _lib.OK:
            raise _lib.PqHipError(rc, "pqhip_quantize_batch_f32")

    def quantize_vector(self, x, dtype=np.uint8):
        """`quantize_vector` (pq.rs:285-298 -> primitives.rs:14-49 -> linalg.rs:118-148); host."""
        x = np.asarray(x, dtype=np.float32)
        if x.ndim != 1 or x.shape[0] != self.reconstructed_len():
            raise PanicError("Quantizer and vector length mismatch")            # primitives.rs:25-29
        K = self.n_quantizer_centroids()
        if K - 1 > np.iinfo(dtype).max:
            raise PanicError("Cannot store centroids in quantizer index type")  # primitives.rs:31-34
        if self._projection is not None:
            # 1-D x 2-D ndarray dot without BLAS: sequential  s = s + x[k]*P[k,c]  per column
            rx = np.zeros(x.shape[0], np.float32)
            for k in range(x.shape[0]):
                rx = rx + x[k] * self._projection[k]
            x = rx
        M, _, dsub = self._quantizers.shape
        out = np.zeros(M, dtype=dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            for m in range(M):
                xs = x[m * dsub:(m + 1) * dsub]
                c = self._quantizers[m]
                xx = _unrolled_dot_rows(xs[None, :], xs)[0]
                cc = _unrolled_dot_rows(c, c)
                dp = _unrolled_dot_rows(c, xs)
                d = (xx + cc) - (dp + dp)
                out[m] = _first_min(d.astype(np.float32))
        return out

    # ---- Reconstruct (traits.rs:102-156) ------------------------------------------------------
    def reconstruct_batch(self, quantized):
        """`reconstruct_batch` default method (traits.rs:109-117)."""
        quantized = np.asarray(quantized)
        if quantized.ndim != 2:
            raise PanicError("reconstruct_batch expects a matrix")
        out = np.zeros((quantized.shape[0], self.reconstructed_len()), np.float32)
        self.reconstruct_batch_into(quantized, out)
        return out

    def reconstruct_batch_into(self, quantized, reconstructions):
        """`reconstruct_batch_into` (pq.rs:309-327 -> primitives.rs:150-173) on the GPU."""
        quantized = np.asarray(quantized)
        if quantized.dtype.kind == "i":
            if (quantized < 0).any():
                raise PanicError("negative code")
            quantized = quantized.astype(np.uint64)
        if quantized.dtype.type not in _INDEX_TYPES:
            raise TypeError("index type must be one of u8/u16/u32/u64")
        if reconstructions.dtype != np.float32:
            raise TypeError("reconstructions must be float32")
        if (quantized.ndim != 2 or reconstructions.ndim != 2
                or reconstructions.shape[0] != quantized.shape[0]
                or reconstructions.shape[1] != self.reconstructed_len()):
            raise PanicError("Reconstructions matrix has incorrect shape, expected: (%d, %d), got: (%d, %d)"
                             % (quantized.shape[0], self.reconstructed_len(),
                                reconstructions.shape[0], reconstructions.shape[-1]))  # primitives.rs:159-167
        if quantized.shape[1] != self.quantized_len():
            raise PanicError("Quantization length does not match number of subquantizers")  # primitives.rs:123-127
        if quantized.shape[0] == 0:
            return
        if any(s < 0 for s in quantized.strides):
            quantized = np.ascontiguousarray(quantized)
        if any(s < 0 for s in reconstructions.strides):
            raise ValueError("negative output strides are not supported")
        crs, ccs = _estrides(quantized)
        ors, ocs = _estrides(reconstructions)
        rc = _lib.lib().pqhip_reconstruct_batch_f32(self._cb(), quantized.ctypes.data,
                                                   quantized.itemsize, quantized.shape[0], crs, ccs,
                                                   reconstructions.ctypes.data, ors, ocs)
        if rc == _lib.ECODE_RANGE:
            raise PanicError("ndarray: index out of bounds")                    # primitives.rs:146
        if rc != _lib.OK:
            raise _lib.PqHipError(rc, "pqhip_reconstruct_batch_f32")

    def reconstruct(self, quantized):
        """`reconstruct` (traits.rs:133-141 -> pq.rs:329-343); single vector, host."""
        quantized = np.asarray(quantized)
        if quantized.ndim != 1 or quantized.shape[0] != self.quantized_len():
            raise PanicError("Quantization length does not match number of subquantizers")
        K = self.n_quantizer_centroids()
        if (quantized.astype(np.int64) < 0).any() or (quantized.astype(np.uint64) >= K).any():
            raise PanicError("ndarray: index out of bounds")
        rec = np.concatenate([self._quantizers[m, int(c)] for m, c in enumerate(quantized)])
        if self._projection is not None:
            # reconstruction.dot(&projection.t()): per output k a contiguous dot with row P[k,:]
            rec = _unrolled_dot_rows(self._projection, rec.astype(np.float32))
        return rec.astype(np.float32)

    # ---- device-resident variants (torch tensors in HBM; used by bench.py and the GPU tests) ----
    # Every wrapper below: normalise the arguments, allocate, call, optionally check the range flag, shape the result.
    # The marshalling they share is reductive_amd/_marshal.py.
    def _slot_for(self, tensor):
        ctx = self._ctx or default_ctx()
        dev = tensor.device.index or 0
        if ctx.devices is None:
            return dev
        return ctx.devices.index(dev)

    def _reconstructions(self, out, n, device):
        """The float32 [n, d] output of the three reconstruct calls, allocated unless given."""
        import torch
        d = self.reconstructed_len()
        if out is None:
            out = torch.empty((n, d), dtype=torch.float32, device=device)
        assert out.is_cuda and out.dtype == torch.float32 and out.stride(1) == 1
        if tuple(out.shape) != (n, d):
            raise PanicError("Reconstructions matrix has incorrect shape, expected: (%d, %d), got: (%d, %d)"
                             % (n, d, out.shape[0], out.shape[1]))
        return out, row_stride(out, n, d)

    def quantize_batch_device(self, x, out=None, stream=None):
        """x: CUDA float32 tensor [n, d] (unit column stride) -> codes tensor [n, M] (uint8; int32 when K > 256).
        Asynchronous on torch's current stream unless `stream` (a raw hipStream_t int) is given."""
        import torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
        if x.shape[1] != self.reconstructed_len():
            raise PanicError("Quantizer and vector length mismatch")
        x = _marshal.unit_columns(x)
        n, M = x.shape[0], self.quantized_len()
        if out is None:
            # u8 codes, or 32-bit codes (int32 tensor, values < 2^31) when K > 256
            dt = torch.uint8 if self.n_quantizer_centroids() <= 256 else torch.int32
            out = torch.empty((n, M), dtype=dt, device=x.device)
        if tuple(out.shape) != (n, M):
            raise PanicError("Quantized matrix has incorrect shape, expected: (%d, %d), got: (%d, %d)"
                             % (n, M, out.shape[0], out.shape[1]))
        # index type I of quantize_batch::<I, _>: uint8, or int16 / int32 / int64 tensors as 2- / 4- / 8-byte containers
        # (u16 / u32 / u64 bit patterns)
        assert out.is_cuda and out.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64) and out.stride(1) == 1
        cb, slot, sp = _marshal.launch(self, x, stream)
        _marshal.run("pqhip_quantize_batch_f32_dev", cb, slot, x.data_ptr(), n, row_stride(x, n, x.shape[1]),
                     out.data_ptr(), out.element_size(), row_stride(out, n, M), sp, panics=_marshal.WIDTH_PANIC)
        return out

    def reconstruct_batch_device(self, codes, out=None, stream=None, check=True):
        """codes: CUDA uint8 (or int16 / int32 / int64 = u16 / u32 / u64 containers) tensor [n, M] -> float32 tensor [n, d].
        check=True (default) synchronises the stream and raises the reference's index panic
        (primitives.rs:146) when a code >= K was met; check=False leaves the call asynchronous and the
        violation pending on the stream's flag (a later check=True call on that stream reports it)."""
        import torch
        assert codes.is_cuda and codes.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64) and codes.dim() == 2
        codes, n, c_rs = _marshal.codes_arg(codes, _marshal.code_width(codes, self.quantized_len()))
        out, o_rs = self._reconstructions(out, n, codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run("pqhip_reconstruct_batch_f32_dev", cb, slot, codes.data_ptr(), codes.element_size(), n, c_rs,
                     out.data_ptr(), o_rs, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    def reconstruct_rows_device(self, codes, rows, scales=None, out=None, stream=None, check=True):
        """Lookup path of a resident quantized matrix ("next" row):
        `reconstruct_batch(codes.select(Axis(0), rows)) * scales.select(rows)` in one pass.
        codes: CUDA uint8 [N, M]; rows: CUDA int64 [n]; scales: None or CUDA float32 [N]."""
        import torch
        assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2
        assert rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()
        codes, N, c_rs = _marshal.codes_arg(codes, _marshal.code_width(codes, self.quantized_len()))
        _marshal.per_row_arg(scales, N, "scales")
        n = rows.shape[0]
        out, o_rs = self._reconstructions(out, n, codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run("pqhip_reconstruct_rows_f32_dev", cb, slot, codes.data_ptr(), 1, N, c_rs, rows.data_ptr(), n,
                     ptr_or_none(scales), out.data_ptr(), o_rs, sp, panics=_marshal.RANGE_PANIC)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    @staticmethod
    def interleave_records(codes, scales, record_bytes=None):
        """Resident-matrix layout with ONE cache line per lookup: CUDA uint8 [N, record_bytes] records holding the M code
        bytes of a row at offset 0 and its f32 scale at the next multiple of 16 bytes (32-byte records at M = 15).
        Returns (records, scale_offset_bytes)."""
        import torch
        assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2
        assert scales.is_cuda and scales.dtype == torch.float32 and scales.shape == (codes.shape[0],)
        m = codes.shape[1]
        off = (m + 15) // 16 * 16
        rb = record_bytes or max(32, 1 << (off + 4 - 1).bit_length())
        assert rb % 4 == 0 and off + 4 <= rb
        rec = torch.zeros((codes.shape[0], rb), dtype=torch.uint8, device=codes.device)
        rec[:, :m] = codes
        rec[:, off:off + 4] = scales.contiguous().view(torch.uint8).view(-1, 4)
        return rec, off

    def reconstruct_records_device(self, records, scale_offset, rows, out=None, stream=None, check=True):
        """reconstruct_rows_device over interleaved records (see interleave_records): same results, one 128-byte
        line per lookup instead of two (pqhip_reconstruct_rows_records_f32_dev)."""
        import torch
        assert records.is_cuda and records.dtype == torch.uint8 and records.dim() == 2 and records.is_contiguous()
        assert rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()
        n = rows.shape[0]
        out, o_rs = self._reconstructions(out, n, records.device)
        cb, slot, sp = _marshal.launch(self, records, stream)
        _marshal.run("pqhip_reconstruct_rows_records_f32_dev", cb, slot, records.data_ptr(), 1, records.shape[0],
                     records.shape[1], scale_offset, rows.data_ptr(), n, out.data_ptr(), o_rs, sp,
                     panics=_marshal.RANGE_PANIC)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    # ---- "next" row: asymmetric distance computation over resident codes -----
    def _adc_tables(self, name, queries, stream):
        """Both table builders."""
        import torch
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.dim() in (1, 2)
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        if q2.shape[1] != self.reconstructed_len():
            raise PanicError("Quantizer and vector length mismatch")
        q2 = _marshal.unit_columns(q2)
        nq = q2.shape[0]
        out = torch.empty((nq, self.quantized_len(), self.n_quantizer_centroids()), dtype=torch.float32,
                          device=queries.device)
        cb, slot, sp = _marshal.launch(self, queries, stream)
        _marshal.run(name, cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, q2.shape[1]), out.data_ptr(), sp)
        return out[0] if single else out

    def adc_tables_device(self, queries, stream=None):
        """queries: CUDA float32 [d] or [nq, d] -> tables [M, K] or [nq, M, K] with
        tables[q, m, j] = `y_q[m].squared_euclidean_distance(quantizers[m])[j]` (linalg.rs:118-148;
        y = query.dot(projection) first for OPQ, pq.rs:293)."""
        return self._adc_tables("pqhip_adc_tables_f32_dev", queries, stream)

    def adc_scan_device(self, codes, tables, out=None, stream=None, check=False):
        """codes: CUDA uint8 (or int32 when K > 256) [n, M]; tables: [M, K] or [nq, M, K] from
        adc_tables_device -> distances [n] or [nq, n]: out[q, i] = sum_m tables[q, m, codes[i, m]]
        (sequential f32 sum over m)."""
        import torch
        assert codes.is_cuda and codes.dtype in (torch.uint8, torch.int32) and codes.dim() == 2
        assert tables.is_cuda and tables.dtype == torch.float32 and tables.is_contiguous()
        M, K = self.quantized_len(), self.n_quantizer_centroids()
        W = _marshal.code_width(codes, M)
        single, nq = _marshal.tables_arg(tables, M, K)
        codes, n, c_rs = _marshal.codes_arg(codes, W)
        if out is None:
            out = torch.empty((n,) if single else (nq, n), dtype=torch.float32, device=codes.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == nq * n
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run("pqhip_adc_scan_f32_dev", cb, slot, tables.data_ptr(), nq, codes.data_ptr(), codes.element_size(), n,
                     c_rs, out.data_ptr(), n, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    # ---- 4-bit packed codes: two codes per byte for K <= 16 ----------------------------------------------------------
    def _packed4_served(self):
        if self.n_quantizer_centroids() > 16:
            raise PanicError("4-bit packed codes need a quantizer of at most 16 centroids")

    def pack_codes4_device(self, codes, out=None, stream=None, check=False):
        """codes: CUDA uint8 or int32 [n, M] of a quantizer with K <= 16 -> 4-bit packed rows, CUDA uint8
        [n, ceil(M / 2)]: code m in byte m >> 1, even m in the low nibble, the pad nibble of an odd M written as 0
        (pqhip_pack_codes4_dev).  A code >= K packs as 0 and raises the range flag (check=True: PanicError)."""
        import torch
        self._packed4_served()
        assert codes.is_cuda and codes.dtype in (torch.uint8, torch.int32) and codes.dim() == 2
        M = self.quantized_len()
        PB = (M + 1) // 2
        codes, n, c_rs = _marshal.codes_arg(codes, _marshal.code_width(codes, M))
        if out is None:
            out = torch.empty((n, PB), dtype=torch.uint8, device=codes.device)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, PB) and (PB == 1 or out.stride(1) == 1)
        if n == 0:
            return out
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run("pqhip_pack_codes4_dev", cb, slot, codes.data_ptr(), codes.element_size(), n, c_rs, out.data_ptr(),
                     row_stride(out, n, PB), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    def unpack_codes4_device(self, packed, rows=None, out=None, stream=None, check=False):
        """packed: CUDA uint8 [n, ceil(M / 2)] -> the codes, CUDA uint8 [n, M]; rows: CUDA int64 [r] -> the codes of those
        rows, [r, M] (pqhip_unpack_codes4_dev).  Nibbles come back as they are.  A row id outside [0, n) gives a zero row
        and raises the range flag (check=True: PanicError)."""
        import torch
        self._packed4_served()
        assert packed.is_cuda and packed.dim() == 2
        M = self.quantized_len()
        PB = _marshal.code_width(packed, M, True)
        packed = _marshal.unit_columns(packed)
        n = packed.shape[0]
        n_out = n
        if rows is not None:
            assert rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 1 and rows.device == packed.device
            rows = rows.contiguous()
            n_out = rows.shape[0]
        if out is None:
            out = torch.empty((n_out, M), dtype=torch.uint8, device=packed.device)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n_out, M) and (M == 1 or out.stride(1) == 1)
        if n_out == 0:
            return out
        # with n = 0 every row id is out of range and no packed byte is read
        src = _marshal.stand_in(packed, n, packed.device, PB)
        cb, slot, sp = _marshal.launch(self, packed, stream)
        _marshal.run("pqhip_unpack_codes4_dev", cb, slot, src.data_ptr(), n, row_stride(src, n, PB), ptr_or_none(rows),
                     n_out, out.data_ptr(), row_stride(out, n_out, M), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    # ---- row masks: restrict a search to an allowed set of rows ------------------------------------------------------
    def pack_row_mask_device(self, allow, perm=None, stream=None, check=False):
        """allow: CUDA bool or uint8 [n_src], nonzero = the row may be returned; perm: None or CUDA int64 [n] -> the mask
        words of the searches' `allow=`, CUDA int32 [ceil(n / 32)]: bit p & 31 of word p >> 5 is allow[perm[p]] (allow[p]
        without perm, n = n_src), the tail bits of the last word 0 (pqhip_pack_row_mask_dev).  A perm entry outside
        [0, n_src) gives bit 0 and raises the range flag (check=True: PanicError)."""
        import torch
        assert allow.is_cuda and allow.dtype in (torch.bool, torch.uint8) and allow.dim() == 1
        ab = allow.contiguous()
        if ab.dtype == torch.bool:
            ab = ab.view(torch.uint8)
        n_src = ab.shape[0]
        n = n_src
        if perm is not None:
            assert perm.is_cuda and perm.dtype == torch.int64 and perm.dim() == 1 and perm.device == allow.device
            perm = perm.contiguous()
            n = perm.shape[0]
        words = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=allow.device)
        if n == 0:
            return words
        ab = _marshal.stand_in(ab, n_src, allow.device)
        cb, slot, sp = _marshal.launch(self, allow, stream)
        _marshal.run("pqhip_pack_row_mask_dev", cb, slot, ab.data_ptr(), n_src, ptr_or_none(perm), n, words.data_ptr(), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return words

    def _adc_search(self, ip, codes, tables, k, scales, stream, check, allow, packed4):
        """Both exhaustive searches; allow given: their masked forms; packed4: their forms over 4-bit packed rows (a mask
        or none)."""
        import torch
        if packed4:
            self._packed4_served()
        name = "pqhip_adc_%ssearch_%sf32_dev" % ("ip_" if ip else "",
                                                 "packed4_" if packed4 else "masked_" if allow is not None else "")
        assert codes.is_cuda and codes.dtype in (torch.uint8, torch.int32) and codes.dim() == 2
        assert tables.is_cuda and tables.dtype == torch.float32 and tables.is_contiguous()
        M, K = self.quantized_len(), self.n_quantizer_centroids()
        W = _marshal.code_width(codes, M, packed4)
        single, nq = _marshal.tables_arg(tables, M, K)
        codes, n, c_rs = _marshal.codes_arg(codes, W)
        _marshal.per_row_arg(scales, n, "scales")
        val = torch.empty((nq, k), dtype=torch.float32, device=codes.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        head = _marshal.search_head(cb, slot, tables, nq, codes, n, c_rs, packed4, _marshal.mask_arg(allow, codes, packed4),
                                    last=(ptr_or_none(scales),) if ip else ())
        _marshal.run(name, *head, k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    def adc_search_device(self, codes, tables, k, stream=None, check=False, allow=None, packed4=False):
        """The k nearest rows per query without the distance matrix: codes and tables as for adc_scan_device ->
        (dist, idx), CUDA float32 and int64 [nq, k] ([k] for 2-D tables).  dist[q, j] is the scan's distance of row
        idx[q, j]; rows are ordered by distance -- NaN above +Inf -- then by index (pqhip_adc_search_f32_dev).  Past
        the last row: index -1, distance +Inf.  allow: None or the words of pack_row_mask_device -- the search then
        ranks the allowed rows only, as if the others were not in the matrix (pqhip_adc_search_masked_f32_dev).
        packed4=True: codes are 4-bit packed rows, CUDA uint8 [n, ceil(M / 2)] (pack_codes4_device; K <= 16), and the
        result is bit for bit that of the unpacked codes (pqhip_adc_search_packed4_f32_dev)."""
        return self._adc_search(False, codes, tables, k, None, stream, check, allow, packed4)

    # ---- ADC similarity search: inner products over resident codes --------------------------------------------------
    def adc_ip_tables_device(self, queries, stream=None):
        """queries: CUDA float32 [d] or [nq, d] -> inner-product tables [M, K] or [nq, M, K]:
        tables[q, m, j] = unrolled_dot(quantizers[m, j], y_q[m]), the dp term of adc_tables_device (y = query.dot(projection)
        first for OPQ).  sum_m tables[q, m, codes[i, m]] is <query_q, reconstruct(codes[i])> (pqhip_adc_ip_tables_f32_dev)."""
        return self._adc_tables("pqhip_adc_ip_tables_f32_dev", queries, stream)

    def adc_ip_search_device(self, codes, tables, k, scales=None, stream=None, check=False, allow=None, packed4=False):
        """The k most similar rows per query: codes as for adc_scan_device, tables from adc_ip_tables_device, scales None
        or CUDA float32 [n] -> (score, idx), CUDA float32 and int64 [nq, k] ([k] for 2-D tables).  score[q, j] =
        fl(scan[q, i] * scales[i]) of row i = idx[q, j] (the scan's sum alone without scales); rows are ordered by
        descending score -- NaN after -Inf -- then by index (pqhip_adc_ip_search_f32_dev).  A zero score comes back as
        +0, a NaN as the canonical NaN.  Past the last row: index -1, score -Inf.  allow: as for adc_search_device
        (pqhip_adc_ip_search_masked_f32_dev).  packed4: as for adc_search_device (pqhip_adc_ip_search_packed4_f32_dev)."""
        return self._adc_search(True, codes, tables, k, scales, stream, check, allow, packed4)

    # ---- ADC search over a partitioned code matrix: exact top-k within the probed lists -----------------------------
    def _adc_search_lists(self, ip, codes, tables, list_off, probes, k, scales, stream, check, probe_bias=None,
                          row_terms=None, allow=None, packed4=False):
        """All four list searches; probe_bias given: the residual ones (row_terms then required for the distance);
        allow given: their masked forms (the words of pack_row_mask_device, in position order); packed4: their forms
        over 4-bit packed rows (a mask or none)."""
        import torch
        if packed4:
            self._packed4_served()
        residual = probe_bias is not None
        name = "pqhip_adc_%ssearch_lists_%s%sf32_dev" % ("ip_" if ip else "", "residual_" if residual else "",
                                                        "packed4_" if packed4 else "masked_" if allow is not None else "")
        assert codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2
        assert tables.is_cuda and tables.dtype == torch.float32 and tables.is_contiguous()
        _marshal.assert_lists(list_off, probes)
        M, K = self.quantized_len(), self.n_quantizer_centroids()
        W = _marshal.code_width(codes, M, packed4)
        single, nq = _marshal.tables_arg(tables, M, K)
        pr, n_probe, p_rs = _marshal.probes_arg(probes, list_off, nq)
        codes, n, c_rs = _marshal.codes_arg(codes, W)
        _marshal.per_row_arg(scales, n, "scales")
        bias = ()
        if residual:
            bias = _marshal.bias_arg(probe_bias, nq, n_probe)
            if not ip:
                _marshal.per_row_arg(row_terms, n, "row_terms")
        val = torch.empty((nq, k), dtype=torch.float32, device=codes.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        mask = _marshal.mask_arg(allow, codes, packed4)
        last = (ptr_or_none(scales),) if ip else ()
        if residual and not ip:
            rt = _marshal.stand_in(row_terms, n, codes.device)      # the C call wants an address even without a row to read
            last = (rt.data_ptr(),)
        _marshal.run(name, *_marshal.search_head(cb, slot, tables, nq, codes, n, c_rs, packed4, mask,
                                                 (list_off, pr, n_probe, p_rs), bias, last),
                     k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    def adc_search_lists_device(self, codes, tables, list_off, probes, k, stream=None, check=False, allow=None,
                                packed4=False):
        """adc_search_device restricted, per query, to the rows of the probed lists: list l is rows
        [list_off[l], list_off[l + 1]) of codes (CUDA uint8 [n, M]); list_off CUDA int64 [n_lists + 1]; probes CUDA int64
        [nq, n_probe] ([n_probe] for 2-D tables) of list ids, -1 = padding -> (dist, idx) [nq, k] ([k]).  The result is
        what adc_search_device returns on codes with every row outside the probed lists removed, idx being positions in
        codes (pqhip_adc_search_lists_f32_dev).  Past the last probed row: index -1, distance +Inf.  check=True also
        reports a list id or an offset out of range.  allow: None or the words of pack_row_mask_device in position order
        (row order of codes): only allowed rows of the probed lists are ranked (pqhip_adc_search_lists_masked_f32_dev).
        packed4=True: codes are 4-bit packed rows, CUDA uint8 [n, ceil(M / 2)]; the result is bit for bit that of the
        unpacked codes (pqhip_adc_search_lists_packed4_f32_dev)."""
        return self._adc_search_lists(False, codes, tables, list_off, probes, k, None, stream, check, allow=allow,
                                      packed4=packed4)

    def adc_ip_search_lists_device(self, codes, tables, list_off, probes, k, scales=None, stream=None, check=False,
                                   allow=None, packed4=False):
        """adc_ip_search_device restricted, per query, to the rows of the probed lists (arguments as for
        adc_search_lists_device, tables from adc_ip_tables_device, scales None or CUDA float32 [n]) -> (score, idx).
        Past the last probed row: index -1, score -Inf (pqhip_adc_ip_search_lists_f32_dev).  allow, packed4: as for
        adc_search_lists_device."""
        return self._adc_search_lists(True, codes, tables, list_off, probes, k, scales, stream, check, allow=allow,
                                      packed4=packed4)

    # ---- the same over residual codes (IVFADC with residual encoding): one table per query, a bias per probe ---------
    def adc_search_lists_residual_device(self, codes, ip_tables, list_off, probes, probe_bias, row_terms, k, stream=None,
                                         check=False, allow=None, packed4=False):
        """adc_search_lists_device over residual codes: self is the quantizer of the residuals x - c_list(x), ip_tables
        are its INNER-PRODUCT tables (adc_ip_tables_device), probe_bias CUDA float32 [nq, n_probe] ([n_probe] for one
        query) holds |q - c_l|^2 of the list in each probe slot and row_terms CUDA float32 [n] holds |r^|^2 + 2 <c_l, r^>
        of each row -> (dist, idx) with dist = fl(fl(bias + term) - fl(s + s)), s the scan's row sum, ordered by
        (key(dist), position) (pqhip_adc_search_lists_residual_f32_dev).  The bias of a skipped probe is never used.
        allow, packed4: as for adc_search_lists_device; the row term of a disallowed row is never read."""
        if probe_bias is None or row_terms is None:
            raise PanicError("the residual distance search needs a probe bias and the row terms")
        return self._adc_search_lists(False, codes, ip_tables, list_off, probes, k, None, stream, check,
                                      probe_bias=probe_bias, row_terms=row_terms, allow=allow, packed4=packed4)

    def adc_ip_search_lists_residual_device(self, codes, ip_tables, list_off, probes, probe_bias, k, scales=None,
                                            stream=None, check=False, allow=None, packed4=False):
        """adc_ip_search_lists_device over residual codes: probe_bias holds <q, c_l> of the list in each probe slot ->
        (score, idx) with score = fl(fl(bias + s) * scale), fl(bias + s) without scales, ordered by (key(-score),
        position) (pqhip_adc_ip_search_lists_residual_f32_dev).  allow, packed4: as for adc_search_lists_device."""
        if probe_bias is None:
            raise PanicError("the residual similarity search needs a probe bias")
        return self._adc_search_lists(True, codes, ip_tables, list_off, probes, k, scales, stream, check,
                                      probe_bias=probe_bias, allow=allow, packed4=packed4)

    # ---- ADC search among given rows: exact top-k over per-query candidate id lists ------------------------------------
    def _adc_among(self, ip, codes, tables, ids, k, lims, row_list, list_bias, extra, what, stream, check):
        """Both candidate searches; row_list and list_bias given: the residual forms.  extra: the scales (ip) or the row
        terms, named `what`."""
        import torch
        name = "pqhip_adc_%samong_f32_dev" % ("ip_" if ip else "")
        M, K = self.quantized_len(), self.n_quantizer_centroids()

        def vector(t, dtype, text):
            if not (hasattr(t, "is_cuda") and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()):
                raise PanicError(text)

        if not (hasattr(codes, "is_cuda") and codes.dtype == torch.uint8 and codes.dim() == 2):
            raise PanicError("codes must be a uint8 [n, n_subquantizers] tensor (4-byte and packed codes are not served)")
        if not (hasattr(tables, "is_cuda") and tables.dtype == torch.float32 and tables.dim() in (2, 3) and tables.is_contiguous()):
            raise PanicError("lookup tables must be a contiguous float32 tensor")
        W = _marshal.code_width(codes, M)
        single, nq = _marshal.tables_arg(tables, M, K)
        vector(ids, torch.int64, "candidate ids must be one contiguous int64 vector, shared or cut per query by lims")
        if lims is not None:
            vector(lims, torch.int64, "lims must be a contiguous int64 vector")
            if lims.shape[0] != nq + 1:
                raise PanicError("lims must hold one offset per query and the end (%d)" % (nq + 1))
        if not isinstance(k, int) or k < 1:
            raise PanicError("k must be a positive integer")
        n = codes.shape[0]
        if extra is not None:
            vector(extra, torch.float32, "%s must be a contiguous float32 vector" % what)
            if extra.shape[0] != n:
                raise PanicError("%s must hold one value per code row" % what)
        if (row_list is None) != (list_bias is None):
            raise PanicError("the residual candidate search needs the list of every row and a bias per list")
        residual = row_list is not None
        n_lists, lb, b_rs = 0, None, 0
        if residual:
            vector(row_list, torch.int64, "row_list must be a contiguous int64 vector")
            if row_list.shape[0] != n:
                raise PanicError("row_list must hold one list id per code row")
            if not (hasattr(list_bias, "is_cuda") and list_bias.dtype == torch.float32 and list_bias.dim() in (1, 2)):
                raise PanicError("list_bias must be a float32 [nq, n_lists] tensor")
            lb = list_bias[None] if list_bias.dim() == 1 else list_bias
            if lb.shape[0] != nq:
                raise PanicError("one row of list biases per query expected")
            if not ip and extra is None:
                raise PanicError("the residual distance search needs the row terms")
        given = [t for t in (codes, tables, ids, lims, extra, row_list, list_bias) if t is not None]
        if not all(t.is_cuda and t.device == codes.device for t in given):
            raise PanicError("the candidate search expects CUDA tensors on one device")
        codes, n, c_rs = _marshal.codes_arg(codes, W)
        _marshal.per_row_arg(extra, n, what)
        if residual:
            n_lists = lb.shape[1]
            lb = _marshal.stand_in(_marshal.unit_columns(lb), n_lists, codes.device, 1)
            b_rs = _marshal.row_stride(lb, nq, max(n_lists, 1))
            row_list = _marshal.stand_in(row_list, n, codes.device)      # the C call tells the residual form by the address
            if not ip:
                extra = _marshal.stand_in(extra, n, codes.device)
        n_ids = ids.shape[0]
        val = torch.empty((nq, k), dtype=torch.float32, device=codes.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run(name, cb, slot, tables.data_ptr(), nq, codes.data_ptr(), codes.element_size(), n, c_rs, ptr_or_none(lims),
                     ptr_or_none(ids, n_ids), n_ids, ptr_or_none(row_list), n_lists, ptr_or_none(lb), b_rs,
                     ptr_or_none(extra, extra is not None and extra.shape[0]) if (ip or residual) else None,
                     k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    def adc_among_device(self, codes, tables, ids, k, lims=None, row_list=None, list_bias=None, row_terms=None,
                         stream=None, check=False):
        """adc_search_device among given rows: ids CUDA int64 [n_ids] names the candidates -- of every query (lims None),
        or ids[lims[q] : lims[q + 1]] of query q (lims CUDA int64 [nq + 1], as a range search returns it) -> (dist, idx)
        [nq, k] ([k] for 2-D tables), the first k candidates by (distance, row).  -1 is padding; any other id outside
        [0, n) is skipped and, like a bad lims, raises the range flag (check=True); an id named twice may come back
        twice.  A row that is not named is not read.  For distinct ids the result is adc_search_device's with the mask
        of the candidates (pqhip_adc_among_f32_dev).  Residual codes: row_list CUDA int64 [n] (the list of every row),
        list_bias CUDA float32 [nq, n_lists] (|q - c_l|^2 per list), row_terms CUDA float32 [n] and INNER-PRODUCT tables,
        dist = fl(fl(bias + term) - fl(s + s)) as adc_search_lists_residual_device forms it."""
        return self._adc_among(False, codes, tables, ids, k, lims, row_list, list_bias, row_terms, "row_terms", stream,
                               check)

    def adc_ip_among_device(self, codes, tables, ids, k, lims=None, row_list=None, list_bias=None, scales=None,
                            stream=None, check=False):
        """adc_ip_search_device among given rows (arguments as for adc_among_device, tables from adc_ip_tables_device,
        scales None or CUDA float32 [n]) -> (score, idx), the first k candidates by (descending score, row).  Residual
        codes: list_bias holds <q, c_l> per list, score = fl(fl(bias + s) * scale) (pqhip_adc_ip_among_f32_dev)."""
        return self._adc_among(True, codes, tables, ids, k, lims, row_list, list_bias, scales, "scales", stream, check)

    # ---- ADC range search: every row within a radius / at or above a similarity, as CSR ------------------------------
    def _adc_range(self, ip, codes, tables, threshold, scales, stream, check, allow, capacity, lists=None, probe_bias=None,
                   row_terms=None):
        """All six range searches -> (lims, val, idx).  lists: (list_off, probes) for the list forms; probe_bias given:
        the residual ones (row_terms then required for the distance).  The capacity protocol of include/pqhip.h: one call
        with `capacity` entries (default 1 << 20), one read of lims[-1] -- the only synchronisation -- and, if the result
        is larger, one more call with exactly that many entries."""
        import torch
        residual = probe_bias is not None
        name = "pqhip_adc_%srange_%s%sf32_dev" % ("ip_" if ip else "", "lists_" if lists is not None else "",
                                                 "residual_" if residual else "")
        assert codes.is_cuda and codes.dtype in (torch.uint8, torch.int32) and codes.dim() == 2
        assert tables.is_cuda and tables.dtype == torch.float32 and tables.is_contiguous()
        M, K = self.quantized_len(), self.n_quantizer_centroids()
        W = _marshal.code_width(codes, M)
        single, nq = _marshal.tables_arg(tables, M, K)
        codes, n, c_rs = _marshal.codes_arg(codes, W)
        dev = codes.device
        thr = _marshal.threshold_arg(threshold, nq, dev)
        _marshal.per_row_arg(scales, n, "scales")
        mask = _marshal.mask_arg(allow, codes, True)
        bias = ()
        last = (ptr_or_none(scales),) if ip else ()
        if lists is not None:
            list_off, probes = lists
            _marshal.assert_lists(list_off, probes)
            pr, n_probe, p_rs = _marshal.probes_arg(probes, list_off, nq)
            lists = (list_off, pr, n_probe, p_rs)
            if residual:
                bias = _marshal.bias_arg(probe_bias, nq, n_probe)
                if not ip:
                    _marshal.per_row_arg(row_terms, n, "row_terms")
                    rt = _marshal.stand_in(row_terms, n, dev)       # the C call wants an address even without a row to read
                    last = (rt.data_ptr(),)
        own_stream = stream is None
        cb, slot, sp = _marshal.launch(self, codes, stream)
        head = _marshal.search_head(cb, slot, tables, nq, codes, n, c_rs, False, mask, lists or (), bias, last)
        lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        cap = (1 << 20) if capacity is None else int(capacity)
        if cap < 0:
            raise PanicError("capacity must not be negative")
        while True:
            val = torch.empty(cap, dtype=torch.float32, device=dev)
            idx = torch.empty(cap, dtype=torch.int64, device=dev)
            _marshal.run(name, *head, thr.data_ptr(), lims.data_ptr(), ptr_or_none(val, cap), ptr_or_none(idx, cap), cap, sp)
            if not own_stream:
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
            total = int(lims[-1])
            if total <= cap:
                break
            cap = total             # the second call always suffices
        if check:
            _marshal.check_range(cb, slot, sp)
        return lims, val[:total], idx[:total]

    def adc_range_device(self, codes, tables, threshold, stream=None, check=False, allow=None, capacity=None):
        """EVERY row whose asymmetric squared distance is <= threshold, without the distance matrix: codes (CUDA uint8
        [n, M]) and tables as for adc_search_device, threshold a scalar or one value per query (float, numpy or tensor)
        -> (lims, dist, idx): CSR, lims CUDA int64 [nq + 1] ([2] for 2-D tables), the rows of query q at
        dist[lims[q]:lims[q + 1]] / idx[..] in ascending row index, dist the scan's value bit for bit
        (pqhip_adc_range_f32_dev).  A NaN distance never qualifies; threshold +Inf returns every non-NaN row.  capacity:
        entries allocated for the first call (default 1 << 20); if the result is larger the call is repeated once with
        exactly its size -- lims[-1] is read in between, the one synchronisation.  allow: None or the words of
        pack_row_mask_device; a disallowed row is not read."""
        return self._adc_range(False, codes, tables, threshold, None, stream, check, allow, capacity)

    def adc_ip_range_device(self, codes, tables, threshold, scales=None, stream=None, check=False, allow=None,
                            capacity=None):
        """Every row whose score fl(scan * scales) (the scan's sum alone without scales) is >= threshold: tables from
        adc_ip_tables_device, the rest as for adc_range_device -> (lims, score, idx), rows in ascending row index, a zero
        score with its sign (pqhip_adc_ip_range_f32_dev).  Threshold -Inf returns every non-NaN row."""
        return self._adc_range(True, codes, tables, threshold, scales, stream, check, allow, capacity)

    def adc_range_lists_device(self, codes, tables, list_off, probes, threshold, stream=None, check=False, allow=None,
                               capacity=None):
        """adc_range_device restricted, per query, to the rows of the probed lists (list_off, probes as for
        adc_search_lists_device) -> (lims, dist, idx); idx are positions in codes and the rows of a query come in the order
        of the concatenation of its probed lists: probe slot first, then position (pqhip_adc_range_lists_f32_dev)."""
        return self._adc_range(False, codes, tables, threshold, None, stream, check, allow, capacity, lists=(list_off, probes))

    def adc_ip_range_lists_device(self, codes, tables, list_off, probes, threshold, scales=None, stream=None, check=False,
                                  allow=None, capacity=None):
        """adc_ip_range_device restricted to the rows of the probed lists -> (lims, score, idx), order as for
        adc_range_lists_device (pqhip_adc_ip_range_lists_f32_dev)."""
        return self._adc_range(True, codes, tables, threshold, scales, stream, check, allow, capacity, lists=(list_off, probes))

    def adc_range_lists_residual_device(self, codes, ip_tables, list_off, probes, probe_bias, row_terms, threshold,
                                        stream=None, check=False, allow=None, capacity=None):
        """adc_range_lists_device over residual codes: dist = fl(fl(bias + term) - fl(s + s)) <= threshold, the arguments
        of adc_search_lists_residual_device with the threshold in the place of k (pqhip_adc_range_lists_residual_f32_dev)."""
        if probe_bias is None or row_terms is None:
            raise PanicError("the residual distance search needs a probe bias and the row terms")
        return self._adc_range(False, codes, ip_tables, threshold, None, stream, check, allow, capacity,
                               lists=(list_off, probes), probe_bias=probe_bias, row_terms=row_terms)

    def adc_ip_range_lists_residual_device(self, codes, ip_tables, list_off, probes, probe_bias, threshold, scales=None,
                                           stream=None, check=False, allow=None, capacity=None):
        """adc_ip_range_lists_device over residual codes: score = fl(fl(bias + s) * scale) >= threshold (fl(bias + s)
        without scales), the arguments of adc_ip_search_lists_residual_device with the threshold in the place of k
        (pqhip_adc_ip_range_lists_residual_f32_dev)."""
        if probe_bias is None:
            raise PanicError("the residual similarity search needs a probe bias")
        return self._adc_range(True, codes, ip_tables, threshold, scales, stream, check, allow, capacity,
                               lists=(list_off, probes), probe_bias=probe_bias)

    # ---- exact re-ranking of search candidates against resident vectors ("IVFADC+R") ---------------------------------
    def rerank_device(self, queries, vectors, candidates, k, ip=False, stream=None, check=False):
        """The k best of each query's candidates by their exact distance to the stored vectors: queries CUDA float32
        [d] or [nq, d]; vectors CUDA float32 or float16 [N, d] (f16 elements are converted exactly); candidates CUDA
        int64 [n_cand] or [nq, n_cand] of row numbers, -1 = padding, 1 <= n_cand <= 1024 -> (value, idx), CUDA float32
        and int64 [nq, k] ([k] for one query).  value is the squared L2 distance, or with ip=True the inner product, in
        the fixed f32 summation order of pqhip_rerank_f32_dev; rows are ordered by ascending distance (descending
        product), NaN last, ties to the smaller row number.  Past the last candidate: index -1 and +Inf (ip: -Inf).
        Row strides are respected (unit column stride is made by a copy if needed).  The quantizer of self is not
        used: d is the width of the vectors.  check=True synchronises and raises on a candidate outside [0, N) other
        than -1; with check=False it is skipped and stays pending on the stream's flag."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors"), (candidates, "candidates")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        if candidates.dtype != torch.int64 or candidates.dim() != queries.dim():
            raise PanicError("candidates must be int64 with one row per query")
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        c2 = candidates[None] if single else candidates
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if c2.shape[0] != nq:
            raise PanicError("candidates must be int64 with one row per query")
        n_cand = c2.shape[1]
        if not 1 <= n_cand <= 1024:
            raise PanicError("between 1 and 1024 candidates per query expected, got %d" % n_cand)
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        if not (queries.is_cuda and vectors.is_cuda and candidates.is_cuda):
            raise PanicError("queries, vectors and candidates must be CUDA tensors")
        if not (queries.device == vectors.device == candidates.device):
            raise PanicError("queries, vectors and candidates must live on one device")
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if c2.stride(1) != 1:
            c2 = c2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        val = torch.empty((nq, k), dtype=torch.float32, device=vectors.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=vectors.device)
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        _marshal.run("pqhip_rerank_f32_dev", cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d),
                     ptr_or_none(vectors, N), vectors.element_size(), N, d, row_stride(vectors, N, d),
                     c2.data_ptr(), n_cand, row_stride(c2, nq, n_cand), 1 if ip else 0, k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    # ---- exact search over resident vectors: the exhaustive top-k by true distance ------------------------------------
    def flat_search_device(self, queries, vectors, k, ip=False, allow=None, stream=None, check=False):
        """The k best of ALL rows of `vectors` per query by their exact value: queries CUDA float32 [d] or [nq, d];
        vectors CUDA float32 or float16 [N, d] (f16 elements are converted exactly); allow None or the mask words of
        pack_row_mask_device, CUDA int32 [ceil(N / 32)] -- then the allowed rows only are ranked, as if the others were
        not in the matrix -> (value, idx), CUDA float32 and int64 [nq, k] ([k] for one query).  Value, order and padding
        are those of rerank_device over the candidate list 0 .. N - 1 (pqhip_flat_search_f32_dev).  Row strides are
        respected (unit column stride is made by a copy if needed).  The quantizer of self is not used: d is the width
        of the vectors.  There is no range flag to raise; check=True only synchronises."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if d > 16384:
            raise PanicError("vectors of at most 16384 elements are searched, got %d" % d)
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        allow = _marshal.vector_mask_words(allow, N)
        tensors = (queries, vectors) if allow is None else (queries, vectors, allow)
        if not all(t.is_cuda for t in tensors):
            raise PanicError("queries, vectors and allow must be CUDA tensors")
        if any(t.device != vectors.device for t in tensors):
            raise PanicError("queries, vectors and allow must live on one device")
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        if allow is not None:
            allow = _marshal.stand_in(allow, allow.shape[0], vectors.device)   # a mask stays a mask (N = 0 reads no word)
        val = torch.empty((nq, k), dtype=torch.float32, device=vectors.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=vectors.device)
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        _marshal.run("pqhip_flat_search_f32_dev", cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d),
                     ptr_or_none(vectors, N), vectors.element_size(), N, d, row_stride(vectors, N, d),
                     None if allow is None else allow.data_ptr(), 1 if ip else 0, k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    # ---- exact search in probed lists: the flat search restricted, per query, to the lists it probes --------------------
    def flat_search_lists_device(self, queries, vectors, list_off, probes, k, ip=False, allow=None, stream=None, check=False):
        """flat_search_device restricted, per query, to the rows of the probed lists (IVF-Flat): vectors CUDA float32 or
        float16 [N, d] in LIST ORDER, list l being rows [list_off[l], list_off[l + 1]); list_off CUDA int64 [n_lists + 1];
        probes CUDA int64 [nq, n_probe] ([n_probe] for one query) of list ids, -1 = padding; allow None or the mask words of
        pack_row_mask_device in position order, CUDA int32 [ceil(N / 32)] -> (value, idx), CUDA float32 and int64 [nq, k]
        ([k] for one query), idx being positions in vectors; past the last probed (allowed) row: index -1 and +Inf (ip:
        -Inf).  Query by query the result is flat_search_device with the mask of those rows, bit for bit; with every list
        probed it is the unmasked call (pqhip_flat_search_lists_f32_dev).  Row strides are respected (unit column
        stride is made by a copy if needed).  The quantizer of self is not used.  check=True synchronises and reports a
        list id or an offset out of range (they are skipped resp. clamped either way)."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if d > 16384:
            raise PanicError("vectors of at most 16384 elements are searched, got %d" % d)
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        if N > (1 << 32) - 2:
            raise PanicError("at most 2^32 - 2 rows are searched in lists")
        pr, n_lists, n_probe, p_rs = _marshal.vector_lists_arg(list_off, probes, nq)
        allow = _marshal.vector_mask_words(allow, N)
        tensors = (queries, vectors, list_off, probes) + (() if allow is None else (allow,))
        if not all(t.is_cuda for t in tensors):
            raise PanicError("queries, vectors, list_off, probes and allow must be CUDA tensors")
        if any(t.device != vectors.device for t in tensors):
            raise PanicError("queries, vectors, list_off, probes and allow must live on one device")
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        if allow is not None:
            allow = _marshal.stand_in(allow, allow.shape[0], vectors.device)   # a mask stays a mask (N = 0 reads no word)
        val = torch.empty((nq, k), dtype=torch.float32, device=vectors.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=vectors.device)
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        _marshal.run("pqhip_flat_search_lists_f32_dev", cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d),
                     ptr_or_none(vectors, N), vectors.element_size(), N, d, row_stride(vectors, N, d),
                     list_off.data_ptr(), n_lists, pr.data_ptr(), n_probe, p_rs,
                     None if allow is None else allow.data_ptr(), 1 if ip else 0, k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    # ---- exact range search over resident vectors: every row within a radius, by true distance ---------------------------
    def _flat_range(self, queries, vectors, threshold, ip, allow, capacity, stream, check, lists=None):
        """Both exact range searches -> (lims, val, idx): queries, vectors and mask marshalled as for flat_search_device,
        the threshold and the capacity protocol as for _adc_range (one call with `capacity` entries, default 1 << 20, one
        read of lims[-1] -- the only synchronisation -- and, if the result is larger, one more call of exactly its
        size).  lists: (list_off, probes) for the list form."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        q2 = queries[None] if queries.dim() == 1 else queries
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if d > 16384:
            raise PanicError("vectors of at most 16384 elements are searched, got %d" % d)
        tensors = (queries, vectors)
        names = "queries, vectors"
        if lists is not None:
            if N > (1 << 32) - 2:
                raise PanicError("at most 2^32 - 2 rows are searched in lists")
            list_off, probes = lists
            pr, n_lists, n_probe, p_rs = _marshal.vector_lists_arg(list_off, probes, nq)
            tensors += (list_off, probes)
            names += ", list_off, probes"
        allow = _marshal.vector_mask_words(allow, N)
        if allow is not None:
            tensors += (allow,)
        if not all(t.is_cuda for t in tensors):
            raise PanicError("%s and allow must be CUDA tensors" % names)
        if any(t.device != vectors.device for t in tensors):
            raise PanicError("%s and allow must live on one device" % names)
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        if allow is not None:
            allow = _marshal.stand_in(allow, allow.shape[0], vectors.device)   # a mask stays a mask (N = 0 reads no word)
        dev = vectors.device
        thr = _marshal.threshold_arg(threshold, nq, dev)
        cap = (1 << 20) if capacity is None else int(capacity)
        if cap < 0:
            raise PanicError("capacity must not be negative")
        own_stream = stream is None
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        head = (cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d), ptr_or_none(vectors, N), vectors.element_size(), N, d,
                row_stride(vectors, N, d), None if allow is None else allow.data_ptr())
        name = "pqhip_flat_range_f32_dev"
        if lists is not None:
            head += (list_off.data_ptr(), n_lists, pr.data_ptr(), n_probe, p_rs)
            name = "pqhip_flat_range_lists_f32_dev"
        lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        while True:
            val = torch.empty(cap, dtype=torch.float32, device=dev)
            idx = torch.empty(cap, dtype=torch.int64, device=dev)
            _marshal.run(name, *head, 1 if ip else 0, thr.data_ptr(), lims.data_ptr(), ptr_or_none(val, cap), ptr_or_none(idx, cap),
                         cap, sp)
            if not own_stream:
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
            total = int(lims[-1])
            if total <= cap:
                break
            cap = total             # the second call always suffices
        if check:
            _marshal.check_range(cb, slot, sp)
        return lims, val[:total], idx[:total]

    def flat_range_device(self, queries, vectors, threshold, ip=False, allow=None, capacity=None, stream=None, check=False):
        """EVERY row of `vectors` whose exact squared distance to the query is <= threshold (ip=True: whose inner product
        is >= threshold): queries, vectors and allow as for flat_search_device, threshold a scalar or one value per query
        (float, numpy or tensor) -> (lims, val, idx): CSR, lims CUDA int64 [nq + 1] ([2] for one query), the rows of query
        q at val[lims[q]:lims[q + 1]] / idx[..] in ascending row index, val the value flat_search_device returns for the
        row, bit for bit (pqhip_flat_range_f32_dev).  A NaN value never qualifies; threshold +Inf (ip: -Inf) returns
        every non-NaN row.  capacity: entries allocated for the first call (default 1 << 20); if the result is larger
        the call is repeated once with exactly its size -- lims[-1] is read in between, the one synchronisation;
        capacity=0 counts first.  A disallowed row is not read.  There is no range flag to raise; check=True only
        synchronises."""
        return self._flat_range(queries, vectors, threshold, ip, allow, capacity, stream, check)

    def flat_range_lists_device(self, queries, vectors, list_off, probes, threshold, ip=False, allow=None, capacity=None,
                                stream=None, check=False):
        """flat_range_device restricted, per query, to the rows of the probed lists (vectors in list order, list_off,
        probes and allow in position order as for flat_search_lists_device) -> (lims, val, idx); idx are positions in
        vectors and the rows of a query come in the order of the concatenation of its probed lists: probe slot first,
        then position; a list named twice returns its rows twice (pqhip_flat_range_lists_f32_dev).  check=True
        synchronises and reports a list id or an offset out of range (they are skipped resp. clamped either way)."""
        return self._flat_range(queries, vectors, threshold, ip, allow, capacity, stream, check, lists=(list_off, probes))

    # ---- exact search among given rows: top-k and range over per-query candidate id lists, by true distance ---------------
    def _flat_among_args(self, queries, vectors, ids, lims):
        """What both exact candidate calls check and marshal: queries and vectors as for flat_search_device, ids and
        lims as for adc_among_device -> (single, q2, vectors, nq, d, N, n_ids)."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if d > 16384:
            raise PanicError("vectors of at most 16384 elements are searched, got %d" % d)
        if N > (1 << 32) - 2:
            raise PanicError("at most 2^32 - 2 rows are searched among candidates")

        def vector(t, text):
            if not (hasattr(t, "is_cuda") and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous()):
                raise PanicError(text)

        vector(ids, "candidate ids must be one contiguous int64 vector, shared or cut per query by lims")
        if lims is not None:
            vector(lims, "lims must be a contiguous int64 vector")
            if lims.shape[0] != nq + 1:
                raise PanicError("lims must hold one offset per query and the end (%d)" % (nq + 1))
        given = [t for t in (queries, vectors, ids, lims) if t is not None]
        if not all(t.is_cuda and t.device == vectors.device for t in given):
            raise PanicError("the exact candidate search expects CUDA tensors on one device")
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        return single, q2, vectors, nq, d, N, ids.shape[0]

    def flat_among_device(self, queries, vectors, ids, k, lims=None, ip=False, stream=None, check=False):
        """flat_search_device among given rows: queries CUDA float32 [d] or [nq, d]; vectors CUDA float32 or float16
        [N, d]; ids CUDA int64 [n_ids] names the candidates -- of every query (lims None), or ids[lims[q] : lims[q + 1]]
        of query q (lims CUDA int64 [nq + 1], as a range search returns it) -> (value, idx), CUDA float32 and int64
        [nq, k] ([k] for one query): the first k candidates by (exact squared distance, row), ip=True by (descending inner
        product, row); past the last candidate index -1 and +Inf (ip: -Inf).  Any number of ids per query.  -1 is
        padding; any other id outside [0, N) is skipped and, like a bad lims, raises the range flag (check=True); an id
        named twice may come back twice.  A row that is not named is not read.  For distinct ids the result is
        flat_search_device's with the mask of the candidates, bit for bit, and rerank_device's where that call takes the
        candidates (pqhip_flat_among_f32_dev).  The quantizer of self is not used."""
        import torch
        single, q2, vectors, nq, d, N, n_ids = self._flat_among_args(queries, vectors, ids, lims)
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        val = torch.empty((nq, k), dtype=torch.float32, device=vectors.device)
        idx = torch.empty((nq, k), dtype=torch.int64, device=vectors.device)
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        _marshal.run("pqhip_flat_among_f32_dev", cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d),
                     ptr_or_none(vectors, N), vectors.element_size(), N, d, row_stride(vectors, N, d),
                     ptr_or_none(lims), ptr_or_none(ids, n_ids), n_ids, 1 if ip else 0, k, val.data_ptr(), k, idx.data_ptr(), k, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (val[0], idx[0]) if single else (val, idx)

    def flat_range_among_device(self, queries, vectors, ids, threshold, lims=None, ip=False, stream=None, check=False):
        """flat_range_device among given rows (queries, vectors, ids and lims as for flat_among_device; threshold a scalar
        or one value per query) -> (lims, val, idx): CSR, the output lims CUDA int64 [nq + 1] ([2] for one query); the
        entries of query q are those of its candidates whose exact squared distance is <= threshold (ip=True: whose
        inner product is >= threshold), IN THE ORDER IN WHICH THEY WERE NAMED, val the value flat_search_device returns
        for the row, bit for bit, idx the id as named; a row named twice is returned twice
        (pqhip_flat_range_among_f32_dev).  A NaN value never qualifies.  Fed the (lims, idx) of a range search over
        codes at a larger radius it returns the exact range result among those rows.  The result is allocated to its
        size: one count call, one read of the total -- the one synchronisation -- then the call that fills.  -1 is
        padding; any other id outside [0, N) is skipped and, like a bad lims, raises the range flag (check=True)."""
        import torch
        _, q2, vectors, nq, d, N, n_ids = self._flat_among_args(queries, vectors, ids, lims)
        dev = vectors.device
        thr = _marshal.threshold_arg(threshold, nq, dev)
        own_stream = stream is None
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        head = (cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d), ptr_or_none(vectors, N), vectors.element_size(), N, d,
                row_stride(vectors, N, d), ptr_or_none(lims), ptr_or_none(ids, n_ids), n_ids, 1 if ip else 0, thr.data_ptr())
        out_lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        _marshal.run("pqhip_flat_range_among_f32_dev", *head, out_lims.data_ptr(), None, None, 0, sp)
        if not own_stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        total = int(out_lims[-1])
        val = torch.empty(total, dtype=torch.float32, device=dev)
        idx = torch.empty(total, dtype=torch.int64, device=dev)
        if total > 0:
            _marshal.run("pqhip_flat_range_among_f32_dev", *head, out_lims.data_ptr(), val.data_ptr(), idx.data_ptr(), total, sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out_lims, val, idx

    # ---- exact search for query batches: f16 matrix-core screen, exact resolve -----------------------------------------------
    def _flat_screen_args(self, queries, vectors, allow):
        """What the screen and its compositions check and marshal (queries, vectors and mask as for flat_range_device,
        d <= FLAT_SCREEN_MAX_D) -> (single, q2, vectors, allow, nq, d, N)."""
        import torch
        for t, what in ((queries, "queries"), (vectors, "vectors")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if queries.dtype != torch.float32 or queries.dim() not in (1, 2):
            raise PanicError("queries must be float32 [d] or [nq, d]")
        if vectors.dtype not in (torch.float32, torch.float16) or vectors.dim() != 2:
            raise PanicError("vectors must be float32 or float16 [N, d]")
        single = queries.dim() == 1
        q2 = queries[None] if single else queries
        nq, d = q2.shape
        N = vectors.shape[0]
        if d < 1 or vectors.shape[1] != d:
            raise PanicError("Query and vector length mismatch")
        if d > FLAT_SCREEN_MAX_D:
            raise PanicError("the matrix-core screen serves vectors of at most %d elements, got %d" % (FLAT_SCREEN_MAX_D, d))
        allow = _marshal.vector_mask_words(allow, N)
        tensors = (queries, vectors) + (() if allow is None else (allow,))
        if not all(t.is_cuda for t in tensors):
            raise PanicError("queries, vectors and allow must be CUDA tensors")
        if any(t.device != vectors.device for t in tensors):
            raise PanicError("queries, vectors and allow must live on one device")
        if q2.stride(1) != 1:
            q2 = q2.contiguous()
        if N > 0 and vectors.stride(1) != 1:
            vectors = vectors.contiguous()
        if allow is not None:
            allow = _marshal.stand_in(allow, allow.shape[0], vectors.device)
        return single, q2, vectors, allow, nq, d, N

    def _flat_screen(self, queries, vectors, threshold, ip, allow, x_exp, cap, stream, retry):
        """One screen call with `cap` entries and, if retry and the result is larger, one more of exactly its size
        -> (lims, idx[:min(total, cap)], total); lims[-1] is read in between, the one synchronisation."""
        import torch
        _, q2, vectors, allow, nq, d, N = self._flat_screen_args(queries, vectors, allow)
        dev = vectors.device
        thr = _marshal.threshold_arg(threshold, nq, dev)
        cap = int(cap)
        if cap < 0:
            raise PanicError("capacity must not be negative")
        x_exp = int(x_exp)
        if not -(1 << 31) <= x_exp < (1 << 31):
            raise PanicError("x_exp must fit 32 bits")
        own_stream = stream is None
        cb, slot, sp = _marshal.launch(self, vectors, stream)
        head = (cb, slot, q2.data_ptr(), nq, row_stride(q2, nq, d), ptr_or_none(vectors, N), vectors.element_size(), N, d,
                row_stride(vectors, N, d), None if allow is None else allow.data_ptr(), 1 if ip else 0, x_exp, thr.data_ptr())
        lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        while True:
            idx = torch.empty(cap, dtype=torch.int64, device=dev)
            _marshal.run("pqhip_flat_screen_f32_dev", *head, lims.data_ptr(), ptr_or_none(idx, cap), cap, sp)
            if not own_stream:
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
            total = int(lims[-1])
            if total <= cap or not retry:
                break
            cap = total             # the second call always suffices
        return lims, idx[:min(total, cap)], total

    def flat_screen_device(self, queries, vectors, threshold, ip=False, allow=None, x_exp=0, capacity=None, stream=None,
                           check=False):
        """Conservative range screen on the matrix cores (pqhip_flat_screen_f32_dev): queries, vectors, allow and
        threshold as for flat_range_device (d <= 2048) -> (lims, idx): CSR, lims CUDA int64 [nq + 1], the ids of query q at
        idx[lims[q]:lims[q + 1]] in ascending order -- a SUPERSET of what flat_range_device returns at the same
        thresholds, within the allowed rows: a row is left out only when its exact value provably misses the threshold,
        and a regular row is returned only within the slack the header states.  x_exp: every row element is multiplied
        by 2^x_exp before it is rounded to f16 (flat_screen_x_exp chooses it from the largest |element|).  The capacity
        protocol is flat_range_device's: one call with `capacity` entries (default 1 << 20), one read of lims[-1] -- the
        one synchronisation -- and one more call of exactly its size if the result is larger; capacity=0 counts first.
        There is no range flag to raise; check=True only synchronises."""
        lims, idx, _ = self._flat_screen(queries, vectors, threshold, ip, allow, x_exp, (1 << 20) if capacity is None else capacity,
                                         stream, True)
        if check:
            import torch
            torch.cuda.synchronize(vectors.device)
        return lims, idx

    def flat_range_batch_device(self, queries, vectors, threshold, ip=False, allow=None, x_exp=None, capacity=None,
                                stream=None, check=False):
        """flat_range_device for a batch of queries: the matrix-core screen at the thresholds (flat_screen_device), then
        flat_range_among_device over its ids -> (lims, val, idx), bit for bit what flat_range_device returns: the screen
        returns a superset of the result in ascending row order, and the candidate call applies the same predicate to
        the same values in the order named.  x_exp None: chosen from the largest |element| of vectors
        (flat_screen_x_exp; one reduction over the matrix -- pass it when it is known).  d <= 2048."""
        if x_exp is None:
            x_exp = flat_screen_x_exp(_matrix_max_abs(vectors))
        lims, ids = self.flat_screen_device(queries, vectors, threshold, ip=ip, allow=allow, x_exp=x_exp, capacity=capacity,
                                            stream=stream)
        return self.flat_range_among_device(queries, vectors, ids, threshold, lims=lims, ip=ip, stream=stream, check=check)

    def flat_search_batch_device(self, queries, vectors, k, ip=False, allow=None, x_exp=None, stream=None, check=False,
                                 stats=None):
        """flat_search_device for a batch of queries, bit for bit in values and ids, at about one stream of the matrix
        per 64 queries instead of one per 4 (d <= 2048).  Sample: every t-th row (flat_batch_sample; -1 where the mask
        disallows it) through flat_among_device; T_q, its k-th value, is a valid threshold whatever the sample -- k rows
        have a value at or below it, so every member of the true top-k has.  Screen at T_q (flat_screen_device): a
        superset of those rows.  Resolve: flat_among_device over the screen's ids, which is the masked search on a
        superset of its result.  A query whose sample holds fewer than k numbers, and a chunk of queries whose
        candidates exceed FLAT_BATCH_FALLBACK_FRACTION of n nq (flat_batch_falls_back), take flat_search_device.
        stats: a dict that receives the candidate total, the queries that fell back and the sample size."""
        import torch
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        single, q2, vectors, allow, nq, d, N = self._flat_screen_args(queries, vectors, allow)
        dev = vectors.device
        if N == 0 or nq == 0:
            return self.flat_search_device(queries, vectors, k, ip=ip, allow=allow, stream=stream, check=check)
        if x_exp is None:
            x_exp = flat_screen_x_exp(_matrix_max_abs(vectors))
        S, t = flat_batch_sample(N, k)
        ids = torch.arange(0, N, t, dtype=torch.int64, device=dev)
        if allow is not None:
            bit = (allow[ids >> 5] >> (ids & 31).to(torch.int32)) & 1
            ids = torch.where(bit != 0, ids, torch.full_like(ids, -1))
        sval, sidx = self.flat_among_device(q2, vectors, ids, k, ip=ip, stream=stream)
        T = sval[:, k - 1]
        thin = (sidx[:, k - 1] < 0) | torch.isnan(T)
        nothing = float("inf") if ip else float("-inf")          # a thin query screens nothing and takes the plain call
        thr = torch.where(thin, torch.full_like(T, nothing), T)
        val = torch.empty((nq, k), dtype=torch.float32, device=dev)
        idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
        plain = thin.clone()
        total_all = 0
        for q0 in range(0, nq, FLAT_BATCH_CHUNK):
            q1 = min(nq, q0 + FLAT_BATCH_CHUNK)
            cap = flat_batch_capacity(N, q1 - q0, k, S)
            lims, cand, total = self._flat_screen(q2[q0:q1], vectors, thr[q0:q1], ip, allow, x_exp, cap, stream, False)
            total_all += total
            if flat_batch_falls_back(total, N, q1 - q0):
                plain[q0:q1] = True
                continue
            val[q0:q1], idx[q0:q1] = self.flat_among_device(q2[q0:q1], vectors, cand, k, lims=lims, ip=ip, stream=stream)
        rows = torch.nonzero(plain).reshape(-1)
        if rows.shape[0] > 0:
            val[rows], idx[rows] = self.flat_search_device(q2[rows], vectors, k, ip=ip, allow=allow, stream=stream)
        if stats is not None:
            stats.update(candidates=total_all, fallback_queries=int(rows.shape[0]), sample=int(ids.shape[0]), x_exp=int(x_exp))
        if check:
            torch.cuda.synchronize(dev)
        return (val[0], idx[0]) if single else (val, idx)

    # ---- growing a partitioned matrix: merge of two list-ordered arrays ------------------------------------------------
    def merge_lists_device(self, list_off_a, a, list_off_b, b, out=None, stream=None, check=False):
        """a, b: CUDA tensors of one dtype, [n_a] / [n_b] or [n_a, c] / [n_b, c], contiguous, their rows in list order
        under list_off_a / list_off_b (CUDA int64 [n_lists + 1]) -> (out, list_off_out): out [n_a + n_b(, c)] holds, for
        every list, its rows of a followed by its rows of b, copied byte for byte (a row is element size x c bytes, at
        most 4,096); list_off_out = list_off_a + list_off_b (pqhip_lists_merge_dev).  None of the tensors needs any
        alignment; out, if given, must not overlap an input.  The offsets are checked on the device: if one of them
        does not start at 0, decreases somewhere or does not end at the number of rows, out is left as it was and
        the stream's range flag is raised (check=True: synchronises and raises PanicError).  The quantizer of self is
        not used."""
        import torch
        for t, what in ((list_off_a, "list_off_a"), (a, "a"), (list_off_b, "list_off_b"), (b, "b")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if a.dtype != b.dtype:
            raise PanicError("a and b must have one dtype, got %s and %s" % (a.dtype, b.dtype))
        if a.dim() not in (1, 2) or b.dim() != a.dim() or tuple(a.shape[1:]) != tuple(b.shape[1:]):
            raise PanicError("a and b must be vectors, or matrices with the same number of columns")
        if list_off_a.dtype != torch.int64 or list_off_b.dtype != torch.int64 or list_off_a.dim() != 1 \
                or list_off_a.shape != list_off_b.shape or list_off_a.shape[0] < 1:
            raise PanicError("the list offsets must be two int64 vectors of one length, n_lists + 1")
        n_a, n_b, n_lists = a.shape[0], b.shape[0], list_off_a.shape[0] - 1
        shape = (n_a + n_b,) + tuple(a.shape[1:])
        row_bytes = a.element_size() * (a.shape[1] if a.dim() == 2 else 1)
        if not 1 <= row_bytes <= 4096:
            raise PanicError("a row must have between 1 and 4096 bytes, has %d" % row_bytes)
        if n_lists == 0 and n_a + n_b > 0:
            raise PanicError("rows need at least one list")
        if out is not None and (not hasattr(out, "is_cuda") or out.dtype != a.dtype or tuple(out.shape) != shape):
            raise PanicError("out must be a %s tensor of shape %s" % (a.dtype, list(shape)))
        for t in (a, b, list_off_a, list_off_b) + (() if out is None else (out,)):
            if not t.is_contiguous():
                raise PanicError("merge_lists_device takes contiguous tensors")
        if not (a.is_cuda and b.is_cuda and list_off_a.is_cuda and list_off_b.is_cuda and (out is None or out.is_cuda)):
            raise PanicError("merge_lists_device takes CUDA tensors")
        if not (a.device == b.device == list_off_a.device == list_off_b.device and (out is None or out.device == a.device)):
            raise PanicError("all tensors of a merge must live on one device")
        if out is None:
            out = torch.empty(shape, dtype=a.dtype, device=a.device)
        off_out = torch.empty(n_lists + 1, dtype=torch.int64, device=a.device)
        cb, slot, sp = _marshal.launch(self, a, stream)
        _marshal.run("pqhip_lists_merge_dev", cb, slot, list_off_a.data_ptr(), n_a, list_off_b.data_ptr(), n_b, n_lists,
                     row_bytes, ptr_or_none(a, n_a), ptr_or_none(b, n_b), ptr_or_none(out, n_a + n_b), off_out.data_ptr(), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out, off_out

    # ---- removing rows from a resident matrix: stable compaction under a row mask --------------------------------------
    def compact_rows_device(self, keep_words, rows, list_off=None, want_src_rows=False, capacity=None, out=None, n=None,
                            stream=None, check=False):
        """The kept rows of `rows`, in order (pqhip_rows_compact_dev).  keep_words: the mask words of the searches' `allow=`
        (pack_row_mask_device), CUDA int32 [ceil(n / 32)], bit set = the row is kept; tail bits of the last word are
        ignored.  rows: a contiguous CUDA tensor [n] or [n, w] of any dtype whose rows have between 1 and 4,096 bytes, or
        None for the plan-only call (n= is then required): the count, the offsets and the source rows, no row moved.
        list_off: None or CUDA int64 [n_lists + 1], the list offsets of a list-ordered `rows`.
        -> (out, list_off_out or None, src_rows or None, count): count the number of kept rows (an int: the stream is
        synchronised to read it), out [count(, w)] row j = the j-th kept row byte for byte (None for the plan-only call),
        list_off_out[l] = kept rows below list_off[l] (the offsets of the compacted lists), src_rows int64 [count] the
        numbers of the kept rows (want_src_rows).
        capacity=None: one plan-only call, the read of the count, an output allocated to its size, then the moving call.
        capacity=c (or out= given, whose rows are the capacity): one call into c rows; if more rows are kept nothing is
        written, out and src_rows come back as None and count tells the size to call again with.  out, if given, must
        not overlap rows; no tensor needs any alignment.  The offsets are checked on the device: if they do not start
        at 0, decrease somewhere or do not end at n, nothing is written, count is unspecified and the stream's range
        flag is raised (check=True: raises PanicError).  The quantizer of self is not used."""
        import torch
        tensors = [(keep_words, "keep_words")] + [(t, what) for t, what in ((rows, "rows"), (list_off, "list_off"), (out, "out"))
                                                  if t is not None]
        for t, what in tensors:
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if rows is None:
            if n is None or out is not None:
                raise PanicError("the plan-only call (rows=None) takes n= and no out=")
            n, tail, row_bytes = int(n), (), 1
        else:
            if rows.dim() not in (1, 2):
                raise PanicError("rows must be a vector or a matrix")
            if n is not None and int(n) != rows.shape[0]:
                raise PanicError("n must be the number of rows")
            n, tail = rows.shape[0], tuple(rows.shape[1:])
            row_bytes = rows.element_size() * (rows.shape[1] if rows.dim() == 2 else 1)
            if not 1 <= row_bytes <= 4096:
                raise PanicError("a row must have between 1 and 4096 bytes, has %d" % row_bytes)
        if n < 0:
            raise PanicError("n must not be negative")
        if keep_words.dtype != torch.int32 or keep_words.dim() != 1 or keep_words.shape[0] != (n + 31) // 32:
            raise PanicError("the row mask must hold ceil(n / 32) int32 words for the n rows")
        if list_off is not None and (list_off.dtype != torch.int64 or list_off.dim() != 1 or list_off.shape[0] < 1):
            raise PanicError("the list offsets must be an int64 vector of length n_lists + 1")
        if capacity is not None and int(capacity) < 0:
            raise PanicError("capacity must not be negative")
        if out is not None:
            if out.dtype != rows.dtype or out.dim() != rows.dim() or tuple(out.shape[1:]) != tail:
                raise PanicError("out must be a %s tensor of shape %s" % (rows.dtype, ["capacity"] + list(tail)))
            if capacity is not None and out.shape[0] < int(capacity):
                raise PanicError("out holds fewer rows than the capacity")
        for t, what in tensors:
            if not t.is_contiguous():
                raise PanicError("compact_rows_device takes contiguous tensors")
        if not all(t.is_cuda for t, _ in tensors):
            raise PanicError("compact_rows_device takes CUDA tensors")
        dev = keep_words.device
        if not all(t.device == dev for t, _ in tensors):
            raise PanicError("all tensors of a compaction must live on one device")
        n_lists = 0 if list_off is None else list_off.shape[0] - 1
        off_out = None if list_off is None else torch.empty(n_lists + 1, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        own_stream = stream is None
        cb, slot, sp = _marshal.launch(self, keep_words, stream)

        def call(cap, dst, src):
            """one call of the entry point -> the count, read after a synchronisation of the stream"""
            moving = rows is not None and dst is not None
            _marshal.run("pqhip_rows_compact_dev", cb, slot, ptr_or_none(keep_words, n), n, row_bytes,
                         ptr_or_none(rows, n) if moving else None, ptr_or_none(dst, n) if moving else None, cap,
                         ptr_or_none(list_off), n_lists, ptr_or_none(off_out), ptr_or_none(src, cap), count.data_ptr(), sp)
            if not own_stream:
                torch.cuda.ExternalStream(stream, device=dev).synchronize()
            return int(count)

        wants = rows is not None or want_src_rows
        if capacity is None and out is None and wants:
            capacity = min(max(call(0, None, None), 0), n)         # (an invalid offset array leaves any count)
        cap = 0 if not wants else int(capacity) if capacity is not None else out.shape[0]
        dst = None
        if rows is not None:
            # the entry point wants an address for the output whenever it has one for the input
            dst = out if out is not None and out.numel() else torch.empty((max(cap, 1),) + tail, dtype=rows.dtype, device=dev)
        src = torch.empty(cap, dtype=torch.int64, device=dev) if want_src_rows else None
        total = call(cap, dst, src)
        if check:
            _marshal.check_range(cb, slot, sp)
        fits = total <= cap
        if rows is not None:
            dst = (out if out is not None else dst)[:total] if fits else None
        return dst, off_out, (src[:total] if fits else None) if want_src_rows else None, total

    # ---- searching several matrices as one: exact merge of the parts' top-k results ------------------------------------
    def merge_topk_device(self, vals, ids, k, largest=False, offsets=None, want_parts=False, stream=None):
        """The k best of each query over the results of P searches (pqhip_topk_merge_f32_dev).  vals CUDA float32 and ids
        CUDA int64, both [P, nq, k_in]: row q of part p is what a search of part p returned for query q, real entries
        first in that search's order, then padding with index -1.  They may be views with any part and row stride (a
        column stride other than one is removed by a copy).  offsets: None or CUDA int64 [P], added to every id >= 0 of
        its part.  largest=False merges distances, True scores.  -> (val, idx), CUDA float32 and int64 [nq, k], and with
        want_parts a third tensor, int32 [nq, k]: the part of each result.  The entries of a query are ordered by (value
        in the library's order: -0 == +0, NaN last; part; rank within the part's row): the merge is stable by part and
        never compares ids, so parts that are consecutive row ranges of one matrix, in order, give that matrix's
        exhaustive search bit for bit.  Past the last entry: index -1, +Inf (largest: -Inf), part -1.  1 <= k, k_in <=
        1024, P <= 65536; k > P k_in is allowed.  The quantizer of self is not used."""
        import torch
        for t, what in ((vals, "vals"), (ids, "ids")) + (() if offsets is None else ((offsets, "offsets"),)):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % what)
        if vals.dtype != torch.float32 or vals.dim() != 3:
            raise PanicError("vals must be float32 [P, nq, k_in]")
        if ids.dtype != torch.int64 or tuple(ids.shape) != tuple(vals.shape):
            raise PanicError("ids must be int64 of the shape of vals")
        P, nq, k_in = vals.shape
        if not 1 <= P <= 65536:
            raise PanicError("between 1 and 65536 parts expected, got %d" % P)
        if not 1 <= k_in <= 1024:
            raise PanicError("between 1 and 1024 entries per part and query expected, got %d" % k_in)
        k = int(k)
        if not 1 <= k <= 1024:
            raise PanicError("k must be between 1 and 1024, was %d" % k)
        if offsets is not None and (offsets.dtype != torch.int64 or tuple(offsets.shape) != (P,)):
            raise PanicError("offsets must be int64 [P], one per part")
        if not (vals.is_cuda and ids.is_cuda and (offsets is None or offsets.is_cuda)):
            raise PanicError("merge_topk_device takes CUDA tensors")
        dev = vals.device
        if ids.device != dev or (offsets is not None and offsets.device != dev):
            raise PanicError("all tensors of a merge must live on one device")
        if vals.stride(2) != 1:
            vals = vals.contiguous()
        if ids.stride(2) != 1:
            ids = ids.contiguous()
        if offsets is not None:
            offsets = offsets.contiguous()
        val = torch.empty((nq, k), dtype=torch.float32, device=dev)
        idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
        part = torch.empty((nq, k), dtype=torch.int32, device=dev) if want_parts else None
        cb, slot, sp = _marshal.launch(self, vals, stream)
        v_rs = vals.stride(1) if nq > 1 else max(vals.stride(1), k_in)
        i_rs = ids.stride(1) if nq > 1 else max(ids.stride(1), k_in)
        _marshal.run("pqhip_topk_merge_f32_dev", cb, slot, ptr_or_none(vals, nq), vals.stride(0), v_rs,
                     ptr_or_none(ids, nq), ids.stride(0), i_rs, P, nq, k_in, ptr_or_none(offsets), 1 if largest else 0, k,
                     ptr_or_none(val, nq), k, ptr_or_none(idx, nq), k, ptr_or_none(part, nq), k, sp)
        return (val, idx, part) if want_parts else (val, idx)

    # ---- building a partitioned matrix on the device: list layout, residuals, query-free row terms -----------------------
    def lists_layout_device(self, assign, n_lists, want_lists=False, stream=None, check=False):
        """assign: CUDA int32 or int64 vector [n] of list ids in [0, n_lists), contiguous -> (ids, list_off, positions) or,
        with want_lists, (ids, list_off, positions, lists), all CUDA int64: what qmatrix.ivf_layout defines, computed on
        the device (pqhip_lists_layout_dev).  ids [n] is the STABLE argsort of the assignments (positions inside a list
        ascend in row number), list_off [n_lists + 1] the prefix sums of the list sizes (empty lists are legal),
        positions[ids[p]] = p and lists[p] = assign[ids[p]].  1 <= n_lists <= 16384.  The ids are checked on the device:
        if one lies outside [0, n_lists), ids, positions and lists are left as allocated and the stream's range flag is
        raised (check=True: synchronises and raises PanicError).  The quantizer of self is not used."""
        import torch
        if not hasattr(assign, "is_cuda"):
            raise PanicError("assign must be a torch tensor")
        if assign.dtype not in (torch.int32, torch.int64) or assign.dim() != 1:
            raise PanicError("assign must be an int32 or int64 vector of list ids")
        n_lists = int(n_lists)
        if not 1 <= n_lists <= 16384:
            raise PanicError("the number of lists must be between 1 and 16384, was %d" % n_lists)
        if not assign.is_contiguous():
            raise PanicError("lists_layout_device takes a contiguous vector")
        if not assign.is_cuda:
            raise PanicError("lists_layout_device takes a CUDA tensor")
        n, dev = assign.shape[0], assign.device
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        positions = torch.empty(n, dtype=torch.int64, device=dev)
        lists = torch.empty(n, dtype=torch.int64, device=dev) if want_lists else None
        list_off = torch.empty(n_lists + 1, dtype=torch.int64, device=dev)
        cb, slot, sp = _marshal.launch(self, assign, stream)
        _marshal.run("pqhip_lists_layout_dev", cb, slot, ptr_or_none(assign, n), assign.element_size(), n, n_lists,
                     list_off.data_ptr(), ptr_or_none(ids, n), ptr_or_none(positions, n), ptr_or_none(lists, n), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return (ids, list_off, positions, lists) if want_lists else (ids, list_off, positions)

    @staticmethod
    def _check_rows_lists(what, assign, centroids, n, d):
        """the (assign, centroids) pair of the two residual calls: int64 [n] and float32 [n_lists, d], contiguous"""
        import torch
        for t, name in ((assign, "assign"), (centroids, "centroids")):
            if not hasattr(t, "is_cuda"):
                raise PanicError("%s must be a torch tensor" % name)
        if assign.dtype != torch.int64 or tuple(assign.shape) != (n,):
            raise PanicError("assign must be an int64 vector with one list id per row (%d)" % n)
        if centroids.dtype != torch.float32 or centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1:
            raise PanicError("centroids must be float32 [n_lists, %d] with at least one list" % d)
        if not assign.is_contiguous() or not centroids.is_contiguous():
            raise PanicError("%s takes contiguous assign and centroids" % what)

    def residuals_device(self, x, assign, centroids, out=None, stream=None, check=False):
        """x: CUDA float32 [n, d] (unit column stride, any row stride), assign: CUDA int64 [n], centroids: CUDA float32
        [n_lists, d] -> out float32 [n, d] with out[i] = x[i] - centroids[assign[i]], one IEEE subtraction per element:
        bit for bit what the torch expression x - centroids[assign] gives, in one pass and without the gathered
        temporary (pqhip_residuals_f32_dev).  out, if given, is float32 [n, d] with unit column stride and must not
        overlap x.  A list id outside [0, n_lists) gives a zero row and raises the stream's range flag (check=True:
        synchronises and raises PanicError).  d is the width of x: the quantizer of self is not used."""
        import torch
        if not hasattr(x, "is_cuda"):
            raise PanicError("x must be a torch tensor")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 1:
            raise PanicError("x must be float32 [n, d]")
        n, d = x.shape
        self._check_rows_lists("residuals_device", assign, centroids, n, d)
        if out is not None and (not hasattr(out, "is_cuda") or out.dtype != torch.float32 or tuple(out.shape) != (n, d)):
            raise PanicError("out must be a float32 tensor of shape [%d, %d]" % (n, d))
        if x.stride(1) != 1 or (out is not None and out.stride(1) != 1):
            raise PanicError("residuals_device takes rows with unit column stride")
        if not (x.is_cuda and assign.is_cuda and centroids.is_cuda and (out is None or out.is_cuda)):
            raise PanicError("residuals_device takes CUDA tensors")
        if not (x.device == assign.device == centroids.device and (out is None or out.device == x.device)):
            raise PanicError("all tensors of residuals_device must live on one device")
        if out is None:
            out = torch.empty((n, d), dtype=torch.float32, device=x.device)
        cb, slot, sp = _marshal.launch(self, x, stream)
        _marshal.run("pqhip_residuals_f32_dev", cb, slot, ptr_or_none(x, n), n, d, row_stride(x, n, d), ptr_or_none(assign, n),
                     centroids.data_ptr(), centroids.shape[0], ptr_or_none(out, n), row_stride(out, n, d), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out

    def residual_terms_device(self, codes, assign, centroids, out=None, stream=None, check=False):
        """self is the residual quantizer (no projection, at most 256 centroids); codes: CUDA uint8 [n, M] (unit column
        stride, any row stride), assign: CUDA int64 [n], centroids: CUDA float32 [n_lists, d] -> out float32 [n], the
        query-free terms t_i = sum_j (r_ij^2 + 2 c_ij r_ij) of the rows, r the reconstruction of the code row and c
        the centroid of its list -- computed from the codebook entries, no reconstruction is written anywhere
        (pqhip_residual_terms_f32_dev).  The order of the f64 arithmetic is fixed: per subquantizer the sequential sum
        over its columns of (r r + 2 c r), then the sequential sum of these over the subquantizers, rounded once to f32
        (tests/residual_terms_ref.py is this definition in numpy).  A code >= K reads entry 0, a list id outside
        [0, n_lists) gives +0; both raise the stream's range flag (check=True: synchronises and raises PanicError).
        A quantizer with a projection is refused (PanicError): its reconstruction includes the inverse rotation."""
        import torch
        if not hasattr(codes, "is_cuda"):
            raise PanicError("codes must be a torch tensor")
        if self._projection is not None:
            raise PanicError("residual_terms_device does not serve a quantizer with a projection")
        if self.n_quantizer_centroids() > 256:
            raise PanicError("residual_terms_device reads 1-byte codes: at most 256 centroids")
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != self.quantized_len():
            raise PanicError("codes must be uint8 [n, %d]" % self.quantized_len())
        n, d = codes.shape[0], self.reconstructed_len()
        self._check_rows_lists("residual_terms_device", assign, centroids, n, d)
        if out is not None and (not hasattr(out, "is_cuda") or out.dtype != torch.float32 or tuple(out.shape) != (n,)
                                or not out.is_contiguous()):
            raise PanicError("out must be a contiguous float32 tensor of shape [%d]" % n)
        if codes.stride(1) != 1:
            raise PanicError("residual_terms_device takes code rows with unit column stride")
        if not (codes.is_cuda and assign.is_cuda and centroids.is_cuda and (out is None or out.is_cuda)):
            raise PanicError("residual_terms_device takes CUDA tensors")
        if not (codes.device == assign.device == centroids.device and (out is None or out.device == codes.device)):
            raise PanicError("all tensors of residual_terms_device must live on one device")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=codes.device)
        cb, slot, sp = _marshal.launch(self, codes, stream)
        _marshal.run("pqhip_residual_terms_f32_dev", cb, slot, ptr_or_none(codes, n), n,
                     row_stride(codes, n, self.quantized_len()), ptr_or_none(assign, n), centroids.data_ptr(),
                     centroids.shape[0], ptr_or_none(out, n), sp)
        if check:
            _marshal.check_range(cb, slot, sp)
        return out
