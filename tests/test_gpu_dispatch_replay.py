"""The encode dispatch golden file (tests/golden/encode_dispatch.txt), replayed on the device: one case per call line but the two
2^46-row calls (dispatch_golden.EXCLUDED).  Each case builds the handle the mock saw (the golden's centroids, the context
options and forced variant of the line; for OPQ a seeded orthonormal projection instead of the mock's identity) and calls the
C ABI on device buffers laid out as the line says (row offset and stride, code offset, stride and width).  It asserts:

- the golden's status, pqhip_last_encode_kernel and launch log: the device makes the decision the mock recorded;
- codes equal to the oracle's (kmeans.rs:141-156 per sub-vector) at the line's index width;
- nothing outside the output window written: the code allocation is pre-filled with a sentinel that the row padding, the
  leading offset bytes and the slack after the last row keep -- all of it for refused calls and empty batches;
- the input rows unchanged.

k-means lines compare the new centroids and the loss with the oracle bit for bit.  The rows are built to make kernels fail:
near-ties around the (2^-16-grid) centroids, exact centroids, midpoints of a centroid and its nearest neighbour (an exact tie:
the lower index wins), rows far outside the unit box, and NaN / +Inf / -Inf / 1e19-scaled / zero rows at both ends of the batch.
Everything is seeded from the call's shape, so a failure reproduces, and lines of one shape share the oracle's result."""
import ctypes
import zlib

import numpy as np
import pytest

import dispatch_golden as dg
from oracle import pq_oracle as orc

pytestmark = pytest.mark.gpu

CALLS = dg.replay_plan(dg.parse())
SENTINEL = 0xA5
SLACK = 64                            # bytes after the last code row
SAMPLE_ABOVE = 1 << 21                # batches larger than this are compared with the oracle on a sample of rows
X_PAD_VALUE = 1e30                    # row padding and slack of the input buffer
_oracle_cache = {}


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.fixture(scope="module")
def ctx(ra):
    """A context of the module's own; every codebook made on it (_pq) is destroyed before it, failed cases' included."""
    from reductive_amd.pq import _Ctx
    c = _Ctx()
    c.pqs = []
    yield c
    for pq in c.pqs:
        pq.close()
    c.close()


def _pq(ra, ctx, P, q):
    pq = ra.Pq(P, q, ctx=ctx)
    ctx.pqs.append(pq)
    return pq


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _nearest_other(q):
    """[M, K] index of each centroid's nearest other centroid (itself when K == 1)."""
    M, K, _ = q.shape
    nn = np.zeros((M, K), np.int64)
    if K == 1:
        return nn
    for m in range(M):
        c = q[m].astype(np.float64)
        dist = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(dist, np.inf)
        nn[m] = dist.argmin(1)
    return nn


def _rows(q, n, seed, finite=False):
    """[n, d] float32 rows on the device.  Row r's class is r % 8: Gaussian noise of three widths around a random centroid per
    sub-vector (0-2), the centroid itself (3), the midpoint of the centroid and its nearest other centroid -- exact in f32, as
    the centroids are multiples of 2^-16 (4, 7), uniform in [-100, 100] (5), uniform in [-1, 2] (6).  The first and the last
    min(5, n // 4) rows are NaN, +Inf and -Inf (in the first component of every sub-vector of a midpoint row), a midpoint row
    times 1e19 and a zero row; `finite` (k-means) keeps only the zero row of these."""
    import torch
    M, K, dsub = q.shape
    d = M * dsub
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    qd = torch.from_numpy(q).to(dev)
    nn = torch.from_numpy(_nearest_other(q)).to(dev)
    mi = torch.arange(M, device=dev)[None, :]
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    chunk = max(1, (1 << 24) // max(d, 1))
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        a = torch.randint(0, K, (r1 - r0, M), generator=g, device=dev)
        cen = qd[mi, a]
        mid = (cen + qd[mi, nn[mi, a]]) * 0.5
        cls = (torch.arange(r0, r1, device=dev) % 8)[:, None, None]
        noise = torch.randn(cen.shape, generator=g, device=dev)
        far = torch.rand(cen.shape, generator=g, device=dev)
        v = cen + noise * 1e-3
        v = torch.where(cls == 1, cen + noise * 3e-2, v)
        v = torch.where(cls == 2, cen + noise * 0.2, v)
        v = torch.where(cls == 3, cen, v)
        v = torch.where((cls == 4) | (cls == 7), mid, v)
        v = torch.where(cls == 5, far * 200 - 100, v)
        v = torch.where(cls == 6, far * 3 - 1, v)
        x[r0:r1] = v.reshape(r1 - r0, d)
        if r0 == 0:
            mid0 = mid[: min(5, r1)].reshape(-1, d).clone()
    s = min(5, n // 4)
    for base in (0, n - s):
        for j in range(s):
            r, row = base + j, mid0[j % mid0.shape[0]].clone()
            if finite and j < 4:
                continue
            if j < 3:
                row.view(M, dsub)[:, 0] = (float("nan"), float("inf"), float("-inf"))[j]
            elif j == 3:
                row = row * 1e19
            else:
                row.zero_()
            x[r] = row
    return x


def _sample(n, seed):
    """Rows compared with the oracle: all of them, or for large batches the first and last 4096 plus 8192 seeded rows."""
    if n <= SAMPLE_ABOVE:
        return None
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(4096), np.arange(n - 4096, n), rng.integers(0, n, 8192)]))


def _oracle(c, q, P, x, rows):
    key = (c.kind, c.M, c.K, c.dsub, c.n)
    if key not in _oracle_cache:
        xs = x if rows is None else x[rows]
        with np.errstate(all="ignore"):
            _oracle_cache[key] = orc.quantize_batch(q, xs.cpu().numpy(), projection=P, n_threads=16,
                                                    dtype=np.uint8 if c.K <= 256 else np.uint32).astype(np.uint64)
    return _oracle_cache[key]


def _variant_case(ra, ctx, c):
    pq = _pq(ra, ctx, None, dg.centroids(1, 4, 2))
    assert ra._lib.lib().pqhip_set_encode_variant(pq._cb(), c.variant) == c.status
    pq.close()


def _encode_case(ra, ctx, c):
    import torch
    L = ra._lib.lib()
    M, K, dsub, d, n, cb = c.M, c.K, c.dsub, c.d, c.n, c.code_bytes
    seed = _seed(c.kind, M, K, dsub, n)
    q = dg.centroids(M, K, dsub)
    P = None
    if c.kind == "opq":
        import synth
        P = synth.orthonormal(_seed("P", M, dsub), d)
    ctx.set_option("candidate_tables", c.tables)
    ctx.set_option("opq_fused", c.fused)
    pq = _pq(ra, ctx, P, q)
    h = pq._cb()
    assert L.pqhip_set_encode_variant(h, c.variant) == 0

    x = _rows(q, n, seed)
    x_rs, o_rs = d + c.x_pad, M + c.o_pad
    xbuf = torch.full((c.x_off + n * x_rs + 16,), X_PAD_VALUE, dtype=torch.float32, device="cuda")
    xbuf[c.x_off:c.x_off + n * x_rs].view(n, x_rs)[:, :d] = x
    x_before = xbuf.clone()
    nbytes = c.c_off + n * o_rs * cb + SLACK
    cbuf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    ra.launch_log(reset=True)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.pqhip_quantize_batch_f32_dev(h, 0, xbuf.data_ptr() + 4 * c.x_off, n, x_rs, cbuf.data_ptr() + c.c_off, cb, o_rs,
                                        ctypes.c_void_p(stream))
    torch.cuda.synchronize()
    log = ra.launch_log(reset=True)
    what = (c.line, pq.last_encode_kernel(), log)
    assert rc == c.status, what
    assert pq.last_encode_kernel() == c.kernel, what
    assert log == c.log, what
    assert torch.equal(xbuf.view(torch.int32), x_before.view(torch.int32)), ("input rows modified",) + what
    del x_before

    host = cbuf.cpu().numpy()
    if rc != 0 or n == 0:
        assert (host == SENTINEL).all(), ("refused call wrote its output", np.flatnonzero(host != SENTINEL)[:8]) + what
        pq.close()
        return
    end = c.c_off + n * o_rs * cb
    assert (host[:c.c_off] == SENTINEL).all() and (host[end:] == SENTINEL).all(), ("wrote before / after the codes",) + what
    region = host[c.c_off:end].reshape(n, o_rs * cb)
    assert (region[:, M * cb:] == SENTINEL).all(), ("wrote the code row padding",) + what
    got = np.ascontiguousarray(region[:, :M * cb]).view("<u%d" % cb).astype(np.uint64)
    rows = _sample(n, seed)
    want = _oracle(c, q, P, x, None if rows is None else torch.from_numpy(rows).cuda())
    if rows is not None:
        got = got[rows]
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, ("codes differ from the oracle in %d rows, first %s" % (bad.size, bad[:8].tolist()),
                           got[bad[:2]].tolist(), want[bad[:2]].tolist()) + what
    pq.close()


def _kmeans_case(ra, ctx, c):
    import torch
    L = ra._lib.lib()
    M, K, dsub, d, n = c.M, c.K, c.dsub, c.d, c.n
    q0 = dg.centroids(M, K, dsub)
    x = _rows(q0, n, _seed(c.kind, M, K, dsub, n), finite=True)
    x_before = x.clone()
    ctx.set_option("kmeans_no_graph", c.no_graph)
    q = q0.copy()
    loss = np.zeros(M, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    torch.cuda.synchronize()
    ra.launch_log(reset=True)
    try:
        rc = L.pqhip_kmeans_iterations_f32_dev(ctx.handle, 0, q.ctypes.data_as(fp), M, K, dsub, x.data_ptr(), n, d,
                                               c.iterations, loss.ctypes.data_as(fp),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("kmeans_no_graph", 0)
    log = ra.launch_log(reset=True)
    assert (rc, log) == (c.status, c.log), c.line
    assert torch.equal(x.view(torch.int32), x_before.view(torch.int32)), ("input rows modified", c.line)
    if rc != 0:
        return
    want_q, want_loss = orc.kmeans_iterations(q0, x.cpu().numpy(), n_iterations=c.iterations, n_threads=16)
    assert q.tobytes() == want_q.tobytes(), ("centroids differ from the oracle", c.line)
    assert loss.tobytes() == want_loss.tobytes(), ("loss differs from the oracle", c.line, loss, want_loss)


@pytest.mark.parametrize("c", CALLS, ids=dg.case_ids(CALLS))
def test_golden_call_on_device(ra, ctx, c):
    if c.kind == "variant":
        _variant_case(ra, ctx, c)
    elif c.kind == "kmeans":
        _kmeans_case(ra, ctx, c)
    else:
        _encode_case(ra, ctx, c)
