"""Growing the three matrix classes on the GPU (qmatrix: _Lists.assign / extend, ResidualPartitionedMatrix.encode, add of
all three).  The result of a growth is DEFINED by the constructors: m.add(x) equals, tensor for tensor, the constructor
applied to the concatenation, in original row order, of what m stores and what assign / encode / quantize_batch_device
give for x.  So every comparison here is torch.equal against a matrix built in one go; assign and encode themselves are
checked against the oracle (the row terms within the float64 accumulation bound that
test_gpu_adc_search_lists_residual.py derives).  Shapes: M = 15, K = 256, dsub = 4, N = 30,011 in 24 lists, B in {1, 4099};
one case with 300 lists (the coarse codes need more than a byte) and one with d = 300 (coarse sub-vectors wider than 256
floats)."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

pytestmark = pytest.mark.gpu

N, B = 30011, 4099
CONFIGS = {"base": (15, 4, 24), "lists300": (15, 4, 300), "wide": (15, 20, 24)}       # M, dsub, n_lists (K = 256)
LIST_TENSORS = ("ids", "list_off", "positions", "codes", "norms")
RESIDUAL_TENSORS = LIST_TENSORS + ("row_terms", "lists")


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


_WORLDS = {}


def world(ra, name):
    """One data set per configuration, computed once: N old and B new vectors around 40 centres, the quantizer of the
    vectors, a residual quantizer, centroids (n_lists distinct rows), the oracle's assignments of all N + B vectors,
    norms, and -- through the library's own helper, the loop body of partition_residual -- the residual codes and row
    terms of the old rows."""
    import torch
    from reductive_amd import qmatrix
    if name in _WORLDS:
        return _WORLDS[name]
    M, dsub, n_lists = CONFIGS[name]
    d, seed = M * dsub, 7000 + 10 * sorted(CONFIGS).index(name)
    w = type("World", (), {})()
    w.M, w.d, w.n_lists = M, d, n_lists
    w.pq = ra.Pq(None, synth.normalish(seed, (M, 256, dsub)))
    w.rpq = ra.Pq(None, synth.normalish(seed + 1, (M, 256, dsub)) * np.float32(0.7))
    centres = synth.normalish(seed + 2, (40, d)) * np.float32(3.0)
    w.x = (centres[np.random.default_rng(seed + 3).integers(0, 40, N + B)] + synth.normalish(seed + 4, (N + B, d))).astype(np.float32)
    w.centroids = np.ascontiguousarray(w.x[np.random.default_rng(seed + 5).choice(N, n_lists, replace=False)])
    w.assign = orc.cluster_assignments(w.centroids, w.x).astype(np.int64)
    w.norms = synth.uniform01(seed + 6, (N + B,)) + np.float32(0.5)
    w.xd = torch.from_numpy(w.x).cuda()
    w.codes = w.pq.quantize_batch_device(w.xd)                               # [N + B, M] u8: the flat codes of every vector
    cd = torch.from_numpy(w.centroids).cuda()
    w.rcodes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    w.rterms = qmatrix._residual_codes_terms(w.rpq, w.xd[:N], cd[torch.from_numpy(w.assign[:N]).cuda()], w.rcodes)
    _WORLDS[name] = w
    return w


def flat(ra, w, rows, norms=True):
    from reductive_amd import qmatrix
    return qmatrix.QuantizedMatrix(w.pq, w.codes[rows].cpu().numpy(), w.norms[rows] if norms else None)


def partitioned(ra, w, rows, norms=True):
    from reductive_amd import qmatrix
    return qmatrix.PartitionedMatrix(flat(ra, w, rows, norms), w.centroids, w.assign[rows])


def residual(ra, w, rows, norms=True, codes=None, terms=None):
    import torch
    from reductive_amd import qmatrix
    codes = w.rcodes[rows] if codes is None else codes
    terms = w.rterms[rows] if terms is None else terms
    nd = torch.from_numpy(w.norms[rows]).cuda() if norms else None
    return qmatrix.ResidualPartitionedMatrix(w.rpq, codes, nd, terms, w.centroids, w.assign[rows])


def snapshot(m):
    names = [t for t in RESIDUAL_TENSORS + ("vectors",) if getattr(m, t, None) is not None]
    return {t: getattr(m, t).clone() for t in names}


def assert_unchanged(m, snap):
    import torch
    for t, v in snap.items():
        assert torch.equal(getattr(m, t), v), t


def assert_same_matrix(got, want, tensors):
    import torch
    assert type(got) is type(want) and len(got) == len(want)
    for t in tensors:
        g, w_ = getattr(got, t), getattr(want, t)
        assert (g is None) == (w_ is None), t
        if g is not None:
            assert g.dtype == w_.dtype and g.shape == w_.shape and g.is_contiguous(), t
            assert torch.equal(g.view(torch.uint8) if g.dtype.is_floating_point else g,
                               w_.view(torch.uint8) if g.dtype.is_floating_point else w_), t
    assert np.array_equal(got.centroids, want.centroids) and got.n_lists == want.n_lists


OLD = slice(0, N)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_assign_and_encode_match_the_oracle(ra, name):
    import torch
    w = world(ra, name)
    rm = residual(ra, w, OLD)
    snap = snapshot(rm)
    new = slice(N, N + B)
    for vectors in (w.xd[new], w.x[new]):                      # CUDA and numpy input
        got = rm.assign(vectors)
        assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (B,)
        assert np.array_equal(got.cpu().numpy(), w.assign[new])                                  # the oracle's
    assert np.array_equal(rm.assign(w.xd[new]).cpu().numpy(),
                          ra.cluster_assignments(w.centroids, w.x[new]).astype(np.int64))        # the library's host call
    assert tuple(rm.assign(w.xd[:0]).shape) == (0,)
    lists, codes, terms = rm.encode(w.xd[new])
    assert lists.dtype == torch.int64 and codes.dtype == torch.uint8 and terms.dtype == torch.float32
    assert np.array_equal(lists.cpu().numpy(), w.assign[new])
    resid = (w.x[new] - w.centroids[w.assign[new]]).astype(np.float32)
    rq = w.rpq.subquantizers()
    assert np.array_equal(codes.cpu().numpy(), orc.quantize_batch(rq, resid))
    r64 = orc.reconstruct_batch(rq, codes.cpu().numpy()).astype(np.float64)
    c64 = w.centroids[w.assign[new]].astype(np.float64)
    t64 = (r64 * r64 + 2.0 * c64 * r64).sum(1)
    t_abs = (r64 * r64 + np.abs(2.0 * c64 * r64)).sum(1)
    err = np.abs(terms.cpu().numpy().astype(np.float64) - t64)
    assert (err <= 2.0 ** -24 * np.abs(t64) + w.d * 2.0 ** -52 * t_abs).all(), err.max()
    # one vector, and numpy input, give the same rows
    l1, c1, t1 = rm.encode(w.x[N:N + 1])
    assert torch.equal(l1, lists[:1]) and torch.equal(c1, codes[:1]) and torch.equal(t1, terms[:1])
    assert_unchanged(rm, snap)


def grown_and_built(ra, w, cls, norms, b):
    """(the old matrix, m.add of b new vectors, the constructor over all N + b rows of the pieces)"""
    import torch
    rows = slice(0, N + b)
    xb = w.xd[N:N + b]
    nb = w.norms[N:N + b] if norms else None
    if cls == "partitioned":
        m = partitioned(ra, w, OLD, norms)
        return m, m.add(xb, nb), partitioned(ra, w, rows, norms)
    m = residual(ra, w, OLD, norms)
    lists, codes, terms = m.encode(xb)
    assert np.array_equal(lists.cpu().numpy(), w.assign[N:N + b])
    want = residual(ra, w, rows, norms, codes=torch.cat([w.rcodes, codes]), terms=torch.cat([w.rterms, terms]))
    return m, m.add(xb, nb), want


@pytest.mark.parametrize("cls", ["partitioned", "residual"])
@pytest.mark.parametrize("name,norms,b", [("base", True, 1), ("base", True, B), ("base", False, 1), ("base", False, B),
                                          ("lists300", True, B), ("wide", False, B)])
def test_add_equals_the_constructor_on_the_concatenation(ra, cls, name, norms, b):
    w = world(ra, name)
    tensors = LIST_TENSORS if cls == "partitioned" else RESIDUAL_TENSORS
    m, g, want = grown_and_built(ra, w, cls, norms, b)
    snap = snapshot(m)
    assert g is not m and len(g) == N + b and len(m) == N
    assert_same_matrix(g, want, tensors)
    assert g.vectors is None
    assert_unchanged(m, snap)


@pytest.mark.parametrize("cls", ["partitioned", "residual"])
def test_searches_of_the_grown_matrix(ra, cls):
    import torch
    w = world(ra, "base")
    m, g, want = grown_and_built(ra, w, cls, True, B)
    rng = np.random.default_rng(7100)
    q = w.xd[N + torch.from_numpy(rng.choice(B, 5, replace=False)).cuda()] * 1.01       # five queries beside new rows
    seen_new = 0
    for nprobe in (1, 3, w.n_lists):
        for fn, kw in (("nearest", {}), ("most_similar", {}), ("most_similar", {"use_norms": False})):
            v1, i1 = getattr(g, fn)(q, 50, nprobe, **kw)
            v2, i2 = getattr(want, fn)(q, 50, nprobe, **kw)
            assert torch.equal(i1, i2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)), (fn, nprobe)
            new = i1[i1 >= N]
            seen_new += int(new.numel())
            # a returned row number >= N addresses the new row of that number
            stored = g.codes[g.positions[new]]
            if cls == "partitioned":
                assert torch.equal(stored, w.codes[new])
            else:
                assert torch.equal(stored, m.encode(w.xd[new])[1])
            radius = v1[:, -1].contiguous()                     # the 50th value: a range that holds those 50 rows
            rfn = "within" if fn == "nearest" else "similar_above"
            r1 = getattr(g, rfn)(q, radius, nprobe, **kw)
            r2 = getattr(want, rfn)(q, radius, nprobe, **kw)
            for x1, x2 in zip(r1, r2):
                assert torch.equal(x1.view(torch.int32) if x1.dtype == torch.float32 else x1,
                                   x2.view(torch.int32) if x2.dtype == torch.float32 else x2), (rfn, nprobe)
            assert int(r1[0][-1]) >= 50 * 5 or nprobe < w.n_lists
    assert seen_new > 0


@pytest.mark.parametrize("cls", ["partitioned", "residual"])
def test_add_twice_extend_and_empty_batches(ra, cls):
    import torch
    w = world(ra, "base")
    tensors = LIST_TENSORS if cls == "partitioned" else RESIDUAL_TENSORS
    m, g, want = grown_and_built(ra, w, cls, True, B)
    cut = 1500
    snap = snapshot(m)
    g1 = m.add(w.xd[N:N + cut], w.norms[N:N + cut])
    g2 = g1.add(w.x[N + cut:N + B], torch.from_numpy(w.norms[N + cut:N + B]).cuda())         # numpy vectors, CUDA norms
    assert_same_matrix(g2, g, tensors)
    assert len(g1) == N + cut
    # B == 0: an equal new matrix
    e = m.add(w.xd[:0], w.norms[:0])
    assert e is not m
    assert_same_matrix(e, m, tensors)
    # extend: two matrices built separately over the same lists
    half = 14000
    build = partitioned if cls == "partitioned" else residual
    a, b = build(ra, w, slice(0, half)), build(ra, w, slice(half, N))
    sa, sb = snapshot(a), snapshot(b)
    assert_same_matrix(a.extend(b), m, tensors)
    assert_unchanged(a, sa)
    assert_unchanged(b, sb)
    assert_unchanged(m, snap)
    # what extend refuses
    other = partitioned(ra, w, OLD) if cls == "residual" else residual(ra, w, OLD)
    with pytest.raises(ra.PanicError, match="same class"):
        m.extend(other)
    with pytest.raises(ra.PanicError, match="norms"):
        m.extend(build(ra, w, slice(half, N), norms=False))
    w2 = world(ra, "lists300")
    with pytest.raises(ra.PanicError, match="centroids"):
        m.extend(build(ra, w2, slice(0, 5000)))
    # norms are required iff the matrix has them
    with pytest.raises(ra.PanicError, match="norms"):
        m.add(w.xd[N:N + 5])
    with pytest.raises(ra.PanicError, match="norms"):
        build(ra, w, OLD, norms=False).add(w.xd[N:N + 5], w.norms[N:N + 5])
    with pytest.raises(ra.PanicError, match="one norm per"):
        m.add(w.xd[N:N + 5], w.norms[N:N + 4])
    with pytest.raises(ra.PanicError):
        m.add(w.xd[N:N + 5, :-1], w.norms[N:N + 5])


@pytest.mark.parametrize("cls", ["flat", "partitioned", "residual"])
def test_attached_vectors_refine_and_row_filters(ra, cls):
    import torch
    w = world(ra, "base")
    build = {"flat": flat, "partitioned": partitioned, "residual": residual}[cls]
    m = build(ra, w, OLD).attach_vectors(w.xd[:N], torch.float16)
    g = m.add(w.xd[N:], w.norms[N:])
    assert g.vectors.dtype == torch.float16 and tuple(g.vectors.shape) == (N + B, w.d) and tuple(m.vectors.shape) == (N, w.d)
    assert torch.equal(g.vectors, w.xd.half())
    probe = () if cls == "flat" else (w.n_lists,)
    picks = torch.tensor([0, 7, 1234, B - 1], device="cuda")
    qs = w.xd[N + picks]
    dist, idx = g.nearest(qs, 10, *probe, refine=100)
    if cls == "residual":                                       # the matrix built in one go, all vectors attached
        _, codes, terms = m.encode(w.xd[N:])
        want = residual(ra, w, slice(0, N + B), codes=torch.cat([w.rcodes, codes]), terms=torch.cat([w.rterms, terms]))
    else:
        want = build(ra, w, slice(0, N + B))
    want.attach_vectors(w.xd, torch.float16)
    d2, i2 = want.nearest(qs, 10, *probe, refine=100)
    assert torch.equal(idx, i2) and torch.equal(dist, d2)
    # the exact stage reaches the new rows: with the old rows filtered out every candidate is a new row, and the
    # distances are those to the appended f16 vectors (f32 arithmetic in another summation order: 1e-4 relative)
    only_new = g.row_filter(rows=np.arange(N), allowed=False)
    assert only_new.n_allowed == B
    dist, idx = g.nearest(qs, 10, *probe, refine=100, allow=only_new)
    assert bool((idx >= N).all())
    exact = ((qs[:, None, :] - g.vectors[idx].float()) ** 2).sum(2)
    assert torch.allclose(dist, exact, rtol=1e-4, atol=1e-4)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    # a filter belongs to the matrix that built it
    old_filter = m.row_filter(np.ones(N, bool))
    with pytest.raises(ra.PanicError, match="another matrix"):
        g.nearest(w.xd[N:N + 2], 5, *probe, allow=old_filter)
    with pytest.raises(ra.PanicError, match="one flag per row"):
        g.row_filter(np.ones(N, bool))
    _, idx = g.nearest(w.xd[:3], 20, *probe, allow=only_new)
    assert bool((idx >= N).all())
    m.nearest(w.xd[:2], 5, *probe, allow=old_filter)            # and still serves the old matrix


def test_flat_add_equals_the_matrix_of_the_concatenated_codes(ra):
    import torch
    w = world(ra, "base")
    for norms in (True, False):
        m = flat(ra, w, OLD, norms)
        snap = snapshot(m)
        g = m.add(w.x[N:], w.norms[N:] if norms else None)
        want = flat(ra, w, slice(0, N + B), norms)
        assert g is not m and type(g) is type(m) and len(g) == N + B
        assert torch.equal(g.codes, want.codes) and g.codes.is_contiguous()
        assert (g.norms is None) == (not norms) and (not norms or torch.equal(g.norms, want.norms))
        assert g.vectors is None
        q = w.xd[N:N + 5]
        for a_, b_ in zip(g.nearest(q, 20) + g.most_similar(q, 20), want.nearest(q, 20) + want.most_similar(q, 20)):
            assert torch.equal(a_, b_)
        assert torch.equal(m.add(w.xd[:0], w.norms[:0] if norms else None).codes, m.codes)
        assert_unchanged(m, snap)
        with pytest.raises(ra.PanicError, match="norms"):
            m.add(w.x[N:], None if norms else w.norms[N:])
