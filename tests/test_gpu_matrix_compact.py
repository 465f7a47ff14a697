"""Removing rows from the three matrix classes on the GPU (qmatrix: compact / remove).  The result is DEFINED by the
constructors: m.compact(allow)[0] equals, tensor for tensor, the constructor applied to the kept rows in their original
order, so every comparison here is torch.equal (on the bits) against a matrix built in one go from the codes, norms, row
terms and assignments this file keeps itself.  The consequence: every search of the new matrix is the filtered search
of the old one, bit for bit, indices mapped through `kept`, padding included.  Shape: N = 3,001, d = 24, M = 6, K = 16 (so
the 4-bit packed form is covered), 24 lists of which some are empty from the start and one is removed entirely."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

N, B, M, K, DSUB, LISTS = 3001, 257, 6, 16, 4, 24
D = M * DSUB
CLASSES = ("flat", "partitioned", "residual")
TENSORS = {"flat": ("codes", "norms", "vectors"),
           "partitioned": ("ids", "list_off", "positions", "codes", "norms", "vectors"),
           "residual": ("ids", "list_off", "positions", "codes", "norms", "row_terms", "lists", "vectors")}


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.fixture(scope="module")
def w(ra):
    """One data set, computed once: N old and B new vectors, both quantizers, centroids, assignments over 18 of the 24
    lists (the new rows get theirs from the library's assign(), as add() does), norms, flat codes, residual codes and row
    terms (the loop body of partition_residual), and the flags of the kept rows: about 60 %, one whole list removed."""
    import torch
    from reductive_amd import qmatrix
    rng = np.random.default_rng(8000)
    w = type("World", (), {})()
    w.pq = ra.Pq(None, synth.normalish(8001, (M, K, DSUB)))
    w.rpq = ra.Pq(None, synth.normalish(8002, (M, K, DSUB)) * np.float32(0.7))
    w.x = synth.normalish(8003, (N + B, D)).astype(np.float32)
    w.centroids = np.ascontiguousarray(w.x[rng.choice(N, LISTS, replace=False)])
    live = np.sort(rng.choice(LISTS, 18, replace=False))
    w.xd = torch.from_numpy(w.x).cuda()
    probe = qmatrix.PartitionedMatrix(qmatrix.QuantizedMatrix(w.pq, np.zeros((1, M), np.uint8)), w.centroids, np.zeros(1, np.int64))
    w.assign = np.concatenate([rng.choice(live, N), probe.assign(w.xd[N:]).cpu().numpy()]).astype(np.int64)
    w.norms = synth.uniform01(8004, (N + B,)) + np.float32(0.5)
    w.codes = w.pq.quantize_batch_device(w.xd)
    w.rcodes = torch.empty((N + B, M), dtype=torch.uint8, device="cuda")
    cd = torch.from_numpy(w.centroids).cuda()
    w.rterms = qmatrix._residual_codes_terms(w.rpq, w.xd, cd[torch.from_numpy(w.assign).cuda()], w.rcodes)
    # what add() stores for the new rows is what encode() gives for them as one batch
    old = qmatrix.ResidualPartitionedMatrix(w.rpq, w.rcodes[:N], None, w.rterms[:N], w.centroids, w.assign[:N])
    lists, w.rcodes[N:], w.rterms[N:] = old.encode(w.xd[N:])
    assert np.array_equal(lists.cpu().numpy(), w.assign[N:])
    w.flags = rng.random(N) < 0.6
    w.gone = int(live[3])
    w.flags[w.assign[:N] == w.gone] = False
    assert np.any(w.assign[:N] == w.gone) and len(set(w.assign[:N])) == 18
    w.q = w.xd[torch.from_numpy(rng.choice(N, 5, replace=False)).cuda()] * 1.01
    return w


def build(w, cls, rows, norms=True, packed=False, vectors=None):
    """the constructor of `cls` over the rows `rows` (world row numbers, in this order) of what the world keeps"""
    import torch
    from reductive_amd import qmatrix
    rows = np.asarray(rows, dtype=np.int64)
    rd = torch.from_numpy(rows).cuda()
    if cls == "residual":
        nd = torch.from_numpy(w.norms[rows]).cuda() if norms else None
        m = qmatrix.ResidualPartitionedMatrix(w.rpq, w.rcodes[rd], nd, w.rterms[rd], w.centroids, w.assign[rows])
    else:
        m = qmatrix.QuantizedMatrix(w.pq, w.codes[rd].cpu().numpy(), w.norms[rows] if norms else None)
        if cls == "partitioned":
            m = qmatrix.PartitionedMatrix(m, w.centroids, w.assign[rows])
    if packed:
        m = m.pack4()
    if vectors is not None:
        m.attach_vectors(w.x[rows], dtype=vectors)
    return m


def bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32) if t.dtype.is_floating_point else t


def assert_same_matrix(got, want, cls):
    import torch
    assert type(got) is type(want) and len(got) == len(want) and got.packed4 == want.packed4
    for t in TENSORS[cls]:
        g, w_ = getattr(got, t, None), getattr(want, t, None)
        assert (g is None) == (w_ is None), t
        if g is not None:
            assert g.dtype == w_.dtype and g.shape == w_.shape and g.is_contiguous(), t
            assert torch.equal(bits(g), bits(w_)), t
    if cls != "flat":
        assert np.array_equal(got.centroids, want.centroids) and got.n_lists == want.n_lists
        assert got.device_terms == want.device_terms


def snapshot(m, cls):
    return {t: getattr(m, t).clone() for t in TENSORS[cls] if getattr(m, t, None) is not None}


def assert_unchanged(m, snap):
    import torch
    for t, v in snap.items():
        assert torch.equal(bits(getattr(m, t)), bits(v)), t


def vector_dtypes():
    import torch
    return {"none": None, "f32": torch.float32, "f16": torch.float16}


@pytest.mark.parametrize("vectors", ["none", "f32", "f16"])
@pytest.mark.parametrize("norms", [True, False])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("cls", CLASSES)
def test_compact_equals_the_constructor_on_the_kept_rows(ra, w, cls, packed, norms, vectors):
    import torch
    vd = vector_dtypes()[vectors]
    m = build(w, cls, np.arange(N), norms, packed, vd)
    snap = snapshot(m, cls)
    kept_rows = np.flatnonzero(w.flags)
    want = build(w, cls, kept_rows, norms, packed, vd)
    for allow in (w.flags, torch.from_numpy(w.flags).cuda(), m.row_filter(w.flags)):
        new, kept = m.compact(allow)
        assert new is not m and kept.is_cuda and kept.dtype == torch.int64
        assert np.array_equal(kept.cpu().numpy(), kept_rows)
        assert_same_matrix(new, want, cls)
    if cls != "flat":
        l = w.gone
        assert int(new.list_off[l + 1] - new.list_off[l]) == 0 and int(m.list_off[l + 1] - m.list_off[l]) > 0
    assert_unchanged(m, snap)
    other = build(w, cls, np.arange(N), norms, packed, vd)
    with pytest.raises(ra.PanicError, match="another matrix"):
        m.compact(other.row_filter(w.flags))
    with pytest.raises(ra.PanicError):
        m.compact(w.flags[:-1])
    with pytest.raises(ra.PanicError):
        m.compact(None)


def mapped(idx, kept):
    """row numbers of the new matrix -> those of the old one; -1 stays"""
    import torch
    return torch.where(idx < 0, idx, kept[idx.clamp(min=0)])


def assert_same_result(got, want, kept, what):
    import torch
    for g, x in zip(got[:-1], want[:-1]):                   # (lims,) values
        assert torch.equal(bits(g), bits(x)), what
    assert torch.equal(mapped(got[-1], kept), want[-1]), what


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("cls", CLASSES)
def test_searches_equal_the_filtered_searches(ra, w, cls, packed):
    import torch
    m = build(w, cls, np.arange(N), True, packed, torch.float32)
    filt = m.row_filter(w.flags)
    new, kept = m.compact(filt)
    probes = [()] if cls == "flat" else [(1,), (3,), (LISTS,)]
    padded = False
    for pr in probes:
        for fn, kw in (("nearest", {}), ("most_similar", {}), ("most_similar", {"use_norms": False})):
            got = getattr(new, fn)(w.q, 300, *pr, **kw)
            want = getattr(m, fn)(w.q, 300, *pr, allow=filt, **kw)
            assert_same_result(got, want, kept, (fn, pr))
            padded |= bool((want[1] < 0).any())
        if not packed:
            radius = new.nearest(w.q, 40, *pr)[0][:, -1].contiguous()
            if bool(torch.isfinite(radius).all()):
                assert_same_result(new.within(w.q, radius, *pr), m.within(w.q, radius, *pr, allow=filt), kept, ("within", pr))
                lims = new.within(w.q, radius, *pr)[0]
                assert int(lims[-1]) >= 5 * 40
    assert padded == (cls != "flat")                        # one probed list holds fewer than 300 allowed rows
    # refine: the shortlist of the filtered search, re-ranked against the attached vectors
    for pr in probes[:2]:
        got = new.nearest(w.q, 10, *pr, refine=50)
        want = m.nearest(w.q, 10, *pr, refine=50, allow=filt)
        assert_same_result(got, want, kept, ("refine", pr))
    if not packed:
        rng = np.random.default_rng(8100)
        named = torch.from_numpy(np.sort(rng.choice(len(new), 400, replace=False))).cuda()
        assert_same_result(new.nearest_among(w.q, named, 20), m.nearest_among(w.q, kept[named], 20), kept, "among")


@pytest.mark.parametrize("cls", CLASSES)
def test_remove_nothing_out_of_range_and_after_add(ra, w, cls):
    import torch
    m = build(w, cls, np.arange(N), True, False, torch.float16)
    snap = snapshot(m, cls)
    same, kept = m.remove([])
    assert same is not m and np.array_equal(kept.cpu().numpy(), np.arange(N))
    assert_same_matrix(same, m, cls)
    for bad in ([N], [-1], np.array([0, 5, N + 7])):
        with pytest.raises(ra.PanicError, match="row numbers must lie in"):
            m.remove(bad)
    rng = np.random.default_rng(8200)
    r1 = rng.choice(N, 1200, replace=False)
    m1, k1 = m.remove(torch.from_numpy(r1).cuda())
    assert np.array_equal(k1.cpu().numpy(), np.setdiff1d(np.arange(N), r1))
    assert_same_matrix(m1, build(w, cls, k1.cpu().numpy(), True, False, torch.float16), cls)
    m2 = m1.add(w.xd[N:], w.norms[N:])
    rows2 = np.concatenate([k1.cpu().numpy(), np.arange(N, N + B)])
    r2 = rng.choice(len(m2), 700, replace=False)
    m3, k3 = m2.remove(r2)
    assert len(m3) == len(m2) - 700
    assert_same_matrix(m3, build(w, cls, rows2[k3.cpu().numpy()], True, False, torch.float16), cls)
    assert_unchanged(m, snap)
    # and the other order: everything added is removed again
    m4, k4 = m2.remove(np.arange(len(m1), len(m2)))
    assert_same_matrix(m4, m1, cls)


@pytest.mark.parametrize("cls", CLASSES)
def test_removing_every_row_is_the_constructor_on_no_rows(ra, w, cls):
    import torch
    m = build(w, cls, np.arange(N), True, False, torch.float32)
    try:
        want = build(w, cls, np.zeros(0, np.int64), True, False, torch.float32)
    except Exception as e:                                  # whatever the constructor raises, compact raises too
        with pytest.raises(type(e)):
            m.compact(np.zeros(N, bool))
        return
    new, kept = m.compact(np.zeros(N, bool))
    assert tuple(kept.shape) == (0,) and len(new) == 0
    assert_same_matrix(new, want, cls)
