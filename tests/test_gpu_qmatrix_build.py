"""Building partitioned matrices on the device (qmatrix: the constructors with a CUDA assignment, partition(on_device=True),
partition_residual(on_device=True), device_terms).  What equals what: the device route gives, tensor for tensor, the
matrices of the host route -- except the row terms of a residual matrix, which are DEFINED by
pqhip_residual_terms_f32_dev (tests/residual_terms_ref.py) and compared with that reference exactly.  Worlds as in
tests/test_gpu_qmatrix_add.py (the recipe is copied): M = 15, K = 256, dsub = 4, N = 30,011 rows in 24 and in 300 lists."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc
from residual_terms_ref import ref_terms

pytestmark = pytest.mark.gpu

N = 30011
CONFIGS = {"base": (15, 4, 24), "lists300": (15, 4, 300)}       # M, dsub, n_lists (K = 256)
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
    """One data set per configuration, computed once: N vectors around 40 centres, the quantizer of the vectors, a
    residual quantizer (and the same one behind a rotation), centroids (n_lists distinct rows), the oracle's assignments,
    norms, the flat codes and -- through the host route's helper -- the residual codes and row terms."""
    import torch
    from reductive_amd import qmatrix
    if name in _WORLDS:
        return _WORLDS[name]
    M, dsub, n_lists = CONFIGS[name]
    d, seed = M * dsub, 7000 + 10 * sorted(CONFIGS).index(name)
    w = type("World", (), {})()
    w.M, w.d, w.n_lists = M, d, n_lists
    w.pq = ra.Pq(None, synth.normalish(seed, (M, 256, dsub)))
    w.rq = synth.normalish(seed + 1, (M, 256, dsub)) * np.float32(0.7)
    w.rpq = ra.Pq(None, w.rq)
    P = np.linalg.qr(synth.normalish(seed + 7, (d, d)).astype(np.float64))[0].astype(np.float32)
    w.ropq = ra.Pq(P, w.rq)
    centres = synth.normalish(seed + 2, (40, d)) * np.float32(3.0)
    w.x = (centres[np.random.default_rng(seed + 3).integers(0, 40, N)] + synth.normalish(seed + 4, (N, d))).astype(np.float32)
    w.centroids = np.ascontiguousarray(w.x[np.random.default_rng(seed + 5).choice(N, n_lists, replace=False)])
    w.assign = orc.cluster_assignments(w.centroids, w.x).astype(np.int64)
    w.norms = synth.uniform01(seed + 6, (N,)) + np.float32(0.5)
    w.xd = torch.from_numpy(w.x).cuda()
    w.ad = torch.from_numpy(w.assign).cuda()
    w.codes = w.pq.quantize_batch_device(w.xd)
    cd = torch.from_numpy(w.centroids).cuda()
    w.rcodes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    w.rterms = qmatrix._residual_codes_terms(w.rpq, w.xd, cd[w.ad], w.rcodes)
    _WORLDS[name] = w
    return w


def flat(w, norms=True):
    from reductive_amd import qmatrix
    return qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy(), w.norms if norms else None)


def assert_same_matrix(got, want, tensors):
    import torch
    assert type(got) is type(want) and len(got) == len(want)
    for t in tensors:
        g, w_ = getattr(got, t), getattr(want, t)
        assert (g is None) == (w_ is None), t
        if g is not None:
            assert g.dtype == w_.dtype and g.shape == w_.shape and g.is_contiguous() and g.device == w_.device, t
            assert torch.equal(g.view(torch.uint8) if g.dtype.is_floating_point else g,
                               w_.view(torch.uint8) if g.dtype.is_floating_point else w_), t
    assert np.array_equal(got.centroids, want.centroids) and got.n_lists == want.n_lists
    assert got.pq == want.pq and got.coarse == want.coarse


def reference_terms(m):
    """the row terms tests/residual_terms_ref.py defines for what the matrix stores, in list order"""
    return ref_terms(m.pq.subquantizers(), m.codes.cpu().numpy(), m.lists.cpu().numpy(), m.centroids)


@pytest.mark.parametrize("norms", [True, False])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_constructors_with_a_device_assignment(ra, name, norms):
    import torch
    from reductive_amd import qmatrix
    w = world(ra, name)
    qm = flat(w, norms)
    assert_same_matrix(qmatrix.PartitionedMatrix(qm, w.centroids, w.ad), qmatrix.PartitionedMatrix(qm, w.centroids, w.assign),
                       LIST_TENSORS)
    nd = torch.from_numpy(w.norms).cuda() if norms else None
    got = qmatrix.ResidualPartitionedMatrix(w.rpq, w.rcodes, nd, w.rterms, w.centroids, w.ad)
    want = qmatrix.ResidualPartitionedMatrix(w.rpq, w.rcodes, nd, w.rterms, w.centroids, w.assign)
    assert_same_matrix(got, want, RESIDUAL_TENSORS)
    assert got.device_terms is False
    # what the device constructor refuses: a wrong length, a wrong dtype, an id outside the lists
    with pytest.raises(ra.PanicError, match="one list id per row"):
        qmatrix.PartitionedMatrix(qm, w.centroids, w.ad[:-1])
    with pytest.raises(ra.PanicError, match="int64 CUDA tensor"):
        qmatrix.PartitionedMatrix(qm, w.centroids, w.ad.int())
    bad = w.ad.clone()
    bad[N // 2] = w.n_lists
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        qmatrix.PartitionedMatrix(qm, w.centroids, bad)


@pytest.mark.parametrize("how", ["vectors", "reconstructions", "train_rows"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_partition_on_the_device_equals_the_host_route(ra, name, how):
    import torch
    w = world(ra, name)
    qm = flat(w)
    kw = {"vectors": dict(vectors=w.xd), "reconstructions": dict(), "train_rows": dict(vectors=w.x, train_rows=5000)}[how]
    want = qm.partition(w.n_lists, n_iterations=3, rng=np.random.default_rng(71), **kw)
    ra.launch_log(reset=True)
    got = qm.partition(w.n_lists, n_iterations=3, rng=np.random.default_rng(71), on_device=True, **kw)
    assert "k_layout_place" in ra.launch_log(reset=True)
    assert_same_matrix(got, want, LIST_TENSORS)
    if name == "base" and how == "vectors":                    # the searches of the two are the same searches
        q = w.xd[torch.tensor([5, 777, 20000], device="cuda")] * 1.01
        for nprobe in (1, 5, w.n_lists):
            for a, b in zip(got.nearest(q, 40, nprobe) + got.most_similar(q, 40, nprobe),
                            want.nearest(q, 40, nprobe) + want.most_similar(q, 40, nprobe)):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b)
            radius = got.nearest(q, 40, nprobe)[0][:, -1].contiguous()
            for a, b in zip(got.within(q, radius, nprobe), want.within(q, radius, nprobe)):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_partition_residual_on_the_device(ra, name):
    import torch
    w = world(ra, name)
    qm = flat(w)
    kw = dict(n_iterations=3, vectors=w.xd)
    want = qm.partition_residual(w.n_lists, residual_pq=w.rpq, rng=np.random.default_rng(72), **kw)
    ra.launch_log(reset=True)
    got = qm.partition_residual(w.n_lists, residual_pq=w.rpq, rng=np.random.default_rng(72), on_device=True, **kw)
    log = ra.launch_log(reset=True)
    assert "k_residuals" in log and "k_residual_terms" in log and "k_layout_place" in log
    assert got.device_terms is True and want.device_terms is False
    assert_same_matrix(got, want, LIST_TENSORS + ("lists",))
    assert got.row_terms.dtype == torch.float32 and got.row_terms.is_contiguous()
    assert got.row_terms.cpu().numpy().tobytes() == reference_terms(got).tobytes()
    # with an OPQ residual quantizer the torch tail is kept: the whole matrix is the host route's
    want = qm.partition_residual(w.n_lists, residual_pq=w.ropq, rng=np.random.default_rng(73), **kw)
    got = qm.partition_residual(w.n_lists, residual_pq=w.ropq, rng=np.random.default_rng(73), on_device=True, **kw)
    assert_same_matrix(got, want, RESIDUAL_TENSORS)


def test_partition_residual_with_training_on_the_device(ra):
    w = world(ra, "base")
    qm = flat(w, norms=False)
    kw = dict(n_subquantizers=5, n_subquantizer_bits=4, n_iterations=3, pq_iterations=2, train_rows=4000)
    want = qm.partition_residual(w.n_lists, rng=np.random.default_rng(74), **kw)
    got = qm.partition_residual(w.n_lists, rng=np.random.default_rng(74), on_device=True, **kw)
    assert got.pq == want.pq and got.pq.quantized_len() == 5 and got.pq.n_quantizer_centroids() == 16
    assert_same_matrix(got, want, LIST_TENSORS + ("lists",))
    assert got.row_terms.cpu().numpy().tobytes() == reference_terms(got).tobytes()


def test_no_array_of_length_n_takes_the_host_route(ra, monkeypatch):
    from reductive_amd import pq as pq_mod
    from reductive_amd import qmatrix
    w = world(ra, "base")
    qm = flat(w)
    want_p = qm.partition(w.n_lists, n_iterations=2, rng=np.random.default_rng(75))
    want_r = qm.partition_residual(w.n_lists, n_iterations=2, residual_pq=w.rpq, rng=np.random.default_rng(75))

    def refuse(*a, **k):
        raise AssertionError("the host route was taken")

    monkeypatch.setattr(qmatrix, "ivf_layout", refuse)
    monkeypatch.setattr(pq_mod, "cluster_assignments", refuse)
    with pytest.raises(AssertionError, match="host route"):
        qm.partition(w.n_lists, n_iterations=2, rng=np.random.default_rng(75))
    got_p = qm.partition(w.n_lists, n_iterations=2, rng=np.random.default_rng(75), on_device=True)
    got_r = qm.partition_residual(w.n_lists, n_iterations=2, residual_pq=w.rpq, rng=np.random.default_rng(75), on_device=True)
    assert_same_matrix(got_p, want_p, LIST_TENSORS)
    assert_same_matrix(got_r, want_r, LIST_TENSORS + ("lists",))


def test_growth_of_a_device_built_residual_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    w = world(ra, "base")
    cut = 26000
    cd = torch.from_numpy(w.centroids).cuda()
    nd = torch.from_numpy(w.norms).cuda()
    # the device-route constructor applied to rows [0, n): codes of the f32 residuals, terms from the kernel
    terms = w.rpq.residual_terms_device(w.rcodes, w.ad, cd)

    def built(rows, device_terms=True):
        m = qmatrix.ResidualPartitionedMatrix(w.rpq, w.rcodes[rows], nd[rows], terms[rows] if device_terms else w.rterms[rows],
                                              w.centroids, w.ad[rows])
        m.device_terms = device_terms
        return m

    m = built(slice(0, cut))
    lists, codes, t = m.encode(w.xd[cut:])
    assert torch.equal(lists, w.ad[cut:]) and torch.equal(codes, w.rcodes[cut:])
    assert torch.equal(t.view(torch.int32), terms[cut:].view(torch.int32))
    g = m.add(w.xd[cut:], w.norms[cut:])
    assert g.device_terms is True
    assert_same_matrix(g, built(slice(0, N)), RESIDUAL_TENSORS)
    assert g.row_terms.cpu().numpy().tobytes() == reference_terms(g).tobytes()
    assert_same_matrix(m.add(w.xd[:0], w.norms[:0]), m, RESIDUAL_TENSORS)
    # pack4 / unpack4 and extend hand the route on; matrices of different routes do not merge
    assert_same_matrix(m.extend(built(slice(cut, N))), g, RESIDUAL_TENSORS)
    assert m.extend(built(slice(cut, N))).device_terms is True
    small = qmatrix.ResidualPartitionedMatrix(ra.Pq(None, w.rq[:, :16]), w.rcodes[:100] & 15, None, terms[:100], w.centroids, w.ad[:100])
    small.device_terms = True
    assert small.pack4().device_terms is True and small.pack4().unpack4().device_terms is True
    with pytest.raises(ra.PanicError, match="device_terms"):
        m.extend(built(slice(cut, N), device_terms=False))
    with pytest.raises(ra.PanicError, match="device_terms"):
        built(slice(cut, N), device_terms=False).extend(m)
