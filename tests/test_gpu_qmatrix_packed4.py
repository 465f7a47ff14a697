"""The three matrix classes over 4-bit packed codes on the GPU (qmatrix: pack4 / unpack4).  A packed matrix is DEFINED
by its unpacked form: every search it serves returns, torch.equal, what the unpacked matrix returns -- values by their
bit patterns -- and m.pack4().add(x) is m.add(x).pack4() tensor for tensor.  Fixture: 3,000 + 400 vectors of 16 (M = 4)
or 15 (M = 5: three-byte rows) columns around 30 centres, 4-bit quantizers trained for three iterations, 16 lists."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

N, B, N_LISTS = 3000, 400, 16
LIST_TENSORS = ("ids", "list_off", "positions", "codes", "norms")
TENSORS = {"flat": ("codes", "norms"), "lists": LIST_TENSORS, "residual": LIST_TENSORS + ("row_terms", "lists")}
KINDS = ("flat", "lists", "residual")


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


_WORLDS = {}


def world(ra, M):
    """the data, the trained quantizer and the three unpacked matrices over the first N vectors, built once per M"""
    from reductive_amd import qmatrix
    if M in _WORLDS:
        return _WORLDS[M]
    d = 16 if M == 4 else 15
    w = type("World", (), {})()
    w.M, w.d = M, d
    centres = synth.normalish(8100 + M, (30, d)) * np.float32(3.0)
    w.x = (centres[np.random.default_rng(8101 + M).integers(0, 30, N + B)] + synth.normalish(8102 + M, (N + B, d))).astype(np.float32)
    w.norms = synth.uniform01(8103 + M, (N + B,)) + np.float32(0.5)
    w.queries = (centres[:9] + synth.normalish(8104 + M, (9, d))).astype(np.float32)
    w.pq = ra.train_pq(M, 4, 3, 1, w.x[:N], rng=np.random.default_rng(8105 + M))
    assert w.pq.n_quantizer_centroids() == 16
    codes = w.pq.quantize_batch(w.x[:N])
    flat = qmatrix.QuantizedMatrix(w.pq, codes, w.norms[:N])
    w.m = {"flat": flat,
           "lists": flat.partition(N_LISTS, n_iterations=3, vectors=w.x[:N], rng=np.random.default_rng(8106)),
           "residual": flat.partition_residual(N_LISTS, n_iterations=3, pq_iterations=3, vectors=w.x[:N],
                                               rng=np.random.default_rng(8107))}
    assert w.m["residual"].pq.n_quantizer_centroids() == 16
    for m in w.m.values():
        m.attach_vectors(w.x[:N])
    _WORLDS[M] = w
    return w


def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_equal_results(got, want):
    import torch
    for g, w_ in zip(got, want):
        assert g.dtype == w_.dtype and g.shape == w_.shape and torch.equal(bits(g), bits(w_))


def assert_same_tensors(got, want, names):
    import torch
    assert type(got) is type(want) and len(got) == len(want) and got.packed4 == want.packed4
    for t in names:
        g, w_ = getattr(got, t), getattr(want, t)
        assert (g is None) == (w_ is None), t
        if g is not None:
            assert g.dtype == w_.dtype and g.shape == w_.shape and torch.equal(bits(g), bits(w_)), t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (4, 5))
def test_pack4_and_unpack4(ra, M, kind):
    import torch
    w = world(ra, M)
    m = w.m[kind]
    p = m.pack4()
    assert type(p) is type(m) and p is not m and p.packed4 is True and m.packed4 is False
    assert p.codes.dtype == torch.uint8 and tuple(p.codes.shape) == (N, (M + 1) // 2) and len(p) == N
    assert np.array_equal(p.codes.cpu().numpy(), ra.pack_codes4(m.codes.cpu().numpy()))
    for name in TENSORS[kind] + ("vectors",):
        if name != "codes":
            assert getattr(p, name) is getattr(m, name), name          # shared, not copied
    assert p.pq is m.pq and p.pack4() is p and m.unpack4() is m
    u = p.unpack4()
    assert u is not p and u.packed4 is False
    assert_same_tensors(u, m, TENSORS[kind])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (4, 5))
def test_searches_on_a_packed_matrix_equal_the_unpacked_ones(ra, M, kind):
    import torch
    w = world(ra, M)
    m = w.m[kind]
    p = m.pack4()
    flags = np.random.default_rng(8200 + M).random(N) < 0.5
    q_all = torch.from_numpy(w.queries).cuda()
    probes = ({},) if kind == "flat" else ({"nprobe": 1}, {"nprobe": 4}, {"nprobe": N_LISTS})
    ra.launch_log(reset=True)
    for q in (q_all, q_all[0]):
        for kw in probes:
            for refine in (None, 50):
                for allow_m, allow_p in ((None, None), (flags, flags), (m.row_filter(flags), p.row_filter(flags)),
                                         (m.row_filter(rows=[5, 77], allowed=False), p.row_filter(rows=[5, 77], allowed=False))):
                    assert_equal_results(p.nearest(q, 10, refine=refine, allow=allow_p, **kw),
                                         m.nearest(q, 10, refine=refine, allow=allow_m, **kw))
                    for use_norms in (True, False):
                        assert_equal_results(p.most_similar(q, 10, use_norms=use_norms, refine=refine, allow=allow_p, **kw),
                                             m.most_similar(q, 10, use_norms=use_norms, refine=refine, allow=allow_m, **kw))
    assert "_p4" in ra.launch_log(reset=True)
    with pytest.raises(ra.PanicError):                                  # a filter belongs to the matrix it was built for
        p.nearest(q_all, 5, allow=m.row_filter(flags), **probes[0])
    with pytest.raises(ra.PanicError):
        m.nearest(q_all, 5, allow=p.row_filter(flags), **probes[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (4, 5))
def test_embeddings_and_the_rest_of_the_surface(ra, M, kind):
    import torch
    w = world(ra, M)
    m = w.m[kind]
    p = m.pack4()
    rows = np.concatenate([np.random.default_rng(8300).integers(0, N, 300), [0, N - 1, 7, 7]])
    assert_equal_results([p.embeddings(rows)], [m.embeddings(rows)])
    assert tuple(p.embeddings([]).shape) == (0, w.d)
    if kind != "flat":
        q = torch.from_numpy(w.queries).cuda()
        assert torch.equal(p.probes(q, 3), m.probes(q, 3))
        assert torch.equal(p.assign(w.x[N:N + 50]), m.assign(w.x[N:N + 50]))
    if kind == "residual":
        assert_equal_results(p.encode(w.x[N:N + 50]), m.encode(w.x[N:N + 50]))     # (lists, unpacked codes, row terms)
    # what a packed matrix does not serve names the way out
    q1 = torch.from_numpy(w.queries[0]).cuda()
    extra = {} if kind == "flat" else {"nprobe": 2}
    calls = [lambda: p.within(q1, 1.0, **extra), lambda: p.similar_above(q1, 1.0, **extra)]
    if kind == "flat":
        calls += [lambda: p.distances(q1), lambda: p.inner_products(q1), lambda: p.partition(4),
                  lambda: p.partition_residual(4)]
    for call in calls:
        with pytest.raises(ra.PanicError, match=r"unpack4\(\)"):
            call()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (4, 5))
def test_growth_of_a_packed_matrix(ra, M, kind):
    import torch
    w = world(ra, M)
    m = w.m[kind]
    xb, nb = w.x[N:], w.norms[N:]
    want = m.add(xb, norms=nb).pack4()
    got = m.pack4().add(xb, norms=nb)
    assert got.packed4 is True and len(got) == N + B and tuple(got.codes.shape) == (N + B, (M + 1) // 2)
    assert_same_tensors(got, want, TENSORS[kind] + ("vectors",))
    q = torch.from_numpy(w.queries).cuda()
    extra = {} if kind == "flat" else {"nprobe": 4}
    assert_equal_results(got.nearest(q, 10, **extra), m.add(xb, norms=nb).nearest(q, 10, **extra))
    assert_equal_results(got.most_similar(q, 10, **extra), want.most_similar(q, 10, **extra))
    if kind != "flat":
        piece = m.add(xb[:1], norms=nb[:1])
        with pytest.raises(ra.PanicError, match="pack4"):
            m.pack4().extend(piece)
        with pytest.raises(ra.PanicError, match="pack4"):
            m.extend(piece.pack4())
        assert_same_tensors(m.pack4().extend(m.pack4()), m.extend(m).pack4(), TENSORS[kind])
