"""The exact search through the matrix classes on the GPU: exact_nearest / exact_most_similar of the three quantized
classes against tests/flat_search_ref.py over their attached vectors, in original row numbers, with and without flags;
qmatrix.FlatMatrix (searches, filters, growth, compaction, lookups); FlatMatrix parts of a MatrixGroup (plain, with
refine= against rerank_ref.ref_rerank of the group's shortlist, two flat halves against the one flat matrix, the range
searches refused).  Shape: d = 32, M = 4, K = 16 over n = 3,000 rows drawn from 500 distinct vectors, so that equal exact
distances are common; 16 lists."""
import numpy as np
import pytest

import flat_search_ref as fr
import rerank_ref as rr
import synth

pytestmark = pytest.mark.gpu

N, D, M, BITS, LISTS = 3000, 32, 4, 4, 16
KS = (1, 10, 200)


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
    """One data set, computed once: vectors, a trained quantizer, the three quantized matrices with vectors attached
    (the partitioned ones f16), five queries near stored rows, flags, and the references everybody shares"""
    import torch
    from reductive_amd import qmatrix
    rng = np.random.default_rng(9300)
    w = type("World", (), {})()
    w.x = np.ascontiguousarray(synth.normalish(9301, (500, D)).astype(np.float32)[rng.integers(0, 500, N)])
    w.h = w.x.astype(np.float16)
    w.pq = ra.train_pq(M, BITS, 3, 1, w.x, rng=np.random.default_rng(9302))
    codes = w.pq.quantize_batch_device(torch.from_numpy(w.x).cuda()).cpu().numpy()
    w.qm = qmatrix.QuantizedMatrix(w.pq, codes).attach_vectors(w.x)
    w.pm = w.qm.partition(LISTS, n_iterations=2, vectors=w.x, rng=np.random.default_rng(9303)).attach_vectors(w.x, dtype=torch.float16)
    w.rm = w.qm.partition_residual(LISTS, n_iterations=2, pq_iterations=2, vectors=w.x,
                                   rng=np.random.default_rng(9304)).attach_vectors(w.x, dtype=torch.float16)
    w.qn = w.x[rng.choice(N, 5, replace=False)] * np.float32(1.01)
    w.q = torch.from_numpy(w.qn).cuda()
    w.flags = rng.random(N) < 0.3
    return w


def same_np(got, want_v, want_i):
    v, i = got
    assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
    fr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)


def same(got, want):
    import torch
    assert len(got) == len(want)
    for g, t in zip(got, want):
        assert g.dtype == t.dtype and g.shape == t.shape and g.device == t.device
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, t.view(torch.int32) if t.dtype == torch.float32 else t)


@pytest.mark.parametrize("which", ["qm", "pm", "rm"])
def test_exact_searches_of_the_quantized_classes(ra, w, which):
    import torch
    m = getattr(w, which)
    stored = w.x if which == "qm" else w.h
    for ip in (False, True):
        fn = m.exact_most_similar if ip else m.exact_nearest
        for k in KS:
            same_np(fn(w.q, k), *fr.ref_flat_search(w.qn, stored, k, ip=ip))
            same_np(fn(w.q, k, allow=w.flags), *fr.ref_flat_search(w.qn, stored, k, ip=ip, allow=w.flags))
        v, i = fn(w.qn[0], 7)                                             # one host query
        assert tuple(v.shape) == (7,)
        same_np((v[None], i[None]), *fr.ref_flat_search(w.qn[:1], stored, 7, ip=ip))
        same_np(fn(w.q, 10, allow=torch.from_numpy(w.flags).cuda()), *fr.ref_flat_search(w.qn, stored, 10, ip=ip, allow=w.flags))
    f = m.row_filter(w.flags)
    if which == "qm":
        same_np(m.exact_nearest(w.q, 10, allow=f), *fr.ref_flat_search(w.qn, stored, 10, allow=w.flags))
    else:
        with pytest.raises(ra.PanicError, match="position order"):
            m.exact_nearest(w.q, 10, allow=f)
    with pytest.raises(ra.PanicError, match="another matrix"):
        m.exact_nearest(w.q, 10, allow=w.qm.row_filter(w.flags) if which != "qm" else w.pm.row_filter(w.flags))
    with pytest.raises(ra.PanicError, match="one flag per row"):
        m.exact_nearest(w.q, 10, allow=w.flags[:-1])
    # the exact values are the values refine= returns
    kw = {} if which == "qm" else {"nprobe": LISTS}
    v, i = m.nearest(w.q, 10, refine=1024, **kw)
    for q in range(5):
        among = np.zeros(N, bool)
        among[i[q].cpu().numpy()] = True
        same((v[q], i[q]), m.exact_nearest(w.q[q], 10, allow=among))


def test_exact_search_needs_vectors(ra, w):
    from reductive_amd import qmatrix
    bare = qmatrix.QuantizedMatrix(w.pq, w.qm.codes.cpu().numpy())
    with pytest.raises(ra.PanicError, match="call attach_vectors first"):
        bare.exact_nearest(w.q, 3)
    with pytest.raises(ra.PanicError, match="call attach_vectors first"):
        bare.exact_most_similar(w.q, 3)


@pytest.mark.parametrize("half", [False, True])
def test_flat_matrix_searches_filters_and_lookups(ra, w, half):
    import torch
    stored = w.h if half else w.x
    fm = ra.FlatMatrix(stored)
    assert ra.qmatrix.FlatMatrix is ra.FlatMatrix and len(fm) == N and fm.pq.reconstructed_len() == D
    assert fm.vectors.dtype == (torch.float16 if half else torch.float32)
    f = fm.row_filter(w.flags)
    f_not = fm.row_filter(rows=np.flatnonzero(~w.flags), allowed=False)
    assert f.n_allowed == f_not.n_allowed == int(w.flags.sum())
    for ip in (False, True):
        fn = fm.most_similar if ip else fm.nearest
        for k in KS:
            want = fr.ref_flat_search(w.qn, stored, k, ip=ip)
            same_np(fn(w.q, k), *want)
            same_np(fn(w.q, k, refine=max(k, 300)), *want)                # accepted, equal to no refine
            want = fr.ref_flat_search(w.qn, stored, k, ip=ip, allow=w.flags)
            same_np(fn(w.q, k, allow=f), *want)
            same_np(fn(w.q, k, allow=f_not), *want)
            same_np(fn(w.q, k, allow=w.flags), *want)
    same(fm.most_similar(w.q, 10, use_norms=False), fm.most_similar(w.q, 10))
    with pytest.raises(ra.PanicError, match="between k and 1024"):
        fm.nearest(w.q, 10, refine=5)
    with pytest.raises(ra.PanicError, match="another matrix"):
        fm.nearest(w.q, 10, allow=w.qm.row_filter(w.flags))
    rows = np.array([5, 0, N - 1, 5])
    e = fm.embeddings(rows)
    assert e.dtype == torch.float32 and e.cpu().numpy().tobytes() == stored[rows].astype(np.float32).tobytes()
    with pytest.raises(ra.PanicError, match="row numbers must lie"):
        fm.embeddings([N])
    # a 16-bit request rounds f32 input once; the constructor refuses other dtypes and shapes
    assert ra.FlatMatrix(w.x, dtype=torch.float16).vectors.cpu().numpy().tobytes() == w.h.tobytes()
    with pytest.raises(ra.PanicError, match="float32 or float16"):
        ra.FlatMatrix(w.x, dtype=torch.float64)
    with pytest.raises(ra.PanicError, match=r"\[N, d\]"):
        ra.FlatMatrix(w.x[0])


@pytest.mark.parametrize("half", [False, True])
def test_flat_matrix_add_compact_remove(ra, w, half):
    import torch
    stored = w.h if half else w.x
    fm = ra.FlatMatrix(stored[:2000])
    grown = fm.add(w.x[2000:])
    assert len(fm) == 2000 and len(grown) == N and grown.vectors.dtype == fm.vectors.dtype
    assert grown.vectors.cpu().numpy().tobytes() == stored.tobytes()
    same(grown.nearest(w.q, 50), ra.FlatMatrix(stored).nearest(w.q, 50))
    new, kept = grown.compact(w.flags)
    assert kept.dtype == torch.int64 and kept.cpu().numpy().tolist() == np.flatnonzero(w.flags).tolist()
    assert new.vectors.dtype == fm.vectors.dtype and new.vectors.cpu().numpy().tobytes() == stored[w.flags].tobytes()
    built = ra.FlatMatrix(stored[w.flags])
    for ip in (False, True):
        same((new.most_similar if ip else new.nearest)(w.q, 50), (built.most_similar if ip else built.nearest)(w.q, 50))
    gone = np.flatnonzero(~w.flags)
    new2, kept2 = grown.remove(gone)
    assert torch.equal(kept2, kept) and torch.equal(new2.vectors, new.vectors)
    new3, kept3 = grown.compact(grown.row_filter(w.flags))
    assert torch.equal(kept3, kept) and torch.equal(new3.vectors, new.vectors)
    assert len(grown) == N                                                 # the old matrix stays as it is
    wide = ra.FlatMatrix(np.tile(w.x[:100], (1, 40)))                      # rows beyond 4,096 bytes
    nw, kw = wide.compact(w.flags[:100])
    assert nw.vectors.cpu().numpy().tobytes() == np.tile(w.x[:100], (1, 40))[w.flags[:100]].tobytes()


def test_group_of_two_flat_halves_is_the_one_flat_matrix(ra, w):
    whole = ra.FlatMatrix(w.x)
    g = ra.MatrixGroup([ra.FlatMatrix(w.x[:1100]), ra.FlatMatrix(w.x[1100:])])
    assert len(g) == N
    gf = g.row_filter(w.flags)
    for ip in (False, True):
        for k in KS:
            fn = (lambda m: m.most_similar) if ip else (lambda m: m.nearest)
            same(fn(g)(w.q, k), fn(whole)(w.q, k))
            same(fn(g)(w.q, k, allow=gf), fn(whole)(w.q, k, allow=w.flags))
            same(fn(g)(w.q, k, refine=300), fn(whole)(w.q, k))
    rows = np.array([0, 1099, 1100, N - 1, 7])
    assert g.embeddings(rows).cpu().numpy().tobytes() == w.x[rows].tobytes()
    part, local = g.locate(rows)
    assert part.tolist() == [0, 0, 1, 1, 0] and local.tolist() == [0, 1099, 0, N - 1101, 7]
    for call in (lambda: g.within(w.q, 1.0), lambda: g.similar_above(w.q, 1.0)):
        with pytest.raises(ra.PanicError, match="range search"):
            call()


def test_group_of_a_quantized_matrix_and_a_flat_delta(ra, w):
    """main index + fresh rows: the shortlist of refine=R is the R best of the group by (the main part's estimate, the
    delta's exact value), and the result is the exact re-ranking of that shortlist"""
    from reductive_amd import qmatrix
    cut, R = 2500, 100
    main = qmatrix.QuantizedMatrix(w.pq, w.qm.codes[:cut].cpu().numpy()).attach_vectors(w.x[:cut])
    delta = ra.FlatMatrix(w.x[cut:])
    g = ra.MatrixGroup([main, delta])
    with pytest.raises(ra.PanicError, match="range search"):
        g.within(w.q, 1.0)
    for ip in (False, True):
        fn = g.most_similar if ip else g.nearest
        _, short = fn(w.q, R)                                            # the group's shortlist
        ev, ei = (main.most_similar if ip else main.nearest)(w.q, R)
        fv, fi = (delta.most_similar if ip else delta.nearest)(w.q, R)
        # the plain search is the merge of the parts' results: estimate for the main part, exact for the delta
        vals = np.concatenate([ev.cpu().numpy(), fv.cpu().numpy()], 1)
        ids = np.concatenate([ei.cpu().numpy(), fi.cpu().numpy() + cut], 1)
        for q in range(5):
            key = -vals[q] if ip else vals[q]
            order = np.lexsort((np.arange(2 * R), key))[:R]              # ties to the earlier part, then its rank
            assert short[q].cpu().numpy().tolist() == ids[q][order].tolist()
        for k in (1, 10):
            want_v, want_i, flag = rr.ref_rerank(w.qn, w.x, short.cpu().numpy(), k, ip=ip)
            assert not flag
            same_np(fn(w.q, k, refine=R), want_v, want_i)
    rows = np.array([0, cut, N - 1])
    e = g.embeddings(rows).cpu().numpy()
    assert e[1:].tobytes() == w.x[rows[1:]].tobytes()
    assert e[0].tobytes() == main.embeddings([0]).cpu().numpy().tobytes()
