"""GPU tests of qmatrix.PartitionedFlatMatrix (IVF-Flat over Pq.flat_search_lists_device) and FlatMatrix.partition:
with every list probed the values are FlatMatrix's bit for bit; a small nprobe equals the reference on the probed lists;
add / compact / remove equal the constructor tensor for tensor; allow= works through row_filter; as a part of a
MatrixGroup beside a QuantizedMatrix the class returns correct global rows."""
import numpy as np
import pytest

import flat_lists_ref as flr
import synth

pytestmark = pytest.mark.gpu

N, D, LISTS = 3000, 32, 12
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
    """One data set, computed once: distinct rows (no ties), the flat matrix, its partition, five queries, flags"""
    import torch
    rng = np.random.default_rng(9500)
    w = type("World", (), {})()
    centres = synth.normalish(9501, (40, D)).astype(np.float32)
    w.x = np.ascontiguousarray(centres[rng.integers(0, 40, N)] + np.float32(0.2) * rng.standard_normal((N, D)).astype(np.float32))
    w.h = w.x.astype(np.float16)
    w.fm = ra.FlatMatrix(w.x)
    w.pm = w.fm.partition(LISTS, n_iterations=3, rng=np.random.default_rng(9502))
    w.qn = w.x[rng.choice(N, 5, replace=False)] * np.float32(1.01)
    w.q = torch.from_numpy(w.qn).cuda()
    w.flags = rng.random(N) < 0.3
    return w


def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want):
    import torch
    assert len(got) == len(want)
    for g, t in zip(got, want):
        assert g.dtype == t.dtype and g.shape == t.shape and g.device == t.device
        assert torch.equal(bits(g), bits(t))


def same_matrix(a, b):
    """tensor for tensor: rows, ids, positions, list_off, centroids"""
    import torch
    for name in ("rows", "ids", "positions", "list_off"):
        g, t = getattr(a, name), getattr(b, name)
        assert g.dtype == t.dtype and g.shape == t.shape, name
        assert torch.equal(g.view(torch.int16) if g.dtype == torch.float16 else bits(g),
                           t.view(torch.int16) if t.dtype == torch.float16 else bits(t)), name
    assert np.array_equal(a.centroids, b.centroids) and a.n_lists == b.n_lists


def test_partition_layout_and_every_list_probed(ra, w):
    import torch
    pm = w.pm
    assert isinstance(pm, ra.PartitionedFlatMatrix) and len(pm) == N and pm.n_lists == LISTS
    assert pm.rows.dtype == torch.float32 and pm.centroids.shape == (LISTS, D)
    ids = pm.ids.cpu().numpy()
    off = pm.list_off.cpu().numpy()
    assert sorted(ids.tolist()) == list(range(N)) and off[0] == 0 and off[-1] == N and (np.diff(off) >= 0).all()
    assert pm.rows.cpu().numpy().tobytes() == w.x[ids].tobytes()
    assert np.array_equal(pm.positions.cpu().numpy()[ids], np.arange(N))
    assign = ra.cluster_assignments(pm.centroids, w.x)
    assert np.array_equal(np.repeat(np.arange(LISTS), np.diff(off)), np.asarray(assign)[ids])
    for l in range(LISTS):                           # inside a list the original row numbers ascend
        assert (np.diff(ids[off[l]:off[l + 1]]) > 0).all()
    assert torch.equal(pm.assign(w.x[:100]), torch.from_numpy(np.asarray(assign[:100], np.int64)).cuda())
    # the same draws from rng as QuantizedMatrix.partition with these vectors: the same centroids and layout
    from reductive_amd import qmatrix
    pq = ra.train_pq(4, 4, 2, 1, w.x, rng=np.random.default_rng(9503))
    qm = qmatrix.QuantizedMatrix(pq, pq.quantize_batch_device(torch.from_numpy(w.x).cuda()).cpu().numpy())
    qp = qm.partition(LISTS, n_iterations=3, vectors=w.x, rng=np.random.default_rng(9502), on_device=True)
    assert np.array_equal(qp.centroids, pm.centroids) and torch.equal(qp.ids, pm.ids) and torch.equal(qp.list_off, pm.list_off)
    for ip in (False, True):
        for k in KS:
            v, i = (pm.most_similar if ip else pm.nearest)(w.q, k, nprobe=LISTS)
            wv, wi = (w.fm.most_similar if ip else w.fm.nearest)(w.q, k)
            same((v, i), (wv, wi))                   # no ties in this data: the rows are the same too
            same((pm.most_similar if ip else pm.nearest)(w.q, k, nprobe=LISTS, refine=300), (wv, wi))
    v, i = pm.nearest(w.q[0], 7, nprobe=LISTS)
    assert tuple(v.shape) == (7,) and torch.equal(i, w.fm.nearest(w.q[0], 7)[1])
    with pytest.raises(ra.PanicError, match="refine must lie"):
        pm.nearest(w.q, 10, nprobe=2, refine=5)


@pytest.mark.parametrize("half", [False, True])
def test_small_nprobe_equals_the_reference_on_the_probed_lists(ra, w, half):
    import torch
    pm = w.fm.partition(LISTS, n_iterations=3, rng=np.random.default_rng(9502)) if not half else \
        ra.FlatMatrix(w.h).partition(LISTS, n_iterations=3, rng=np.random.default_rng(9502))
    assert pm.rows.dtype == (torch.float16 if half else torch.float32)
    rows, off, ids = pm.rows.cpu().numpy(), pm.list_off.cpu().numpy(), pm.ids.cpu().numpy()
    flags_pos = w.flags[ids]
    f = pm.row_filter(w.flags)
    assert f.n_allowed == int(w.flags.sum())
    for nprobe in (1, 3):
        pr = pm.probes(w.q, nprobe).cpu().numpy()
        assert pr.shape == (5, nprobe)
        for ip in (False, True):
            fn = pm.most_similar if ip else pm.nearest
            for k in (10, 200):
                want_v, want_p, flag = flr.ref_flat_search_lists(w.qn, rows, off, pr, k, ip=ip)
                assert not flag
                v, i = fn(w.q, k, nprobe=nprobe)
                flr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, np.where(want_p < 0, -1, ids[np.maximum(want_p, 0)]))
                want_v, want_p, _ = flr.ref_flat_search_lists(w.qn, rows, off, pr, k, ip=ip, allow=flags_pos)
                for allow in (f, w.flags):
                    v, i = fn(w.q, k, nprobe=nprobe, allow=allow)
                    flr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, np.where(want_p < 0, -1, ids[np.maximum(want_p, 0)]))
                    got = i.cpu().numpy()
                    assert w.flags[got[got >= 0]].all()
    with pytest.raises(ra.PanicError, match="another matrix"):
        pm.nearest(w.q, 5, nprobe=2, allow=w.pm.row_filter(w.flags) if pm is not w.pm else w.fm.row_filter(w.flags))
    e = pm.embeddings(np.array([0, N - 1, 17]))
    assert e.dtype == torch.float32 and e.cpu().numpy().tobytes() == (w.h if half else w.x)[[0, N - 1, 17]].astype(np.float32).tobytes()


@pytest.mark.parametrize("half", [False, True])
def test_add_compact_remove_equal_the_constructor(ra, w, half):
    import torch
    stored = w.h if half else w.x
    cen = w.pm.centroids
    assign = np.asarray(ra.cluster_assignments(cen, stored.astype(np.float32)), np.int64)
    whole = ra.PartitionedFlatMatrix(stored, cen, assign)
    assert whole.rows.dtype == (torch.float16 if half else torch.float32)
    # the device route of the constructor gives the same matrix
    same_matrix(ra.PartitionedFlatMatrix(stored, cen, torch.from_numpy(assign).cuda()), whole)
    part = ra.PartitionedFlatMatrix(stored[:2000], cen, assign[:2000])
    grown = part.add(stored[2000:])
    assert len(part) == 2000 and len(grown) == N
    same_matrix(grown, whole)
    same(grown.nearest(w.q, 50, nprobe=3), whole.nearest(w.q, 50, nprobe=3))
    same_matrix(part.add(stored[:0]), part)
    new, kept = whole.compact(w.flags)
    assert kept.dtype == torch.int64 and kept.cpu().numpy().tolist() == np.flatnonzero(w.flags).tolist()
    built = ra.PartitionedFlatMatrix(stored[w.flags], cen, assign[w.flags])
    same_matrix(new, built)
    for ip in (False, True):
        same((new.most_similar if ip else new.nearest)(w.q, 50, nprobe=4), (built.most_similar if ip else built.nearest)(w.q, 50, nprobe=4))
    new2, kept2 = whole.remove(np.flatnonzero(~w.flags))
    assert torch.equal(kept2, kept)
    same_matrix(new2, built)
    new3, kept3 = whole.compact(whole.row_filter(w.flags))
    assert torch.equal(kept3, kept)
    same_matrix(new3, built)
    assert len(whole) == N                                                 # the old matrix stays as it is
    with pytest.raises(ra.PanicError):
        ra.PartitionedFlatMatrix(stored, cen[:, :5], assign)
    with pytest.raises(ra.PanicError):
        ra.PartitionedFlatMatrix(stored, cen, assign[:10])


def test_rows_beyond_4096_bytes_take_the_torch_route(ra, w):
    wide = np.tile(w.x[:300], (1, 40))                                     # 1,280 f32 = 5,120 bytes
    cen = np.tile(w.pm.centroids, (1, 40))
    assign = np.asarray(ra.cluster_assignments(cen, wide), np.int64)
    whole = ra.PartitionedFlatMatrix(wide, cen, assign)
    same_matrix(ra.PartitionedFlatMatrix(wide[:200], cen, assign[:200]).add(wide[200:]), whole)
    new, kept = whole.compact(w.flags[:300])
    same_matrix(new, ra.PartitionedFlatMatrix(wide[w.flags[:300]], cen, assign[w.flags[:300]]))
    assert kept.cpu().numpy().tolist() == np.flatnonzero(w.flags[:300]).tolist()


def test_group_of_a_quantized_matrix_and_a_partitioned_flat_delta(ra, w):
    """global rows: the plain search is the merge of the main part's estimates and the delta's exact values over the
    probed lists; a range search raises as it does for a FlatMatrix part"""
    import torch
    from reductive_amd import qmatrix
    cut, R, nprobe = 1800, 100, 4
    pq = ra.train_pq(4, 4, 2, 1, w.x, rng=np.random.default_rng(9504))
    codes = pq.quantize_batch_device(torch.from_numpy(w.x[:cut]).cuda()).cpu().numpy()
    main = qmatrix.QuantizedMatrix(pq, codes).attach_vectors(w.x[:cut])
    delta = ra.FlatMatrix(w.x[cut:]).partition(6, n_iterations=2, rng=np.random.default_rng(9505))
    g = ra.MatrixGroup([main, delta])
    assert len(g) == N
    with pytest.raises(ra.PanicError, match="range search"):
        g.within(w.q, 1.0, nprobe=nprobe)
    with pytest.raises(ra.PanicError, match="needs nprobe"):
        g.nearest(w.q, 5)
    gf = g.row_filter(w.flags)
    for ip in (False, True):
        fn = g.most_similar if ip else g.nearest
        for allow, fa, fb in ((None, None, None), (gf, w.flags[:cut], w.flags[cut:])):
            _, got = fn(w.q, R, nprobe=nprobe, allow=allow)
            ev, ei = (main.most_similar if ip else main.nearest)(w.q, R, allow=fa)
            fv, fi = (delta.most_similar if ip else delta.nearest)(w.q, R, nprobe=nprobe, allow=fb)
            vals = np.concatenate([ev.cpu().numpy(), fv.cpu().numpy()], 1)
            fi = fi.cpu().numpy()
            ids = np.concatenate([ei.cpu().numpy(), np.where(fi < 0, -1, fi + cut)], 1)
            for q in range(5):
                key = -vals[q] if ip else vals[q]
                order = np.lexsort((np.arange(2 * R), key))[:R]          # ties to the earlier part, then its rank
                assert got[q].cpu().numpy().tolist() == ids[q][order].tolist()
        # refine: every part re-ranks its members of the shortlist exactly; the delta's values are its search values
        v, i = fn(w.q, 10, nprobe=nprobe, refine=R)
        i = i.cpu().numpy()
        assert (i >= 0).all() and (i < N).all()
        import rerank_ref as rr
        _, short = fn(w.q, R, nprobe=nprobe)
        want_v, want_i, flag = rr.ref_rerank(w.qn, w.x, short.cpu().numpy(), 10, ip=ip)
        assert not flag
        flr.assert_same(v.cpu().numpy(), i, want_v, want_i)
    rows = np.array([cut, N - 1, cut + 5])
    assert g.embeddings(rows).cpu().numpy().tobytes() == w.x[rows].tobytes()
