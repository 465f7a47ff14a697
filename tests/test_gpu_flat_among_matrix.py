"""GPU tests of the exact searches among given rows on the resident matrices (Pq.flat_among_device /
flat_range_among_device underneath): exact_nearest_among / exact_most_similar_among / exact_within_among /
exact_similar_above_among of the three quantized classes and nearest_among / most_similar_among / within_among /
similar_above_among of FlatMatrix and PartitionedFlatMatrix, each against the same class's masked exact search run query
by query, bit for bit, in original row numbers; and the one-liner the range form exists for: a radius query over the
codes verified against the stored vectors."""
import numpy as np
import pytest

import flat_among_ref as far
import flat_range_ref as frr
import synth

pytestmark = pytest.mark.gpu

N, D, LISTS, NQ, K = 2200, 24, 10, 5, 10
LENGTHS = (300, 0, 1100, 17, 2200)


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
    """One data set, computed once: clustered rows, the five classes over them, five queries with the reference values
    of every row, per-query candidate lists (ascending, distinct) with their flags"""
    import torch
    from reductive_amd import qmatrix
    rng = np.random.default_rng(9700)
    w = type("World", (), {})()
    centres = synth.normalish(9701, (30, D)).astype(np.float32)
    w.x = np.ascontiguousarray(centres[rng.integers(0, 30, N)] + np.float32(0.2) * rng.standard_normal((N, D)).astype(np.float32))
    w.x[1500] = w.x[7]                                # ties
    w.x[2100] = w.x[7]
    w.qn = (w.x[rng.choice(N, NQ, replace=False)] * np.float32(1.01)).astype(np.float32)
    w.qn[0] = w.x[7]
    w.q = torch.from_numpy(w.qn).cuda()
    parts = [np.sort(rng.permutation(N)[:m]).astype(np.int64) for m in LENGTHS]
    parts[0][:3] = (7, 1500, 2100)                    # the tied rows among the candidates of query 0 (ascending)
    parts[0] = np.unique(parts[0])
    w.lims = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    w.rows = np.concatenate(parts)
    w.flags = np.zeros((NQ, N), bool)
    for j, p in enumerate(parts):
        w.flags[j, p] = True
    w.values = {ip: frr.all_values(w.qn, w.x, ip) for ip in (False, True)}
    # about 60 rows of all per query, a different count each
    w.thr = {ip: np.array([np.sort(v[i])[::-1 if ip else 1][40 + 9 * i] for i in range(NQ)], np.float32)
             for ip, v in w.values.items()}
    w.fm = ra.FlatMatrix(w.x)
    w.pfm = w.fm.partition(LISTS, n_iterations=3, rng=np.random.default_rng(9702))
    w.pq = ra.train_pq(4, 4, 3, 1, w.x, rng=np.random.default_rng(9703))
    w.codes = w.pq.quantize_batch_device(torch.from_numpy(w.x).cuda())
    w.qm = qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy()).attach_vectors(w.x)
    w.pm = w.qm.partition(LISTS, n_iterations=3, vectors=w.x, rng=np.random.default_rng(9704))
    w.rm = w.qm.partition_residual(LISTS, n_iterations=3, pq_iterations=3, vectors=w.x, rng=np.random.default_rng(9704))
    for m in (w.pm, w.rm):
        m.attach_vectors(w.x)
    return w


def bits(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a, np.float32).view(np.uint32).tolist()


def cpu(got):
    return tuple(np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in got)


def assert_topk_rows(got, per_query):
    """got (val, idx) [nq, k] against one (val, idx) [k] per query, bit for bit"""
    for j, want in enumerate(per_query):
        assert cpu(got)[1][j].tolist() == cpu(want)[1].tolist(), j
        assert bits(got[0][j]) == bits(want[0]), j


def assert_csr_rows(got, per_query):
    """got (lims, val, idx) against one single-query CSR per query"""
    lims, val, idx = cpu(got)
    assert lims[0] == 0 and lims[-1] == val.size == idx.size
    for j, want in enumerate(per_query):
        wl, wv, wi = cpu(want)
        a = slice(lims[j], lims[j + 1])
        assert idx[a].tolist() == wi.tolist() and bits(val[a]) == bits(wv), j


@pytest.mark.parametrize("name", ["qm", "pm", "rm"])
def test_quantized_classes_exact_among_is_the_masked_exact_search(ra, w, name):
    import torch
    m = getattr(w, name)
    rows = (w.lims, w.rows)
    for ip in (False, True):
        top, exact = (m.exact_most_similar_among, m.exact_most_similar) if ip else (m.exact_nearest_among, m.exact_nearest)
        got = top(w.q, rows, K)
        assert tuple(got[0].shape) == (NQ, K) and got[1].dtype == torch.int64
        assert_topk_rows(got, [exact(w.q[j], K, allow=w.flags[j]) for j in range(NQ)])
        assert (cpu(got)[1][1] == -1).all() and cpu(got)[1][0].min() >= 0
        wv, wi, _ = far.ref_flat_among(w.qn, w.x, w.rows, K, lims=w.lims, ip=ip, values=w.values[ip])
        assert cpu(got)[1].tolist() == wi.tolist() and bits(got[0]) == bits(wv)             # original row numbers
        rng_among, rng_exact = (m.exact_similar_above_among, m.exact_similar_above) if ip else (m.exact_within_among, m.exact_within)
        thr = w.thr[ip]
        got = rng_among(w.q, rows, thr)
        assert_csr_rows(got, [rng_exact(w.q[j], float(thr[j]), allow=w.flags[j]) for j in range(NQ)])
        assert int(got[0][-1]) > 50
        srt = cpu(rng_among(w.q, rows, thr, sort=True))
        assert srt[0].tolist() == cpu(got)[0].tolist()
        for j in range(NQ):
            seg = srt[1][srt[0][j]:srt[0][j + 1]]
            assert (np.diff(seg) <= 0).all() if ip else (np.diff(seg) >= 0).all()
    # query 0 is row 7 itself, which ties with rows 1500 and 2100: ties to the smaller original row on every class
    assert cpu(m.exact_nearest_among(w.q, rows, K))[1][0][:3].tolist() == [7, 1500, 2100]
    # a shared vector of rows (numpy, on the host), a single 1-D query
    shared = w.rows[w.lims[2]:w.lims[3]]
    one = m.exact_nearest_among(w.q[2], shared, K)
    assert tuple(one[0].shape) == (K,)
    assert_topk_rows((one[0][None], one[1][None]), [m.exact_nearest(w.q[2], K, allow=w.flags[2])])
    allq = m.exact_nearest_among(w.q, torch.from_numpy(shared).cuda(), K)
    assert_topk_rows(allq, [m.exact_nearest(w.q[j], K, allow=w.flags[2]) for j in range(NQ)])
    r1 = m.exact_within_among(w.q[2], shared, float(w.thr[False][2]))
    assert tuple(r1[0].shape) == (2,)
    assert_csr_rows(r1, [m.exact_within(w.q[2], float(w.thr[False][2]), allow=w.flags[2])])


def test_exact_among_needs_the_vectors(ra, w):
    from reductive_amd import qmatrix
    bare = qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy())
    for call in (lambda: bare.exact_nearest_among(w.q, w.rows, K), lambda: bare.exact_most_similar_among(w.q, w.rows, K),
                 lambda: bare.exact_within_among(w.q, w.rows, 1.0), lambda: bare.exact_similar_above_among(w.q, w.rows, 1.0)):
        with pytest.raises(ra.PanicError, match="call attach_vectors first"):
            call()
    with pytest.raises(ra.PanicError, match="vector of integers"):
        w.qm.exact_nearest_among(w.q, w.rows[None], K)
    with pytest.raises(ra.PanicError, match="one offset per query"):
        w.qm.exact_nearest_among(w.q, (w.lims[:-1], w.rows), K)


def test_flat_matrix_among(ra, w):
    import torch
    rows = (torch.from_numpy(w.lims).cuda(), torch.from_numpy(w.rows).cuda())
    for ip in (False, True):
        top, search = (w.fm.most_similar_among, w.fm.most_similar) if ip else (w.fm.nearest_among, w.fm.nearest)
        got = top(w.q, rows, K)
        assert_topk_rows(got, [search(w.q[j], K, allow=w.flags[j]) for j in range(NQ)])
        assert_topk_rows(got, [(v, i) for v, i in zip(*(w.qm.exact_most_similar_among if ip else w.qm.exact_nearest_among)(w.q, rows, K))])
        rng_among, rng = (w.fm.similar_above_among, w.fm.similar_above) if ip else (w.fm.within_among, w.fm.within)
        got = rng_among(w.q, rows, w.thr[ip])
        assert_csr_rows(got, [rng(w.q[j], float(w.thr[ip][j]), allow=w.flags[j]) for j in range(NQ)])
        assert int(got[0][-1]) > 50
    # the order named: the rows of query 2 reversed come back reversed
    back = w.rows[w.lims[2]:w.lims[3]][::-1].copy()
    a = cpu(w.fm.within_among(w.q[2], w.rows[w.lims[2]:w.lims[3]], float(w.thr[False][2])))
    b = cpu(w.fm.within_among(w.q[2], back, float(w.thr[False][2])))
    assert a[2].size > 5 and b[2].tolist() == a[2][::-1].tolist() and bits(b[1]) == bits(a[1][::-1])


def test_partitioned_flat_matrix_among_in_original_rows(ra, w):
    pm = w.pfm
    assert pm.ids.cpu().numpy().tolist() != list(range(N))                  # the layout is a real permutation
    pos = pm.positions.cpu().numpy()
    rows = (w.lims, w.rows)
    for ip in (False, True):
        top, search = (pm.most_similar_among, pm.most_similar) if ip else (pm.nearest_among, pm.nearest)
        got = top(w.q, rows, K)
        # the same class's masked search over all lists: ties by position in both
        assert_topk_rows(got, [search(w.q[j], K, nprobe=LISTS, allow=w.flags[j]) for j in range(NQ)])
        # against FlatMatrix: the same values; the same rows where no value ties
        flat = (w.fm.most_similar_among if ip else w.fm.nearest_among)(w.q, rows, K)
        assert bits(got[0]) == bits(flat[0])
        assert cpu(got)[1][2:].tolist() == cpu(flat)[1][2:].tolist()
        thr = w.thr[ip]
        rng_among = pm.similar_above_among if ip else pm.within_among
        got = rng_among(w.q, rows, thr)
        want = far.ref_flat_range_among(w.qn, w.x, w.rows, thr, lims=w.lims, ip=ip, values=w.values[ip])
        lims, val, idx = cpu(got)
        assert lims.tolist() == want[0].tolist() and idx.tolist() == want[2].tolist() and bits(val) == bits(want[1])
    # ties go to the smaller POSITION: rows 7, 1500 and 2100 in the order of their positions
    tied = sorted((7, 1500, 2100), key=lambda r: pos[r])
    assert cpu(pm.nearest_among(w.q, rows, K))[1][0][:3].tolist() == tied
    # -1 is padding, a row out of range is skipped; both on the way to positions and back
    odd = np.array([7, -1, N + 5, 2100, -7, 3], np.int64)
    v, i = cpu(pm.nearest_among(w.q[0], odd, 6))
    assert sorted(i[:3].tolist()) == [3, 7, 2100] and i[3:].tolist() == [-1, -1, -1] and set(i[:2].tolist()) == {7, 2100}
    l, v, i = cpu(pm.within_among(w.q[0], odd, float("inf")))
    assert i.tolist() == [7, 2100, 3] and l.tolist() == [0, 3]
    import ctypes
    import torch
    from reductive_amd import _lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib().pqhip_check_codes_dev(pm.pq._cb(), 0, stream) == _lib.ECODE_RANGE     # raised, and lowered here


def test_a_radius_query_over_the_codes_is_verified_against_the_vectors(ra, w):
    """m.exact_within_among(q, m.within(q, r + slack)[::2], r): a subset of exact_within(q, r), and equal to it on the
    rows within() returned"""
    thr = w.thr[False]
    for m, kw in ((w.qm, {}), (w.pm, dict(nprobe=LISTS)), (w.rm, dict(nprobe=LISTS))):
        found = m.within(w.q, 2 * thr, **kw)
        got = cpu(m.exact_within_among(w.q, found[::2], thr))
        full = cpu(m.exact_within(w.q, thr))
        flims, _, fidx = cpu(found)
        assert 0 < got[0][-1] <= full[0][-1]
        for j in range(NQ):
            named = fidx[flims[j]:flims[j + 1]]
            a, b = slice(got[0][j], got[0][j + 1]), slice(full[0][j], full[0][j + 1])
            keep = np.isin(full[2][b], named)
            assert sorted(zip(got[2][a].tolist(), bits(got[1][a]))) == sorted(zip(full[2][b][keep].tolist(), bits(full[1][b][keep])))
            # in the order within() named them
            assert got[2][a].tolist() == [r for r in named.tolist() if r in set(full[2][b].tolist())]
    ipt = w.thr[True]
    found = w.qm.similar_above(w.q, ipt - np.abs(ipt) * np.float32(0.5))
    got = cpu(w.qm.exact_similar_above_among(w.q, found[::2], ipt))
    full = cpu(w.qm.exact_similar_above(w.q, ipt))
    assert 0 < got[0][-1] <= full[0][-1] and set(got[2].tolist()) <= set(full[2].tolist())
