"""GPU tests of the exact range searches on the resident matrices: FlatMatrix.within / similar_above and
PartitionedFlatMatrix.within / similar_above (Pq.flat_range_device / flat_range_lists_device) against
tests/flat_range_ref.py, and exact_within / exact_similar_above of the three quantized classes, which must return
FlatMatrix's result in original row numbers."""
import numpy as np
import pytest

import flat_range_ref as frr
import synth

pytestmark = pytest.mark.gpu

N, D, LISTS, NQ = 2200, 24, 10, 5


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
    """One data set, computed once: clustered rows, the flat matrix, its partition, the quantized matrix with the vectors
    attached, five queries with the reference values of every row, flags"""
    import torch
    from reductive_amd import qmatrix
    rng = np.random.default_rng(9600)
    w = type("World", (), {})()
    centres = synth.normalish(9601, (30, D)).astype(np.float32)
    w.x = np.ascontiguousarray(centres[rng.integers(0, 30, N)] + np.float32(0.2) * rng.standard_normal((N, D)).astype(np.float32))
    w.x[1500] = w.x[7]                                # ties
    w.x[2100] = w.x[7]
    w.h = w.x.astype(np.float16)
    w.fm = ra.FlatMatrix(w.x)
    w.fh = ra.FlatMatrix(w.h)
    w.pm = w.fm.partition(LISTS, n_iterations=3, rng=np.random.default_rng(9602))
    w.qn = (w.x[rng.choice(N, NQ, replace=False)] * np.float32(1.01)).astype(np.float32)
    w.qn[0] = w.x[7]
    w.q = torch.from_numpy(w.qn).cuda()
    w.flags = rng.random(N) < 0.3
    w.values = {(ip, half): frr.all_values(w.qn, w.h if half else w.x, ip) for ip in (False, True) for half in (False, True)}
    # about 60 rows per query, a different count each
    w.thr = {key: np.array([np.sort(v[i])[::-1 if key[0] else 1][40 + 9 * i] for i in range(NQ)], np.float32)
             for key, v in w.values.items()}
    w.pq = ra.train_pq(4, 4, 3, 1, w.x, rng=np.random.default_rng(9603))
    w.codes = w.pq.quantize_batch_device(torch.from_numpy(w.x).cuda())
    w.qm = qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy()).attach_vectors(w.x)
    return w


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def cpu(got):
    return tuple(t.cpu().numpy() for t in got)


def same(got, want):
    """CSR against CSR (numpy or torch): lims and idx equal, val bit for bit"""
    g = cpu(got) if hasattr(got[0], "cpu") else got
    t = cpu(want) if hasattr(want[0], "cpu") else want
    assert g[0].tolist() == t[0].tolist() and g[2].tolist() == t[2].tolist() and bits(g[1]) == bits(t[1])


def same_up_to_ties(got, want):
    """two sorted CSR results: the same values in the same order, and per query the same (value, row) pairs"""
    g, t = cpu(got), cpu(want)
    assert g[0].tolist() == t[0].tolist() and bits(g[1]) == bits(t[1])
    for i in range(g[0].size - 1):
        a, b = slice(g[0][i], g[0][i + 1]), slice(t[0][i], t[0][i + 1])
        assert sorted(zip(bits(g[1][a]), g[2][a].tolist())) == sorted(zip(bits(t[1][b]), t[2][b].tolist()))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_flat_matrix_range_against_the_reference(ra, w, ip, half):
    import torch
    from reductive_amd import qmatrix
    fm, x = (w.fh, w.h) if half else (w.fm, w.x)
    thr, values = w.thr[ip, half], w.values[ip, half]
    fn = fm.similar_above if ip else fm.within
    want = frr.ref_flat_range(w.qn, x, thr, ip=ip, values=values)
    assert (np.diff(want[0]) >= 40).all() and len(set(np.diff(want[0]).tolist())) == NQ
    got = fn(w.q, thr)
    same(got, want)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
    same(fn(w.qn, torch.from_numpy(thr).cuda()), want)                      # host queries, device thresholds
    same(fn(w.q, float(thr[2])), frr.ref_flat_range(w.qn, x, thr[2], ip=ip, values=values))        # a scalar for all
    one = fn(w.q[1], float(thr[1]))                                         # a single 1-D query
    assert tuple(one[0].shape) == (2,)
    same(one, frr.ref_flat_range(w.qn[1:2], x, thr[1], ip=ip, values=values[1:2]))
    if ip:
        same(fm.similar_above(w.q, thr, use_norms=False), want)             # accepted and ignored
    # sort=True: by value, ties in row order
    lims, val, idx = cpu(fn(w.q, thr, sort=True))
    sv, si = qmatrix.sort_ranges(torch.from_numpy(want[0]), torch.from_numpy(want[1]), torch.from_numpy(want[2]), ip)
    same((lims, val, idx), (want[0], sv.numpy(), si.numpy()))
    for i in range(NQ):
        seg = val[lims[i]:lims[i + 1]]
        assert (np.diff(seg) <= 0).all() if ip else (np.diff(seg) >= 0).all()
    # the quantized matrix with these vectors attached returns the same, bit for bit
    qm = w.qm if not half else qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy()).attach_vectors(w.x, dtype=torch.float16)
    exact = qm.exact_similar_above if ip else qm.exact_within
    same(exact(w.q, thr), got)
    same(exact(w.q, thr, sort=True), (lims, val, idx))
    same(exact(w.q[1], float(thr[1])), one)


def test_filters_on_the_flat_matrix_and_the_exact_calls(ra, w):
    thr, values = w.thr[False, False], w.values[False, False]
    want = frr.ref_flat_range(w.qn, w.x, thr, allow=w.flags, values=values)
    assert want[0][-1] > 0
    f = w.fm.row_filter(w.flags)
    same(w.fm.within(w.q, thr, allow=f), want)
    same(w.fm.within(w.q, thr, allow=w.flags), want)
    same(w.qm.exact_within(w.q, thr, allow=w.flags), want)
    same(w.qm.exact_within(w.q, thr, allow=w.qm.row_filter(w.flags)), want)
    want = frr.ref_flat_range(w.qn, w.x, w.thr[True, False], ip=True, allow=w.flags, values=w.values[True, False])
    same(w.fm.similar_above(w.q, w.thr[True, False], allow=f), want)
    same(w.qm.exact_similar_above(w.q, w.thr[True, False], allow=w.flags), want)
    with pytest.raises(ra.PanicError, match="another matrix"):
        w.fm.within(w.q, thr, allow=w.fh.row_filter(w.flags))
    from reductive_amd import qmatrix
    bare = qmatrix.QuantizedMatrix(w.pq, w.codes.cpu().numpy())
    with pytest.raises(ra.PanicError, match="call attach_vectors first"):
        bare.exact_within(w.q, thr)
    with pytest.raises(ra.PanicError, match="call attach_vectors first"):
        bare.exact_similar_above(w.q, thr)


def test_partitioned_quantized_classes_return_original_rows(ra, w):
    thr, values = w.thr[False, False], w.values[False, False]
    want = frr.ref_flat_range(w.qn, w.x, thr, values=values)
    want_f = frr.ref_flat_range(w.qn, w.x, thr, allow=w.flags, values=values)
    want_ip = frr.ref_flat_range(w.qn, w.x, w.thr[True, False], ip=True, values=w.values[True, False])
    parts = (w.qm.partition(LISTS, n_iterations=3, vectors=w.x, rng=np.random.default_rng(9604)),
             w.qm.partition_residual(LISTS, n_iterations=3, pq_iterations=3, vectors=w.x, rng=np.random.default_rng(9604)))
    for pm in parts:
        assert pm.ids.cpu().numpy().tolist() != list(range(N))              # the layout is a real permutation
        pm.vectors = None                                                   # (partition carries the attached vectors over)
        with pytest.raises(ra.PanicError, match="call attach_vectors first"):
            pm.exact_within(w.q, thr)
        pm.attach_vectors(w.x)
        same(pm.exact_within(w.q, thr), want)
        same(pm.exact_within(w.q, thr), w.fm.within(w.q, thr))
        same(pm.exact_similar_above(w.q, w.thr[True, False]), want_ip)
        same(pm.exact_within(w.q, thr, allow=w.flags), want_f)
        with pytest.raises(ra.PanicError, match="position order"):
            pm.exact_within(w.q, thr, allow=pm.row_filter(w.flags))


@pytest.mark.parametrize("half", [False, True])
def test_partitioned_flat_matrix_range(ra, w, half):
    import torch
    fm, x = (w.fh, w.h) if half else (w.fm, w.x)
    pm = w.pm if not half else fm.partition(LISTS, n_iterations=3, rng=np.random.default_rng(9602))
    ids, off = pm.ids.cpu().numpy(), pm.list_off.cpu().numpy()
    list_of_row = np.empty(N, np.int64)
    list_of_row[ids] = np.repeat(np.arange(LISTS), np.diff(off))
    for ip in (False, True):
        thr, values = w.thr[ip, half], w.values[ip, half]
        fn = pm.similar_above if ip else pm.within
        flat = fm.similar_above if ip else fm.within
        # every list probed: FlatMatrix's result, in the order of the probed lists; sorted, equal up to the order of ties
        same_up_to_ties(fn(w.q, thr, nprobe=LISTS, sort=True), flat(w.q, thr, sort=True))
        # against the reference in position order, mapped to original rows
        for nprobe in (LISTS, 2):
            probes = pm.probes(w.q, nprobe).cpu().numpy()
            want = frr.ref_flat_range_lists(w.qn, x[ids], off, probes, thr, ip=ip, values=values[:, ids])
            got = fn(w.q, thr, nprobe=nprobe)
            same(got, (want[0], want[1], ids[want[2]]))
            if nprobe == 2:                                                  # the subset in the probed lists
                full = cpu(flat(w.q, thr))
                lims, val, rows = cpu(got)
                assert lims[-1] < full[0][-1]
                for i in range(NQ):
                    a = slice(full[0][i], full[0][i + 1])
                    inside = np.isin(list_of_row[full[2][a]], probes[i])
                    assert sorted(zip(full[2][a][inside].tolist(), bits(full[1][a][inside]))) == \
                        sorted(zip(rows[lims[i]:lims[i + 1]].tolist(), bits(val[lims[i]:lims[i + 1]])))
    thr, values = w.thr[False, half], w.values[False, half]
    # filters: a RowFilter of this matrix (position order inside) and bool flags in original row order
    probes = pm.probes(w.q, 3).cpu().numpy()
    want = frr.ref_flat_range_lists(w.qn, x[ids], off, probes, thr, allow=w.flags[ids], values=values[:, ids])
    assert want[0][-1] > 0
    same(pm.within(w.q, thr, nprobe=3, allow=pm.row_filter(w.flags)), (want[0], want[1], ids[want[2]]))
    same(pm.within(w.q, thr, nprobe=3, allow=w.flags), (want[0], want[1], ids[want[2]]))
    # a scalar radius, a single 1-D query, use_norms accepted
    one = pm.within(w.q[1], float(thr[1]), nprobe=LISTS)
    assert tuple(one[0].shape) == (2,)
    assert sorted(cpu(one)[2].tolist()) == cpu(fm.within(w.q[1], float(thr[1])))[2].tolist()
    same(pm.similar_above(w.q, w.thr[True, half], nprobe=2, use_norms=False), pm.similar_above(w.q, w.thr[True, half], nprobe=2))


def test_range_after_add_and_compact_equals_the_constructor(ra, w):
    import torch
    thr = w.thr[False, False]
    extra = (w.x[:300] + np.float32(0.05)).astype(np.float32)
    both = np.concatenate([w.x, extra])
    fm2 = w.fm.add(extra)
    same(fm2.within(w.q, thr), ra.FlatMatrix(both).within(w.q, thr))
    same(fm2.within(w.q, thr), frr.ref_flat_range(w.qn, both, thr))
    fm3, kept = fm2.compact(np.arange(N + 300) % 3 != 0)
    kept = kept.cpu().numpy()
    same(fm3.within(w.q, thr), ra.FlatMatrix(both[kept]).within(w.q, thr))
    same(fm3.within(w.q, thr), frr.ref_flat_range(w.qn, both[kept], thr))
    # the partitioned matrix: the constructor with the same centroids and assignments lays the rows out the same way
    pm2 = w.pm.add(extra)
    ids = w.pm.ids.cpu().numpy()
    assign = np.empty(N, np.int64)
    assign[ids] = np.repeat(np.arange(LISTS), np.diff(w.pm.list_off.cpu().numpy()))
    assign2 = np.concatenate([assign, w.pm.assign(extra).cpu().numpy()])
    built = ra.PartitionedFlatMatrix(both, w.pm.centroids, assign2)
    for nprobe in (3, LISTS):
        same(pm2.within(w.q, thr, nprobe=nprobe), built.within(w.q, thr, nprobe=nprobe))
    pm3, kept = pm2.compact(np.arange(N + 300) % 3 != 0)
    kept = kept.cpu().numpy()
    built = ra.PartitionedFlatMatrix(both[kept], w.pm.centroids, assign2[kept])
    for nprobe in (3, LISTS):
        same(pm3.within(w.q, thr, nprobe=nprobe), built.within(w.q, thr, nprobe=nprobe))
    same_up_to_ties(pm3.within(w.q, thr, nprobe=LISTS, sort=True), fm3.within(w.q, thr, sort=True))


def test_group_with_a_flat_part_still_refuses_a_range_search(ra, w):
    group = ra.MatrixGroup([w.qm, w.fm])
    with pytest.raises(ra.PanicError, match="not served"):
        group.within(w.q, 1.0)


def test_range_recall_of_the_quantized_search_is_measurable(ra, w, capsys):
    """the figure nobody could compute before: recall and precision of QuantizedMatrix.within against exact_within at the
    same radius.  Printed, not asserted: it is a property of the quantizer, not of this code."""
    thr = w.thr[False, False]
    lims, _, idx = cpu(w.qm.within(w.q, thr))
    elims, _, eidx = cpu(w.qm.exact_within(w.q, thr))
    hit = sum(len(set(idx[lims[i]:lims[i + 1]].tolist()) & set(eidx[elims[i]:elims[i + 1]].tolist())) for i in range(NQ))
    with capsys.disabled():
        print("\nrange recall of within() at the exact radius: %d of %d true rows found, %d returned"
              % (hit, int(elims[-1]), int(lims[-1])))
    assert elims[-1] > 0
