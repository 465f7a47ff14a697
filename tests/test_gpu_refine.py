"""GPU tests of `refine=` on QuantizedMatrix, PartitionedMatrix and ResidualPartitionedMatrix: the ADC search with k = R
followed by the exact re-ranking of its candidates against the attached vectors (tests/rerank_ref.py), and what it buys
on the trained fixture of test_gpu_residual_encoding_is_more_accurate_than_flat_codes."""
import numpy as np
import pytest

import rerank_ref as rr
import synth
from test_gpu_adc_search_lists import ra  # noqa: F401


def _same(got, want):
    assert got[0].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    assert np.array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())


def _check_refined(search, q, vectors, k, R, ip):
    """search(k, refine) -> (value, idx): refine=R equals the reference applied to the candidates that the same call
    returns with k = R and refine=None"""
    cand = search(R, None)[1].cpu().numpy()
    v, i = search(k, R)
    single = q.ndim == 1
    want_v, want_i, flag = rr.ref_rerank(q, vectors, cand, k, ip=ip)
    assert not flag
    assert tuple(v.shape) == ((k,) if single else (q.shape[0], k))
    rr.assert_same(np.atleast_2d(v.cpu().numpy()), np.atleast_2d(i.cpu().numpy()), want_v, want_i)
    return cand


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_gpu_refine_on_the_three_matrix_classes(ra, dtype):
    import torch
    from reductive_amd import qmatrix
    N, M, K, dsub, nq, n_lists = 3000, 6, 16, 4, 7, 9
    d = M * dsub
    rng = np.random.default_rng(9970)
    x = rng.standard_normal((N, d)).astype(np.float32)
    ys = rng.standard_normal((nq, d)).astype(np.float32)
    pq = ra.Pq(None, synth.normalish(9971, (M, K, dsub)))
    norms = (1.0 + rng.random(N)).astype(np.float32)
    qm = qmatrix.QuantizedMatrix(pq, pq.quantize_batch(x), norms)
    yd = torch.from_numpy(ys).cuda()
    before = qm.most_similar(yd, 5), qm.nearest(yd, 5)
    with pytest.raises(ra.PanicError, match="attach_vectors"):
        qm.nearest(yd, 5, refine=50)
    with pytest.raises(ra.PanicError, match="attach_vectors"):
        qm.partition(n_lists, vectors=x, rng=np.random.default_rng(1)).nearest(yd, 5, 3, refine=50)
    tdt = getattr(torch, dtype)
    assert qm.attach_vectors(x, dtype=tdt) is qm
    assert qm.vectors.dtype == tdt and tuple(qm.vectors.shape) == (N, d) and qm.vectors.is_cuda
    kept = qm.vectors.cpu().numpy()                          # what the refinement reads: x rounded once for f16
    assert kept.astype(np.float32).tobytes() == x.astype(kept.dtype).astype(np.float32).tobytes()
    with pytest.raises(ra.PanicError):
        qm.attach_vectors(x[:-1])
    with pytest.raises(ra.PanicError):
        qm.attach_vectors(x, dtype=torch.bfloat16)
    for r in (4, 1025):
        with pytest.raises(ra.PanicError, match="between k and 1024"):
            qm.nearest(yd, 5, refine=r)
    pm = qm.partition(n_lists, vectors=x, rng=np.random.default_rng(9972))
    rm = qm.partition_residual(n_lists, vectors=x, n_iterations=5, pq_iterations=5, rng=np.random.default_rng(9972))
    assert pm.vectors is qm.vectors and rm.vectors is qm.vectors      # original row order: handed on as they are
    # refine=None is what it was
    _same(qm.most_similar(yd, 5), before[0])
    _same(qm.nearest(yd, 5), before[1])
    _same(qm.nearest(yd, 5), pq.adc_search_device(qm.codes, pq.adc_tables_device(yd), 5))
    _same(qm.most_similar(yd, 5, refine=None), before[0])
    for k, R in ((5, 5), (5, 60), (10, 1024)):
        for q, qt in ((ys, yd), (ys[2], yd[2])):
            _check_refined(lambda kk, r: qm.nearest(qt, kk, refine=r), q, kept, k, R, False)
            _check_refined(lambda kk, r: qm.most_similar(qt, kk, refine=r), q, kept, k, R, True)
            _check_refined(lambda kk, r: qm.most_similar(qt, kk, use_norms=False, refine=r), q, kept, k, R, True)
            for m in (pm, rm):
                for nprobe in (1, 3, n_lists):
                    c = _check_refined(lambda kk, r: m.nearest(qt, kk, nprobe, refine=r), q, kept, k, R, False)
                    _check_refined(lambda kk, r: m.most_similar(qt, kk, nprobe, refine=r), q, kept, k, R, True)
                    assert c.min() >= -1 and c.max() < N
    # a refined result over every row is the exact search: with R >= N nothing is lost to the quantizer
    small = qmatrix.QuantizedMatrix(pq, pq.quantize_batch(x[:800])).attach_vectors(x[:800], dtype=tdt)
    v, i = small.nearest(yd, 10, refine=1024)
    want_v, want_i, _ = rr.ref_rerank(ys, kept[:800], np.tile(np.arange(800), (nq, 1)), 10)
    rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)


def trained_fixture():
    """x [20000, 32], queries [200, 32]: the data of test_gpu_residual_encoding_is_more_accurate_than_flat_codes (that
    test builds it inline; the same seeds and draws are restated here), and the float64 distances of every pair"""
    N, d, nq = 20000, 32, 200
    rng = np.random.default_rng(9830)
    centres = (rng.standard_normal((40, d)) * 3.0).astype(np.float32)
    x = (centres[rng.integers(0, 40, N)] + rng.standard_normal((N, d))).astype(np.float32)
    ys = (x[rng.choice(N, nq, replace=False)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    x64, y64 = x.astype(np.float64), ys.astype(np.float64)
    d2 = np.stack([((x64 - y) ** 2).sum(1) for y in y64])
    return x, ys, d2


def restricted_truth(d2_row, cand_row, k, gamma):
    """the float64 top-k of one query restricted to its candidates (ties to the smaller row), and whether the f32 values
    are bound to give the same set: the k-th and (k+1)-th candidate distances a <= b are separated when
    b (1 - gamma) > a (1 + gamma) -- an f32 value lies within gamma * dist of the exact one (every term is >= 0, so the
    sum of absolute terms is the distance itself), all of the first k then stay below all of the rest."""
    ids = np.unique(cand_row[cand_row >= 0])
    order = ids[np.lexsort((ids, d2_row[ids]))]
    top = order[:k]
    if order.size <= k:
        return top, True
    a, b = d2_row[order[k - 1]], d2_row[order[k]]
    return top, bool(b * (1.0 - gamma) > a * (1.0 + gamma))


def test_fixture_stays_within_the_cap_on_the_cpu():
    """With the reference alone: for the most crowded candidate sets the fixture allows -- the true 100 nearest rows of
    every query -- at most 5 % of the queries have their 10th and 11th distances closer than the f32 bound, and for all
    others the reference's top-10 is the float64 top-10."""
    x, ys, d2 = trained_fixture()
    gamma = rr.f32_bound(x.shape[1])
    cand = np.argsort(d2, axis=1, kind="stable")[:, :100]
    v, i, _ = rr.ref_rerank(ys, x, cand, 10)
    left_out = 0
    for q in range(ys.shape[0]):
        top, separated = restricted_truth(d2[q], cand[q], 10, gamma)
        if not separated:
            left_out += 1
            continue
        assert sorted(i[q].tolist()) == sorted(top.tolist())
    print("queries left out: %d of %d" % (left_out, ys.shape[0]))
    assert left_out <= 0.05 * ys.shape[0]


@pytest.mark.gpu
def test_gpu_refine_removes_the_quantizer_ceiling(ra):
    """On the trained fixture at nprobe = 8, R = 100: recall@10 against the true float64 neighbours is strictly greater
    with refinement than without, for flat and for residual codes, and for every query the refined top-10 is the float64
    top-10 restricted to that query's candidate set.  A query whose 10th and 11th float64 candidate distances are not
    separated by the f32 bound (restricted_truth) is left out of the last check; at most 5 % may be."""
    import torch
    from reductive_amd import qmatrix
    M, bits, n_lists, k, nprobe, R = 8, 4, 64, 10, 8, 100
    x, ys, d2 = trained_fixture()
    nq = ys.shape[0]
    gamma = rr.f32_bound(x.shape[1])
    flat = ra.train_pq(M, bits, 10, 1, x, rng=np.random.default_rng(9831))
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x)).attach_vectors(x)
    pm = qm.partition(n_lists, vectors=x, rng=np.random.default_rng(9832))
    rm = qm.partition_residual(n_lists, vectors=x, rng=np.random.default_rng(9832))
    truth = np.argsort(d2, axis=1, kind="stable")[:, :k]
    yd = torch.from_numpy(ys).cuda()

    def recall(found):
        f = found.cpu().numpy()
        return float(np.mean([len(set(f[q].tolist()) & set(truth[q].tolist())) / k for q in range(nq)]))
    for name, m in (("flat", pm), ("residual", rm)):
        for probes in (1, 8, 64):
            plain = recall(m.nearest(yd, k, probes)[1])
            refined = recall(m.nearest(yd, k, probes, refine=R)[1])
            print("%s codes, nprobe %d: recall@10 %.4f, with refine=%d %.4f" % (name, probes, plain, R, refined))
            if probes == nprobe:
                assert refined > plain
        cand = m.nearest(yd, R, nprobe)[1].cpu().numpy()
        got = m.nearest(yd, k, nprobe, refine=R)[1].cpu().numpy()
        left_out = 0
        for q in range(nq):
            top, separated = restricted_truth(d2[q], cand[q], k, gamma)
            if not separated:
                left_out += 1
                continue
            assert sorted(got[q][got[q] >= 0].tolist()) == sorted(top.tolist()), (name, q)
        print("%s codes: %d of %d queries left out" % (name, left_out, nq))
        assert left_out <= 0.05 * nq
