"""CPU tests of the exact re-ranking: pins tests/rerank_ref.py (the numpy statement of pqhip_rerank_f32_dev) against
float64 and against the rules of the header, and the argument checks of Pq.rerank_device, which raise before the
library is reached."""
import numpy as np
import pytest

import rerank_ref as rr


def _data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)


@pytest.mark.parametrize("ip", [False, True])
@pytest.mark.parametrize("d", [1, 20, 63, 64, 65, 300, 768, 4096])
def test_reference_is_within_the_derived_bound_of_float64(d, ip):
    """Bound (rr.f32_bound): with u = 2^-24, a term is formed with 3 roundings' worth of relative error for L2
    (t = fl(q - x): u; t * t doubles it: 2u; the multiply's own rounding: u) or 1 for the inner product, and then
    passes through at most ceil(d / 64) chain additions and 6 tree additions, each a factor (1 + delta), |delta| <= u.
    So |value - exact| <= gamma_r * sum_j |term_j| with r = {3, 1} + ceil(d / 64) + 6 and gamma_r = r u / (1 - r u)
    (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  The float64 evaluation's own error, at most
    (d + 2) 2^-53 relative to the same sum, is added."""
    q, x = _data(d, 200, d, 3)
    for i in range(q.shape[0]):
        got = rr.row_values(q[i], x, ip=ip).astype(np.float64)
        want, scale = rr.f64_values(q[i], x, ip=ip)
        bound = (rr.f32_bound(d, ip=ip) + (d + 2) * 2.0 ** -53) * scale
        assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())


def test_bound_counts_the_roundings():
    u = 2.0 ** -24
    assert rr.f32_bound(300) == pytest.approx(14 * u, rel=1e-5)          # 3 + 5 + 6
    assert rr.f32_bound(4096, ip=True) == pytest.approx(71 * u, rel=1e-5)  # 1 + 64 + 6


def test_summation_order_is_lane_chains_then_the_tree():
    """a case where the defined order differs from the sequential sum and from pairwise summation of neighbours"""
    d = 130
    q = np.zeros(d, np.float32)
    x = np.zeros((1, d), np.float32)
    # inner product with q = 1: the terms are x itself
    q[:] = 1.0
    x[0, 0], x[0, 64], x[0, 128] = 2.0 ** 24, 1.0, 1.0           # lane 0 chain: fl(fl(2^24 + 1) + 1) = 2^24
    x[0, 32] = -2.0 ** 24                                         # tree step s = 32 cancels lane 0 against lane 32
    x[0, 1] = 3.0
    v = rr.row_values(q, x, ip=True)
    assert v[0] == np.float32(3.0)                                # the two ones are lost in lane 0's chain, as defined
    assert np.float32(np.float64(x[0].astype(np.float64).sum())) == np.float32(5.0)


def test_ties_go_to_the_smaller_row_id():
    q = np.zeros((1, 8), np.float32)
    x = np.ones((6, 8), np.float32)
    x[2] = 0.5
    cand = np.array([[5, 3, 2, 0, 4, 1]], np.int64)
    v, i, flag = rr.ref_rerank(q, x, cand, 6)
    assert not flag
    assert i.tolist() == [[2, 0, 1, 3, 4, 5]]
    assert v[0, 0] == np.float32(2.0) and (v[0, 1:] == np.float32(8.0)).all()
    v, i, _ = rr.ref_rerank(q + 1, x, cand, 3, ip=True)
    assert i.tolist() == [[0, 1, 3]] and (v == np.float32(8.0)).all()


def test_nan_zero_and_inf_handling():
    q = np.ones((1, 4), np.float32)
    x = np.array([[1, 1, 1, 1],            # L2 0
                  [np.nan, 1, 1, 1],       # NaN: after everything
                  [np.inf, 1, 1, 1],       # +Inf distance
                  [2, 1, 1, 1],
                  [np.nan, 0, 0, 0]], np.float32)
    cand = np.array([[4, 2, 1, 0, 3]], np.int64)
    v, i, _ = rr.ref_rerank(q, x, cand, 5)
    assert i.tolist() == [[0, 3, 2, 1, 4]]
    assert v[0, 0] == 0 and not np.signbit(v[0, 0]) and v[0, 2] == np.inf and np.isnan(v[0, 3:]).all()
    # inner product: -0 and +0 tie (row id decides) and come back as +0; -Inf is a number, NaN comes after it
    q = np.array([[1, 0, 0, 0]], np.float32)
    x = np.array([[-0.0, 5, 5, 5], [0.0, 5, 5, 5], [-np.inf, 0, 0, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    v, i, _ = rr.ref_rerank(q, x, np.array([[3, 2, 1, 0, 4]], np.int64), 5, ip=True)
    assert i.tolist() == [[4, 0, 1, 2, 3]]
    assert not np.signbit(v[0, 1]) and not np.signbit(v[0, 2]) and v[0, 3] == -np.inf and np.isnan(v[0, 4])


def test_padding_bad_ids_and_k_beyond_the_candidates():
    q, x = _data(7, 50, 70, 2)
    cand = np.array([[-1, 3, 50, 7, -1, -5], [-1, -1, -1, -1, -1, -1]], np.int64)
    v, i, flag = rr.ref_rerank(q, x, cand, 4)
    assert flag                                                   # 50 and -5 are outside [0, 50) and are not padding
    assert sorted(i[0, :2].tolist()) == [3, 7] and i[0, 2:].tolist() == [-1, -1]
    assert (v[0, 2:] == np.inf).all() and (i[1] == -1).all() and (v[1] == np.inf).all()
    assert not rr.ref_rerank(q, x, np.array([[-1, 3], [4, -1]], np.int64), 1)[2]
    v, i, _ = rr.ref_rerank(q, x, cand, 4, ip=True)
    assert (v[0, 2:] == -np.inf).all() and (v[1] == -np.inf).all()
    # no rows at all: every id but -1 flags, the outputs are padding
    v, i, flag = rr.ref_rerank(q, x[:0], np.array([[0, -1], [-1, -1]], np.int64), 3)
    assert flag and (i == -1).all() and (v == np.inf).all()


def test_duplicated_ids_are_returned_twice():
    q, x = _data(8, 10, 5, 1)
    v, i, flag = rr.ref_rerank(q, x, np.array([[4, 4, 9]], np.int64), 3)
    assert not flag and sorted(i[0].tolist()) == [4, 4, 9]
    assert v[0, i[0] == 4][0] == v[0, i[0] == 4][1]


@pytest.mark.parametrize("d", [1, 20, 63, 65, 300])
def test_widths_below_and_off_multiples_of_64(d):
    """the lanes beyond d hold +0 and the tree still runs over all 64: the same as zero-padding the row to 64 columns"""
    q, x = _data(d, 30, d, 1)
    pad = -d % 64
    qp, xp = np.pad(q, ((0, 0), (0, pad))), np.pad(x, ((0, 0), (0, pad)))
    for ip in (False, True):
        assert rr.row_values(q[0], x, ip=ip).tobytes() == rr.row_values(qp[0], xp, ip=ip).tobytes()
    if d <= 64:                   # one term per lane: the tree alone, checked against an explicit pairwise fold
        t = np.zeros((30, 64), np.float32)
        t[:, :d] = (q[0] - x) * (q[0] - x)
        for s in (32, 16, 8, 4, 2, 1):
            t = t[:, :s] + t[:, s:]
        assert rr.row_values(q[0], x).tobytes() == t[:, 0].tobytes()


def test_f16_vectors_equal_f32_vectors_of_the_converted_values():
    q, x = _data(9, 40, 100, 2)
    h = x.astype(np.float16)
    cand = np.random.default_rng(1).integers(0, 40, (2, 16))
    for ip in (False, True):
        a = rr.ref_rerank(q, h, cand, 8, ip=ip)
        b = rr.ref_rerank(q, h.astype(np.float32), cand, 8, ip=ip)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_argument_checks_raise_before_the_library_is_reached(monkeypatch):
    import torch
    import reductive_amd
    from reductive_amd import _lib
    from reductive_amd.pq import PanicError

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pq = reductive_amd.Pq(None, np.zeros((2, 4, 3), np.float32))
    monkeypatch.setattr(pq, "_cb", no_library)
    q = torch.zeros(2, 6)
    x = torch.zeros(9, 6)
    c = torch.zeros(2, 5, dtype=torch.int64)
    bad = [
        (dict(queries=q.double()), "queries must be float32"),
        (dict(queries=torch.zeros(1, 2, 6)), "queries must be float32"),
        (dict(vectors=x.to(torch.bfloat16)), "vectors must be float32 or float16"),
        (dict(vectors=x[0]), "vectors must be float32 or float16"),
        (dict(candidates=c.int()), "candidates must be int64"),
        (dict(candidates=c[0]), "candidates must be int64"),
        (dict(candidates=c[:1]), "one row per query"),
        (dict(vectors=torch.zeros(9, 7)), "length mismatch"),
        (dict(candidates=torch.zeros(2, 0, dtype=torch.int64)), "between 1 and 1024 candidates"),
        (dict(candidates=torch.zeros(2, 1025, dtype=torch.int64)), "between 1 and 1024 candidates"),
        (dict(k=0), "k must be between 1 and 1024"),
        (dict(k=1025), "k must be between 1 and 1024"),
        (dict(queries=q.numpy()), "must be a torch tensor"),
        (dict(), "must be CUDA tensors"),                  # everything else in order: host tensors stop here
    ]
    for change, message in bad:
        args = dict(queries=q, vectors=x, candidates=c, k=3)
        args.update(change)
        with pytest.raises(PanicError, match=message):
            pq.rerank_device(**args)


def test_refine_without_vectors_or_out_of_range_raises_before_any_search():
    from reductive_amd.pq import PanicError
    from reductive_amd.qmatrix import _Refine

    class Stub(_Refine):
        pass
    m = Stub()
    with pytest.raises(PanicError, match="attach_vectors"):
        m._check_refine(10, 100)
    m.vectors = object()
    assert m._check_refine(10, 100) == 100 and m._check_refine(10, 10) == 10
    for r in (9, 1025):
        with pytest.raises(PanicError, match="between k and 1024"):
            m._check_refine(10, r)
