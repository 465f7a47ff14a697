"""Reference of the exact re-ranking (include/pqhip.h: pqhip_rerank_f32_dev) in numpy: the value of a row is 64 lane
partials, lane l the sequential f32 chain from +0 over j = l, l + 64, .. < d of fl(t * t), t = fl(q_j - x_j) (squared L2)
or fl(q_j * x_j) (inner product), reduced by the fixed tree p_l <- fl(p_l + p_(l+s)), s = 32 .. 1; every numpy f32
operation below is one rounded operation.  The candidates of a query that lie in [0, n_rows) are ordered by
(key(dist), row id) -- key(-score) for the inner product -- with the lexsort of adc_lists_ref.ref_lists_search (NaN
flag, value with -0 == +0, row id), and the outputs are padded with index -1 and +Inf / -Inf.  f16 vectors are converted
exactly to f32 first.  Compare with adc_ip_ref.assert_same (NaN as the canonical quiet NaN)."""
import numpy as np

from adc_ip_ref import assert_same   # noqa: F401  (re-exported for the tests)


def as_f32(vectors):
    """f32 as it is; f16 converted exactly"""
    v = np.asarray(vectors)
    assert v.dtype in (np.float32, np.float16)
    return v.astype(np.float32)


def row_values(query, rows, ip=False):
    """[n] f32: the value of every row of rows [n, d] for the query [d]"""
    q = np.asarray(query, np.float32)
    x = as_f32(rows)
    n, d = x.shape
    p = np.zeros((n, 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, d, 64):
            w = min(64, d - j0)
            if ip:
                term = q[j0:j0 + w] * x[:, j0:j0 + w]
            else:
                t = q[j0:j0 + w] - x[:, j0:j0 + w]
                term = t * t
            p[:, :w] = p[:, :w] + term
        for s in (32, 16, 8, 4, 2, 1):
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
    return p[:, 0].copy()


def candidate_ids(cand_row, n_rows):
    """(C_q in the order given, range flag): -1 is padding, any other id outside [0, n_rows) is skipped and flags"""
    c = np.asarray(cand_row, np.int64)
    ok = (c >= 0) & (c < n_rows)
    return c[ok], bool(((c != -1) & ~ok).any())


def ref_rerank(queries, vectors, cand, k, ip=False):
    """queries [nq, d] (or [d]), vectors [n, d] f32 / f16, cand [nq, n_cand] (or [n_cand]) int64 -> (value [nq, k] f32,
    idx [nq, k] int64, range flag)"""
    q2 = np.atleast_2d(np.asarray(queries, np.float32))
    c2 = np.atleast_2d(np.asarray(cand, np.int64))
    x = np.asarray(vectors)
    nq = q2.shape[0]
    assert c2.shape[0] == nq
    out_v = np.full((nq, k), -np.inf if ip else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    flag = False
    for q in range(nq):
        ids, bad = candidate_ids(c2[q], x.shape[0])
        flag |= bad
        if ids.size == 0:
            continue
        v32 = row_values(q2[q], x[ids], ip=ip)
        v = v32.astype(np.float64)
        nan = np.isnan(v)
        val = (-1.0 if ip else 1.0) * np.where(nan, 0.0, v) + 0.0        # -0 -> +0; NaN rows ordered by the flag
        order = np.lexsort((ids, val, nan))[:min(k, ids.size)]           # last key is primary
        out_i[q, :order.size] = ids[order]
        out_v[q, :order.size] = v32[order] + np.float32(0.0)             # a zero comes back as +0
    return out_v, out_i, flag


def f64_values(query, rows, ip=False):
    """the same quantity in float64, and the sum of the absolute terms (what the error bound scales with)"""
    q = np.asarray(query, np.float32).astype(np.float64)
    x = as_f32(rows).astype(np.float64)
    term = q * x if ip else (q - x) ** 2
    return term.sum(1), np.abs(term).sum(1)


def f32_bound(d, ip=False):
    """gamma with |value - exact| <= gamma * sum |term|: a term carries the roundings of its own formation -- L2: the
    subtraction, then squaring (2u) and the multiply's rounding (u), 3u in all; inner product: one multiply, u -- and of
    every addition it passes through: at most ceil(d / 64) in its lane's chain and six in the tree.  With r roundings
    the factor is (1 + u)^r - 1 <= r u / (1 - r u), u = 2^-24."""
    u = 2.0 ** -24
    r = (1 if ip else 3) + -(-d // 64) + 6
    return r * u / (1.0 - r * u)
