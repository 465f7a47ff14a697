"""Reference arithmetic of the ADC similarity search (include/pqhip.h: pqhip_adc_ip_tables_f32_dev,
pqhip_adc_ip_search_f32_dev), composed from the oracle's pieces: the inner-product tables are the `dp` term of
orc.adc_tables (CANON-F32 rule 1 unrolled dots, after the sequential query rotation of pq.rs:293), the scores are
orc.adc_scan over those tables times the row scales (one rounded f32 multiply), and the selection orders rows by
(key(-score), index)."""
import numpy as np


def unrolled_dot_rows(a, b):
    """CANON-F32 rule 1 (ndarray unrolled_dot) of every row of a [r, n] with b [n] (or with the matching row of b
    [r, n]): eight separately rounded f32 partial sums, then s = 0; s += p0 + p4; ... s += p3 + p7; then the tail."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    n = a.shape[-1]
    p = np.zeros((8, a.shape[0]), np.float32)
    i = 0
    while n - i >= 8:
        for l in range(8):
            p[l] = p[l] + a[:, i + l] * b[..., i + l]
        i += 8
    s = np.zeros(a.shape[0], np.float32)
    for u, v in ((0, 4), (1, 5), (2, 6), (3, 7)):
        s = s + (p[u] + p[v])
    for j in range(i, n):
        s = s + a[:, j] * b[..., j]
    return s.astype(np.float32)


def rotate_query(y, P):
    """y.dot(P) for a single vector (pq.rs:293): per output column one sequential f32 chain s = fl(s + fl(y[k] P[k][c]))
    from +0."""
    y = np.asarray(y, np.float32)
    P = np.asarray(P, np.float32)
    s = np.zeros(P.shape[1], np.float32)
    for k in range(P.shape[0]):
        s = s + y[k] * P[k]
    return s.astype(np.float32)


def ip_tables(quantizers, queries, projection=None):
    """[M, K] (one query [d]) or [nq, M, K]: ip[q][m][j] = unrolled_dot(quantizers[m][j], y_q[m])."""
    q = np.asarray(quantizers, np.float32)
    M, K, dsub = q.shape
    ys = np.asarray(queries, np.float32)
    single = ys.ndim == 1
    ys = ys[None] if single else ys
    out = np.empty((ys.shape[0], M, K), np.float32)
    for i in range(ys.shape[0]):
        y = rotate_query(ys[i], projection) if projection is not None else ys[i]
        for m in range(M):
            out[i, m] = unrolled_dot_rows(q[m], y[m * dsub:(m + 1) * dsub])
    return out[0] if single else out


def l2_from_ip(quantizers, queries, ip, projection=None):
    """fl(fl(yy + cc) - fl(ip + ip)), the distance table that k_adc_tables writes, from the IP table."""
    q = np.asarray(quantizers, np.float32)
    M, K, dsub = q.shape
    ys = np.asarray(queries, np.float32)
    single = ys.ndim == 1
    ys = ys[None] if single else ys
    ip3 = ip[None] if single else ip
    out = np.empty_like(ip3)
    for i in range(ys.shape[0]):
        y = rotate_query(ys[i], projection) if projection is not None else ys[i]
        for m in range(M):
            ym = y[m * dsub:(m + 1) * dsub]
            yy = unrolled_dot_rows(ym[None], ym)[0]
            cc = unrolled_dot_rows(q[m], q[m])
            out[i, m] = (yy + cc) - (ip3[i, m] + ip3[i, m])
    return out[0] if single else out


def scores(scan, scales=None):
    """fl(s * scales) per row (s itself without scales)."""
    s = np.asarray(scan, np.float32)
    if scales is None:
        return s
    with np.errstate(invalid="ignore"):                 # 0 * Inf is NaN, as on the device
        return (s * np.asarray(scales, np.float32)).astype(np.float32)


def ref_ip_search(score, k):
    """score [n] or [nq, n] f32 -> (score, idx) [nq, k]: rows ordered by (key(-score), index) -- the largest score
    first, -0 == +0, NaN after every number -- with index -1 / score -Inf past the last row.  Returned scores: zero as
    +0, NaN as NaN (compare with assert_same)."""
    s2 = np.atleast_2d(np.asarray(score, np.float32))
    nq, n = s2.shape
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    rows = np.arange(n)
    for q in range(nq):
        v = s2[q].astype(np.float64)
        nan = np.isnan(v)
        val = -np.where(nan, 0.0, v) + 0.0
        order = np.lexsort((rows, val, nan))        # last key is primary: NaN flag, -score, row index
        top = order[:min(k, n)]
        out_i[q, :top.size] = top
        out_s[q, :top.size] = s2[q, top] + np.float32(0.0)     # -0 -> +0
    return out_s, out_i


def assert_same(got_s, got_i, want_s, want_i):
    """indices exactly; scores bit for bit, NaN as the canonical quiet NaN"""
    got_s = np.asarray(got_s, np.float32)
    want_s = np.asarray(want_s, np.float32)
    assert np.array_equal(got_i, want_i)
    gn, wn = np.isnan(got_s), np.isnan(want_s)
    assert np.array_equal(gn, wn)
    assert (got_s[gn].view(np.uint32) == 0x7fc00000).all()
    assert got_s[~gn].tobytes() == want_s[~wn].tobytes()
