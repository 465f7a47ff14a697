"""Reference of the query-free row terms (include/pqhip.h: pqhip_residual_terms_f32_dev), written element by element from
the definition: with r = quantizers[m][code[i][m]][e] and c = centroids[assign[i]][m ds + e] widened to f64,
    p[i][m] = sequential f64 sum over e, from +0, of (r r + 2 c r)          (two exact products, one rounded add, then
                                                                              one rounded add into the running sum)
    t[i]    = (float32) of the sequential f64 sum over m, from +0, of p[i][m]
numpy float64 scalars are IEEE doubles and Python never fuses a multiply with an add, so the loops below ARE the
definition; they are vectorised over the rows only, which changes no operation and no order.  A code >= K reads entry 0;
a list id outside [0, n_lists) gives +0."""
import numpy as np


def ref_terms(quantizers, codes, assign, centroids):
    """quantizers [M, K, ds] f32, codes [n, M] integer, assign [n] integer, centroids [n_lists, M ds] f32 -> f32 [n]"""
    q = np.asarray(quantizers, np.float32)
    M, K, ds = q.shape
    codes = np.asarray(codes).astype(np.int64)
    assign = np.asarray(assign).astype(np.int64)
    cen = np.asarray(centroids, np.float32)
    n = codes.shape[0]
    good = (assign >= 0) & (assign < cen.shape[0])
    a = np.where(good, assign, 0)
    codes = np.where(codes >= K, 0, codes)
    t = np.zeros(n, np.float64)
    for m in range(M):
        p = np.zeros(n, np.float64)
        for e in range(ds):
            r = q[m, codes[:, m], e].astype(np.float64)
            c = cen[a, m * ds + e].astype(np.float64)
            p = p + (r * r + (2.0 * c) * r)
        t = t + p
    out = t.astype(np.float32)
    out[~good] = np.float32(0.0)
    return out


def abs_sum(quantizers, codes, assign, centroids):
    """S_i = sum_j (r^2 + |2 c r|) in float64: the scale of the accumulated rounding error of a row's term"""
    q = np.asarray(quantizers, np.float32)
    M, K, ds = q.shape
    codes = np.asarray(codes).astype(np.int64)
    r = q[np.arange(M)[None, :], codes].reshape(codes.shape[0], M * ds).astype(np.float64)
    c = np.asarray(centroids, np.float32)[np.asarray(assign)].astype(np.float64)
    return (r * r + np.abs(2.0 * c * r)).sum(1)
