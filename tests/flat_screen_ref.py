"""Reference and bound model of the matrix-core range screen (include/pqhip.h: pqhip_flat_screen_f32_dev)
and of the two compositions built on it (Pq.flat_range_batch_device, Pq.flat_search_batch_device), in numpy.

The screen has no single right answer: any O_q with R_q <= O_q <= A is sound, and the contract caps what a regular row
may add.  So the reference here is (a) the exact range result R_q (flat_range_ref), (b) the slack of the contract in
f64 from the inputs, (c) the bound E the kernel uses, with its constants parsed from the header, and (d) a model of the
screening value -- operands rounded to f16 in numpy, the product sum in f64 plus the worst-case f32 accumulation term --
against which E is checked.  The compositions are modelled with the WIDEST sound screen of the model (every row not
provably outside under E), so that their equality with the exhaustive references is that of the argument in DESIGN.md."""
import math
import os
import re

import numpy as np

import flat_among_ref as far
import flat_range_ref as frr
import flat_search_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "reductive_amd", "csrc", "kernels_flat_screen.hip.h")
DRIVER = "pqhip_flat_screen.hip"
NAME = "pqhip_flat_screen_f32_dev"
OPTION = "flat_screen_wgs"
U16 = 2.0 ** -11            # unit roundoff of f16
U32 = 2.0 ** -24            # unit roundoff of f32
F16_MIN_NORMAL = 2.0 ** -14


def constants():
    """the bound's constexprs, read at call time so that a missing header fails the test that asks"""
    text = open(HEADER).read()
    out = {}
    for name in ("kFlatScreenRel", "kFlatScreenAbsX", "kFlatScreenAbs"):
        m = re.search(r"constexpr\s+(?:float|double)\s+%s\s*=\s*(0x[0-9a-fA-F.]+p[-+]?\d+)f?;" % name, text)
        assert m, name
        out[name] = float.fromhex(m.group(1))
    for name in ("kFlatScreenQueryTop", "kFlatScreenMaxExp", "kFlatScreenMaxD"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+);" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def slack(x, q, x_exp):
    """the contract's slack per (query, row) in f64: 2^-8 (||x||^2 + ||q||^2) + 2^-12 2^-x_exp ||q||_1 -> [nq, n]"""
    x = np.asarray(x, np.float64)
    q = np.atleast_2d(np.asarray(q, np.float64))
    xx = (x * x).sum(1)
    qq = (q * q).sum(1)
    q1 = np.abs(q).sum(1)
    return 2.0 ** -8 * (xx[None, :] + qq[:, None]) + 2.0 ** -12 * 2.0 ** -x_exp * q1[:, None]


def screen_bound(x, q, x_exp, ip=False):
    """E per (query, row) in f64, the kernel's formula on exact norms: kFlatScreenRel (xx + qq) + kFlatScreenAbsX
    2^-x_exp ||q||_1 (half of both for the inner product) + kFlatScreenAbs -> [nq, n]"""
    c = constants()
    x = np.asarray(x, np.float64)
    q = np.atleast_2d(np.asarray(q, np.float64))
    xx = (x * x).sum(1)
    qq = (q * q).sum(1)
    q1 = np.abs(q).sum(1)
    half = 0.5 if ip else 1.0
    return half * (c["kFlatScreenRel"] * (xx[None, :] + qq[:, None])
                   + c["kFlatScreenAbsX"] * 2.0 ** -x_exp * q1[:, None]) + c["kFlatScreenAbs"]


def to_f16(v, flush):
    """f64 values -> f16 (RNE) -> f64; flush: f16 subnormals become zero"""
    with np.errstate(over="ignore"):
        h = np.asarray(v, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)
    if flush:
        h = np.where(np.abs(h) < F16_MIN_NORMAL, 0.0, h)
    return h


def query_exp(q):
    """e_q of the prep kernel: 2^e_q max |q_j| in [2^kFlatScreenQueryTop, 2 * that); 0 for the zero vector"""
    m = float(np.abs(np.asarray(q, np.float64)).max())
    return 0 if m == 0.0 else constants()["kFlatScreenQueryTop"] - (math.frexp(m)[1] - 1)


def model_values(x, q, x_exp, ip=False, flush=False):
    """The screening value of every (query, row) as the kernel forms it, in f64, and the worst it can be off by f32
    arithmetic the model does not replay: (v^ [nq, n], arith [nq, n]).  v^ = xx + qq - 2 dot (L2) resp. dot with dot the
    f64 sum of the f16 operands' products, scaled back.  arith: the f32 accumulation of up to dp products in any order
    (gamma = (dp - 1) 2^-23 on sum |X~ Q~|: twice the RNE figure, for an accumulator that truncates), the f32 sum of the
    squares in xx ((d + 1) 2^-24 xx) and the three roundings of the epilogue (3 * 2^-24 (xx + qq + 2 sum))."""
    x = np.asarray(x, np.float64)
    q2 = np.atleast_2d(np.asarray(q, np.float64))
    d = x.shape[1]
    dp = -(-d // 32) * 32
    X = to_f16(x * 2.0 ** x_exp, flush)
    xx = (x * x).sum(1)
    vh = np.empty((q2.shape[0], x.shape[0]))
    arith = np.empty_like(vh)
    for i, qv in enumerate(q2):
        e = query_exp(qv)
        Q = to_f16(qv * 2.0 ** e, flush)
        back = 2.0 ** (-e - x_exp)
        dot = (X * Q[None, :]).sum(1) * back
        mag = (np.abs(X) * np.abs(Q)[None, :]).sum(1) * back
        qq = (qv * qv).sum()
        acc = (dp - 1) * 2.0 ** -23 * mag
        if ip:
            vh[i] = dot
            arith[i] = acc + 3 * U32 * mag
        else:
            vh[i] = xx + qq - 2.0 * dot
            arith[i] = 2.0 * acc + (d + 1) * U32 * xx + 3 * U32 * (xx + qq + 2.0 * mag)
    return vh, arith


def regular_rows(x, x_exp):
    """rows with finite elements whose scaled elements stay below 2^15"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(1) & (np.abs(x * 2.0 ** x_exp) < 2.0 ** 15).all(1)


def widest_screen(q, x, thr, x_exp, ip=False, allow=None, values=None):
    """CSR (lims, idx) of the widest sound screen the model allows: every allowed row that is not provably outside under
    E around its EXACT value (v - E <= thr resp. v + E >= thr, written as the negation so that NaN passes)"""
    v = frr.all_values(q, x, ip) if values is None else values
    nq, n = v.shape
    t = np.broadcast_to(np.asarray(thr, np.float32).reshape(-1), (nq,)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        E = screen_bound(np.asarray(x, np.float64), q, x_exp, ip)
        v64 = v.astype(np.float64)
        outside = (v64 + E < t[:, None]) if ip else (v64 - E > t[:, None])
    keep = ~outside
    if allow is not None:
        keep &= np.asarray(allow, bool)[None, :]
    lims = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    idx = np.concatenate([np.flatnonzero(k) for k in keep]).astype(np.int64) if nq else np.zeros(0, np.int64)
    return lims, idx


def ref_flat_range_batch(q, x, thr, x_exp=0, ip=False, allow=None):
    """the composition: widest screen, then the exact range among its ids -> (lims, val, idx)"""
    v = frr.all_values(q, x, ip)
    lims, ids = widest_screen(q, x, thr, x_exp, ip, allow, v)
    out_l, val, idx, flagged = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=v)
    assert not flagged
    return out_l, val, idx


def ref_flat_search_batch(q, x, k, sample, fallback, x_exp=0, ip=False, allow=None):
    """the composition with the rules handed in: sample(n, k) -> (S, t), fallback(total, n, nq) -> bool;
    -> (val, idx, fell_back [nq] bool)"""
    q2 = np.atleast_2d(np.asarray(q, np.float32))
    x = np.asarray(x)
    nq, n = q2.shape[0], x.shape[0]
    v = frr.all_values(q2, x, ip)
    _, t = sample(n, k)
    ids = np.arange(0, n, t, dtype=np.int64)
    if allow is not None:
        ids = np.where(np.asarray(allow, bool)[ids], ids, -1)
    sv, si, flagged = far.ref_flat_among(q2, x, ids, k, ip=ip, values=v)
    assert not flagged
    T = sv[:, k - 1]
    thin = (si[:, k - 1] < 0) | np.isnan(T)
    thr = np.where(thin, np.float32(np.inf if ip else -np.inf), T).astype(np.float32)
    lims, cand = widest_screen(q2, x, thr, x_exp, ip, allow, v)
    plain = thin.copy()
    if fallback(int(lims[-1]), n, nq):
        plain[:] = True
    val, idx, flagged = far.ref_flat_among(q2, x, cand, k, lims=lims, ip=ip, values=v)
    assert not flagged
    if plain.any():
        pv, pi = fr.ref_flat_search(q2[plain], x, k, ip=ip, allow=allow)
        val[plain], idx[plain] = pv, pi
    return val, idx, plain
