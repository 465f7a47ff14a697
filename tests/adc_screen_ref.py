"""Numpy model of the u8 table screen over resident codes (pqhip_adc_screen_f32_dev) and of the composition
built on it (Pq.adc_search_batch_device): prep() the preparation in float64, screen() the integer bound with the scaled
epilogue, chain() the exact f32 value of the contract, ref_adc_search_batch the sample / screen / resolve / fall back."""
import numpy as np

from adc_among_ref import ref_among
from adc_masked_ref import ref_masked_search

NAME = "pqhip_adc_screen_f32_dev"
OPTION = "adc_screen_wgs"
KEEP_ALL, PER_ROW = 65535, -2
# the constants of DESIGN.md §5e, stated here on their own: Rel, Abs, F64, MaxSum, MinStep, Steps
REL, ABS, F64, MAX_SUM, MIN_STEP, STEPS = 257 * 2.0 ** -32, 2.0 ** -100, 2.0 ** -40, 2.0 ** 126, 2.0 ** -120, 254


def chain(t, codes):
    """the scan's value of every row: the sequential f32 chain over m from +0; t [M, K] f32, codes [n, M] -> f32 [n]"""
    s = np.zeros(codes.shape[0], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(t.shape[0]):
            s = (s + t[m, codes[:, m]]).astype(np.float32)
    return s


def values(t, codes, ip=False, scales=None):
    v = chain(t, codes)
    if ip and scales is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            v = (v * np.asarray(scales, np.float32)).astype(np.float32)
    return v


def prep(t, thr, ip=False, scaled=False, cmax=0.0):
    """the parameters and the u8 image of one query -> dict(ulim, step, img [M, K] u8, base, E, B, s32)"""
    M, K = t.shape
    thr = np.float32(thr)
    out = dict(ulim=KEEP_ALL, step=1.0, img=np.zeros((M, K), np.uint8), base=0.0, E=0.0, B=np.float32(0), s32=np.float32(0), thr=thr)
    tp = (np.float32(-1 if ip else 1) * np.asarray(t, np.float32)).astype(np.float64)
    if not np.isfinite(tp).all() or np.isnan(thr):
        return out
    lo, hi = tp.min(1), tp.max(1)
    total = absum = A = spread = 0.0
    for m in range(M):
        total += lo[m]
        absum += abs(lo[m])
        A += np.abs(tp[m]).max()
        spread += hi[m] - lo[m]
    if A > MAX_SUM:
        return out
    th = float(-thr if ip else thr)
    if not scaled and np.isinf(thr):
        out["ulim"] = -1 if th < 0 else KEEP_ALL
        return out
    if scaled and thr == -np.inf:
        return out
    E = REL * M * A + ABS
    base = total - F64 * absum
    out.update(E=E, base=base)
    if not scaled:
        num = (th - base) + E + F64 * (abs(th) + abs(base))
        if not num > 0.0:
            out["ulim"] = -1
            return out
        step = max(num / STEPS, MIN_STEP)
        out["ulim"] = int(min(float(KEEP_ALL), np.floor(num / step * (1.0 + F64))))
    else:
        B = (E - base) + F64 * abs(base)
        num = spread + 2.0 * E
        if thr > 0 and cmax > 0:
            num = min(num, B - float(thr) / float(cmax) * (1.0 - 2.0 ** -20))
        step = max(num / STEPS, MIN_STEP)
        b32, s32 = np.float32(B), np.float32(step)
        out.update(ulim=PER_ROW, B=b32 if float(b32) >= B else np.nextafter(b32, np.float32(np.inf)),
                   s32=s32 if float(s32) <= step else np.nextafter(s32, np.float32(-np.inf)))
    out["step"] = step
    out["img"] = np.minimum(255.0, np.floor((tp - lo[:, None]) / step * (1.0 - F64))).astype(np.uint8)
    return out


def screen(t, codes, thr, ip=False, scales=None):
    """bool [n]: the rows of one query that the screen returns (before the mask), and the parameters"""
    sc = None if scales is None else np.asarray(scales, np.float32)
    fin = None if sc is None else sc[(sc >= 0) & np.isfinite(sc)]
    p = prep(t, thr, ip, sc is not None, 0.0 if fin is None or fin.size == 0 else float(fin.max()))
    U = p["img"][np.arange(t.shape[0])[None, :], codes].astype(np.int64).sum(1)
    if p["ulim"] != PER_ROW:
        return U <= p["ulim"], p
    with np.errstate(invalid="ignore", over="ignore"):
        # fma(-s, U, B) in float64 is exact before its one rounding to f32 (24 + 16 bits)
        w = (p["B"].astype(np.float64) - p["s32"].astype(np.float64) * U).astype(np.float32)
        wu = ((np.abs(w).astype(np.float64) * 2.0 ** -22 + w).astype(np.float32) + np.float32(2.0 ** -100)).astype(np.float32)
        pv = (wu * sc).astype(np.float32)
        return ~((sc >= 0) & np.isfinite(sc) & (pv < p["thr"])), p


def slack(p, M, v=None, c=None):
    """how far beyond the threshold a regular row may lie and still be returned.  Unscaled: the header's.  Scaled (v the
    row's chain, c >= 0 its scale): a returned row has fl(w c) >= thr with v <= w < v + G up to 2^-21 relative (the fma,
    the widening, the product), G = M s + 2 E + the roundings of B and s32 U; so thr - v c <= G c + 2^-20 (|v| + G) c."""
    G = M * p["step"] + 2.0 * p["E"] + 2.0 ** -39 * (abs(float(p["thr"])) + abs(p["base"]))
    if c is None:
        return G
    G += 2.0 ** -22 * (abs(float(p["B"])) + 255 * p["step"])
    return G * c + 2.0 ** -20 * (np.abs(v) + G) * c + 1e-37


def ref_adc_search_batch(tables, codes, k, sample, falls_back, ip=False, scales=None, allow=None):
    """(value, idx, plain): the composition of Pq.adc_search_batch_device over the references; plain: the queries that
    took the plain call.  sample / falls_back: the pure rules of reductive_amd.pq."""
    nq, n = tables.shape[0], codes.shape[0]
    flags = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    s = np.stack([chain(tq, codes) for tq in tables])
    full = np.stack([values(tq, codes, ip, scales) for tq in tables])
    want = ref_masked_search(full, flags, k, ip=ip)
    ids = np.arange(0, n, sample(n, k)[1], dtype=np.int64)
    ids = np.where(flags[ids], ids, -1)
    sv, si, _ = ref_among(s, ids, k, ip=ip, extra=scales)
    thin = (si[:, k - 1] < 0) | np.isnan(sv[:, k - 1])
    keep = [np.flatnonzero(screen(tables[q], codes, sv[q, k - 1], ip, scales)[0] & flags & ~thin[q]) for q in range(nq)]
    lims = np.concatenate([[0], np.cumsum([r.size for r in keep])]).astype(np.int64)
    plain = thin | falls_back(int(lims[-1]), n, nq)
    val, idx, _ = ref_among(s, np.concatenate(keep) if nq else ids[:0], k, lims=lims, ip=ip, extra=scales)
    val[plain], idx[plain] = want[0][plain], want[1][plain]
    return val, idx, plain, want
