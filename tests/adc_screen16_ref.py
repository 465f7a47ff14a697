"""Numpy model of the 16-bit table screen over resident codes (pqhip_adc_screen16_f32_dev): prep16() the
preparation in float64 with L = floor(65,535 / M) levels per entry, screen16() the integer bound with the scaled epilogue,
slack16() the stated tightness.  The exact f32 value of the contract is chain() / values() of adc_screen_ref.py."""
import numpy as np

from adc_screen_ref import chain, values  # noqa: F401

NAME = "pqhip_adc_screen16_f32_dev"
KEEP_ALL, PER_ROW, SUM_MAX = 65535, -2, 65535
# the constants of DESIGN.md §5e / §5g, stated here on their own: Rel, Abs, F64, MaxSum, MinStep
REL, ABS, F64, MAX_SUM, MIN_STEP = 257 * 2.0 ** -32, 2.0 ** -100, 2.0 ** -40, 2.0 ** 126, 2.0 ** -120


def levels(M):
    """L: the value an entry saturates at, the most with M L <= 65,535"""
    return SUM_MAX // M


def prep16(t, thr, ip=False, scaled=False, cmax=0.0):
    """the parameters and the u16 image of one query -> dict(ulim, step, img [M, K] u16, base, E, B, s32, thr)"""
    M, K = t.shape
    L = levels(M)
    thr = np.float32(thr)
    out = dict(ulim=KEEP_ALL, step=1.0, img=np.zeros((M, K), np.uint16), base=0.0, E=0.0, B=np.float32(0), s32=np.float32(0), thr=thr)
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
        step = max(num / (L - 1), MIN_STEP)
        out["ulim"] = int(min(float(KEEP_ALL), np.floor(num / step * (1.0 + F64))))
    else:
        B = (E - base) + F64 * abs(base)
        num = spread + 2.0 * E
        if thr > 0 and cmax > 0:
            num = min(num, B - float(thr) / float(cmax) * (1.0 - 2.0 ** -20))
        step = max(num / (L - 1), MIN_STEP)
        b32, s32 = np.float32(B), np.float32(step)
        out.update(ulim=PER_ROW, B=b32 if float(b32) >= B else np.nextafter(b32, np.float32(np.inf)),
                   s32=s32 if float(s32) <= step else np.nextafter(s32, np.float32(-np.inf)))
    out["step"] = step
    out["img"] = np.minimum(float(L), np.floor((tp - lo[:, None]) / step * (1.0 - F64))).astype(np.uint16)
    return out


def screen16(t, codes, thr, ip=False, scales=None):
    """(bool [n], parameters, U [n]): the rows of one query that the screen returns (before the mask)"""
    sc = None if scales is None else np.asarray(scales, np.float32)
    fin = None if sc is None else sc[(sc >= 0) & np.isfinite(sc)]
    p = prep16(t, thr, ip, sc is not None, 0.0 if fin is None or fin.size == 0 else float(fin.max()))
    U = p["img"][np.arange(t.shape[0])[None, :], codes].astype(np.int64).sum(1)
    if p["ulim"] != PER_ROW:
        return U <= p["ulim"], p, U
    with np.errstate(invalid="ignore", over="ignore"):
        # fma(-s, U, B) in float64 is exact before its one rounding to f32 (24 + 16 bits)
        w = (p["B"].astype(np.float64) - p["s32"].astype(np.float64) * U).astype(np.float32)
        wu = ((np.abs(w).astype(np.float64) * 2.0 ** -22 + w).astype(np.float32) + np.float32(2.0 ** -100)).astype(np.float32)
        pv = (wu * sc).astype(np.float32)
        return ~((sc >= 0) & np.isfinite(sc) & (pv < p["thr"])), p, U


def slack16(p, M, v=None, c=None):
    """how far beyond the threshold a regular row may lie and still be returned.  Unscaled: the header's, M s + 2 E + the
    f64 slack.  Scaled (v the row's chain, c >= 0 its scale): a returned row has fl(w c) >= thr with v <= w < v + G up to
    2^-21 relative (the fma, the widening, the product), G = M s + 2 E + the roundings of B and of s32 U (U <= M L); so
    thr - v c <= G c + 2^-20 (|v| + G) c."""
    G = M * p["step"] + 2.0 * p["E"] + 2.0 ** -39 * (abs(float(p["thr"])) + abs(p["base"]))
    if c is None:
        return G
    G += 2.0 ** -22 * (abs(float(p["B"])) + M * levels(M) * p["step"])
    return G * c + 2.0 ** -20 * (np.abs(v) + G) * c + 1e-37
