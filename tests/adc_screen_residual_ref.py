"""Numpy model of the u8 table screen over residual codes in probed lists (pqhip_adc_screen_lists_residual_f32_dev;
DESIGN.md §5h): the preparation in float64 (constants of adc_screen_ref), the f32 predicate operation for operation, the
whole call.  The model has no integer limit per slot: the kernel's must not change a result."""
import numpy as np

import adc_screen_ref as asr

NAME = "pqhip_adc_screen_lists_residual_f32_dev"
f32 = np.float32


def threshold(thr, ip):
    """the threshold a query is screened at: a distance threshold of -Inf becomes the least finite f32"""
    return f32(-np.finfo(f32).max) if not ip and thr == -np.inf else f32(thr)


def call_wide(terms=None, scales=None):
    """(the least non-NaN term, the largest finite scale >= 0 or None): the reductions in front of the passes"""
    t, c = np.asarray([] if terms is None else terms, f32), np.asarray([0] if scales is None else scales, f32)
    t, c = t[~np.isnan(t)], c[(c >= 0) & np.isfinite(c)]
    return (float(t.min()) if t.size else np.inf), (None if scales is None else float(c.max()) if c.size else 0.0)


def floor_sum(thr, biases, ip, tmin=np.inf, cmax=None):
    """the least chain value that can still qualify, lowered by the f32 margin; biases: those of the query's valid slots"""
    b = np.asarray(biases, f32)
    b, th = b[~np.isnan(b)], float(f32(thr))
    if not ip:
        mb, mt = (float(b.min()) if b.size else np.inf), float(tmin)
        fr, mag = (mb + mt - th) * 0.5, abs(mb) + abs(mt) + abs(th)
    else:
        mb, t, ok = (float(b.max()) if b.size else -np.inf), th, True
        if cmax is not None:
            ok = th >= 2.0 ** -100 and cmax > 0
            t = th / float(cmax) if ok else 0.0
        fr, mag = (t - mb if ok else -np.inf), abs(t) + abs(mb)
    return fr - 2.0 ** -19 * mag - 2.0 ** -98


def prep(t, thr, floor):
    """adc_screen_prep_slot on the NEGATED table in its scaled mode (adc_screen_ref.prep without a scale), the step's span ended by `floor`"""
    p = asr.prep(t, thr, True, True, 0.0)
    if p["ulim"] == asr.PER_ROW and floor > -np.inf:
        tp = (-np.asarray(t, f32)).astype(np.float64)
        lo, spread = tp.min(1), 0.0
        for m in range(t.shape[0]):
            spread += tp[m].max() - lo[m]
        B = (p["E"] - p["base"]) + asr.F64 * abs(p["base"])
        step = max(min(spread + 2.0 * p["E"], B - floor) / asr.STEPS, asr.MIN_STEP)
        s32 = f32(step)
        p.update(step=step, s32=s32 if float(s32) <= step else np.nextafter(s32, f32(-np.inf)),
                 img=np.minimum(255.0, np.floor((tp - lo[:, None]) / step * (1.0 - asr.F64))).astype(np.uint8))
    return p


def keep(p, codes, bias, x, ip):
    """bool [n]: the rows a slot with `bias` returns; x [n] f32: the row terms (ip False) resp. the scales (ones without)"""
    U = p["img"][np.arange(codes.shape[1])[None, :], codes].astype(np.int64).sum(1)
    if p["ulim"] != asr.PER_ROW:
        return np.ones(U.shape, bool)
    bias, x = f32(bias), np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        # fma(-s, U, B) and fma(|w|, 2^-22, w) are exact in float64 before their one rounding to f32
        w = (p["B"].astype(np.float64) - p["s32"].astype(np.float64) * U).astype(f32)
        w = ((np.abs(w).astype(np.float64) * 2.0 ** -22 + w).astype(f32) + f32(2.0 ** -100)).astype(f32)
        if ip:
            return ~((x >= 0) & np.isfinite(x) & (((bias + w).astype(f32) * x).astype(f32) < p["thr"]))
        return ~(((bias + x).astype(f32) - (w + w).astype(f32)).astype(f32) > p["thr"])


def slack(p, M, s, bias, x, ip):
    """how far beyond the threshold a regular returned row may lie (include/pqhip.h); s: its chain, float64"""
    G = M * p["step"] + 2.0 * p["E"] + 2.0 ** -39 * (abs(float(p["thr"])) + abs(p["base"])) + 2.0 ** -22 * (abs(float(p["B"])) + 255 * p["step"])
    if ip:
        return (G + 2.0 ** -20 * (np.abs(bias) + np.abs(s) + G)) * x + 1e-37
    return 2.0 * G + 2.0 ** -20 * (np.abs((f32(bias) + np.asarray(x, f32)).astype(np.float64)) + 2.0 * np.abs(s) + 2.0 * G) + 1e-37


def ref_screen(tables, codes, list_off, probes, bias, thr, ip, terms=None, scales=None, allow=None):
    """(lims, idx) of the whole call: probe slot first, then ascending position, allowed rows only"""
    n, n_lists = codes.shape[0], len(list_off) - 1
    flags = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    x = np.asarray(terms if not ip else np.ones(n) if scales is None else scales, f32)
    tmin, cmax = call_wide(None if ip else terms, scales)
    rng = lambda l: (int(np.clip(list_off[l], 0, n)), int(np.clip(list_off[l + 1], 0, n)))
    out = []
    for q in range(tables.shape[0]):
        slots = [(j, rng(l)) for j, l in enumerate(probes[q].tolist()) if 0 <= l < n_lists and rng(l)[1] > rng(l)[0]]
        th = threshold(thr[q], ip)
        p = prep(tables[q], th, floor_sum(th, [bias[q, j] for j, _ in slots], ip, tmin, cmax))
        out += [np.concatenate([np.arange(lo, hi)[flags[lo:hi] & keep(p, codes[lo:hi], bias[q, j], x[lo:hi], ip)] for j, (lo, hi) in slots]
                               + [np.zeros(0, np.int64)])]
    return np.concatenate([[0], np.cumsum([r.size for r in out])]).astype(np.int64), np.concatenate(out + [np.zeros(0, np.int64)])
