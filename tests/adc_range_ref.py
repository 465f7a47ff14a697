"""Reference of the ADC range searches (include/pqhip.h: pqhip_adc_*range*_f32_dev), written from their definition: a
per-row predicate with the IEEE comparison -- value <= thr for distances, value >= thr for similarities (ip=True), so a NaN
on either side never qualifies -- then the stated order: ascending row index for the exhaustive calls, the order of the
concatenation of the probed lists (probe slot first, then position) for the list calls.  Values are kept bit for bit (no
key, the sign of a zero stays).  The values of ALL rows come from the caller (the scan of the same tables); the residual
form applies the two formulas of adc_residual_ref.py per probe slot, one f32 rounding per operation:
    dist = fl(fl(bias[q][p] + term[i]) - fl(s + s))        score = fl(fl(bias[q][p] + s) * scale[i])
A mask (allow bool [n]) removes rows before the predicate: a disallowed row enters nothing.
Every function returns CSR: (lims int64 [nq + 1], val f32 [total], idx int64 [total]).  Numpy only."""
import numpy as np


def _hits(v, thr, ip):
    with np.errstate(invalid="ignore"):
        return (v >= np.float32(thr)) if ip else (v <= np.float32(thr))


def _csr(vals, idxs):
    lims = np.zeros(len(vals) + 1, np.int64)
    np.cumsum([v.size for v in vals], out=lims[1:])
    val = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, np.float32)
    idx = np.concatenate(idxs).astype(np.int64) if idxs else np.zeros(0, np.int64)
    return lims, val, idx


def _thresholds(thr, nq):
    t = np.asarray(thr, np.float32).reshape(-1)
    return np.broadcast_to(t, (nq,)) if t.size == 1 else t


def ref_range(values, thr, ip=False, allow=None):
    """values [n] or [nq, n] f32 of every row (distances, or scores with ip=True); thr a scalar or [nq] -> CSR, the
    qualifying rows of each query in ascending row index"""
    v2 = np.atleast_2d(np.asarray(values, np.float32))
    nq, n = v2.shape
    t = _thresholds(thr, nq)
    ok = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    vals, idxs = [], []
    for q in range(nq):
        rows = np.flatnonzero(ok & _hits(v2[q], t[q], ip))
        vals.append(v2[q, rows])
        idxs.append(rows)
    return _csr(vals, idxs)


def _segments(list_off, probe_row, n):
    """(probe slot, lo, hi) of every served probe, in probe order: -1 and ids outside [0, n_lists) are skipped, ranges are
    clamped to [0, n] and an inverted or empty range is skipped (adc_lists_ref.probed_positions, slot by slot)"""
    list_off = np.asarray(list_off, np.int64)
    n_lists = list_off.size - 1
    for p, l in enumerate(np.asarray(probe_row, np.int64).tolist()):
        if 0 <= l < n_lists:
            lo, hi = int(np.clip(list_off[l], 0, n)), int(np.clip(list_off[l + 1], 0, n))
            if hi > lo:
                yield p, lo, hi


def ref_range_lists(values, list_off, probes, thr, ip=False, allow=None):
    """values [nq, n] of every row; list_off [n_lists + 1]; probes [nq, n_probe] -> CSR, idx = positions, the rows of a
    query in the order of the concatenation of its probed lists (a list named twice appears twice)"""
    v2 = np.atleast_2d(np.asarray(values, np.float32))
    pr = np.atleast_2d(np.asarray(probes, np.int64))
    nq, n = v2.shape
    assert pr.shape[0] == nq
    t = _thresholds(thr, nq)
    ok = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    vals, idxs = [], []
    for q in range(nq):
        v_q, i_q = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
        for _, lo, hi in _segments(list_off, pr[q], n):
            pos = np.arange(lo, hi, dtype=np.int64)
            pos = pos[ok[pos] & _hits(v2[q, pos], t[q], ip)]
            v_q.append(v2[q, pos])
            i_q.append(pos)
        vals.append(np.concatenate(v_q))
        idxs.append(np.concatenate(i_q))
    return _csr(vals, idxs)


def ref_range_residual(s, list_off, probes, bias, thr, terms=None, scales=None, ip=False, allow=None):
    """s [nq, n] f32: the scan over the inner-product tables; bias [nq, n_probe]; terms [n] (distance) or scales [n] / None
    (similarity) -> CSR as ref_range_lists.  The bias is that of the probe slot through which a row is reached; the bias
    of a skipped probe, and the term / scale of a disallowed row, enter nothing."""
    s2 = np.atleast_2d(np.asarray(s, np.float32))
    pr = np.atleast_2d(np.asarray(probes, np.int64))
    b2 = np.atleast_2d(np.asarray(bias, np.float32))
    nq, n = s2.shape
    assert pr.shape[0] == nq and b2.shape == pr.shape
    t = _thresholds(thr, nq)
    ok = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    vals, idxs = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            v_q, i_q = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
            for p, lo, hi in _segments(list_off, pr[q], n):
                pos = np.arange(lo, hi, dtype=np.int64)
                pos = pos[ok[pos]]                                   # before anything of the row is read
                b = b2[q, p]
                if ip:
                    v = (b + s2[q, pos]).astype(np.float32)
                    if scales is not None:
                        v = (v * np.asarray(scales, np.float32)[pos]).astype(np.float32)
                else:
                    x1 = (b + np.asarray(terms, np.float32)[pos]).astype(np.float32)
                    x2 = (s2[q, pos] + s2[q, pos]).astype(np.float32)
                    v = (x1 - x2).astype(np.float32)
                hit = _hits(v, t[q], ip)
                v_q.append(v[hit])
                i_q.append(pos[hit])
            vals.append(np.concatenate(v_q))
            idxs.append(np.concatenate(i_q))
    return _csr(vals, idxs)
