"""Reference of the ADC list searches over residual codes (include/pqhip.h: pqhip_adc_search_lists_residual_f32_dev,
pqhip_adc_ip_search_lists_residual_f32_dev), composed from the oracle: the row sums s come from orc.adc_scan over the
inner-product tables of adc_ip_ref.ip_tables; every position is mapped to the probe slot through which it is reached
(the rules of adc_lists_ref.probed_positions for bad input); the two formulas of the header are applied in f32, one
rounding per operation:
    dist  = fl(fl(bias[q][p] + term[i]) - fl(s + s))        score = fl(fl(bias[q][p] + s) * scale[i])
and adc_lists_ref.ref_lists_search orders the rows of S_q by (key(value), position) and pads."""
import numpy as np

from adc_ip_ref import ip_tables
from adc_lists_ref import ref_lists_search
from oracle import pq_oracle as orc


def scan(quantizers, queries, codes, projection=None):
    """s [nq, n] f32: the oracle's scan of the codes over the queries' inner-product tables"""
    t = ip_tables(quantizers, np.atleast_2d(np.asarray(queries, np.float32)), projection=projection)
    return orc.adc_scan(t, np.ascontiguousarray(codes))


def probe_slots(list_off, probe_row, n):
    """slot [n] int64: the probe slot through which each position is reached, -1 for a position outside S_q.  -1 and
    ids outside [0, n_lists) are skipped, ranges are clamped to [0, n], an inverted range is empty."""
    list_off = np.asarray(list_off, np.int64)
    n_lists = list_off.size - 1
    slot = np.full(n, -1, np.int64)
    for p, l in enumerate(np.asarray(probe_row, np.int64).tolist()):
        if 0 <= l < n_lists:
            lo, hi = int(np.clip(list_off[l], 0, n)), int(np.clip(list_off[l + 1], 0, n))
            if hi > lo:
                slot[lo:hi] = p
    return slot


def residual_values(s, list_off, probes, bias, terms=None, scales=None, ip=False):
    """[nq, n] f32: the value of every row for every query (0 where the row is outside S_q: never selected)"""
    s2 = np.atleast_2d(np.asarray(s, np.float32))
    pr = np.atleast_2d(np.asarray(probes, np.int64))
    b2 = np.atleast_2d(np.asarray(bias, np.float32))
    nq, n = s2.shape
    assert pr.shape[0] == nq and b2.shape == pr.shape
    out = np.zeros((nq, n), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            slot = probe_slots(list_off, pr[q], n)
            on = slot >= 0
            b = b2[q][slot[on]]                                   # the bias of a skipped probe is never read
            if ip:
                v = (b + s2[q, on]).astype(np.float32)
                if scales is not None:
                    v = (v * np.asarray(scales, np.float32)[on]).astype(np.float32)
            else:
                x1 = (b + np.asarray(terms, np.float32)[on]).astype(np.float32)
                x2 = (s2[q, on] + s2[q, on]).astype(np.float32)
                v = (x1 - x2).astype(np.float32) + np.float32(0.0)   # a zero distance comes back as +0
            out[q, on] = v
    return out


def ref_residual_search(s, list_off, probes, bias, k, terms=None, scales=None, ip=False):
    """(value, idx) [nq, k]: the first min(k, |S_q|) rows of S_q by (key(dist), position), resp. (key(-score),
    position), then -1 and +Inf / -Inf"""
    vals = residual_values(s, list_off, probes, bias, terms=terms, scales=scales, ip=ip)
    return ref_lists_search(vals, list_off, probes, k, ip=ip)
