"""Reference of the ADC searches among given rows (include/pqhip.h: pqhip_adc_among_f32_dev, pqhip_adc_ip_among_f32_dev),
from the definition: per query the candidate set C_q is the entries of ids[lims[q] : lims[q + 1]] (of ids itself without
lims) that lie in [0, n) -- lims clamped to [0, n_ids], an inverted range empty, duplicates kept --, every candidate is
scored by the value formula of the header from a given scan matrix s [nq, n] (orc.adc_scan over the query's tables), one
rounding per operation, and the candidates are ordered by (key(value), row id) resp. (key(-score), row id) with the key
references of the exhaustive searches (test_gpu_adc_search.ref_search, adc_ip_ref.ref_ip_search).  Those break ties by
the index in the array they are given, so the candidates are handed over in ascending row id.  Numpy only."""
import numpy as np

from adc_ip_ref import ref_ip_search
from test_gpu_adc_search import ref_search


def candidates(ids, lims, q, n, row_list=None, n_lists=0):
    """(rows int64 ascending, flagged): the members of C_q, duplicates kept, and whether the range flag is raised by this
    query -- an id other than -1 outside [0, n), a lims end outside [0, n_ids], an inverted range, or (residual) a named
    row whose list id lies outside [0, n_lists), which is skipped"""
    ids = np.asarray(ids, np.int64)
    flagged = False
    if lims is None:
        mine = ids
    else:
        b, e = int(lims[q]), int(lims[q + 1])
        cb, ce = min(max(b, 0), ids.size), min(max(e, 0), ids.size)
        flagged = cb != b or ce != e or e < b
        mine = ids[cb:ce] if ce > cb else ids[:0]
    inside = (mine >= 0) & (mine < n)
    flagged = flagged or bool((~inside & (mine != -1)).any())
    rows = np.sort(mine[inside], kind="stable")
    if row_list is not None:
        l = np.asarray(row_list, np.int64)[rows]
        ok = (l >= 0) & (l < n_lists)
        flagged = flagged or bool((~ok).any())
        rows = rows[ok]
    return rows, flagged


def among_values(s_q, rows, ip, extra=None, row_list=None, bias_q=None):
    """the value of every candidate in `rows` for one query: s_q [n] the scan's row sums; extra [n] the scales (ip) or
    the row terms (residual distance) or None; row_list [n] and bias_q [n_lists]: the residual forms"""
    s = np.asarray(s_q, np.float32)[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        if row_list is None:
            if ip and extra is not None:
                return (s * np.asarray(extra, np.float32)[rows]).astype(np.float32)
            return s
        b = np.asarray(bias_q, np.float32)[np.asarray(row_list, np.int64)[rows]]
        if ip:
            v = (b + s).astype(np.float32)
            return v if extra is None else (v * np.asarray(extra, np.float32)[rows]).astype(np.float32)
        x1 = (b + np.asarray(extra, np.float32)[rows]).astype(np.float32)
        x2 = (s + s).astype(np.float32)
        return (x1 - x2).astype(np.float32) + np.float32(0.0)          # a zero distance comes back as +0


def ref_among(s, ids, k, lims=None, ip=False, extra=None, row_list=None, bias=None):
    """(value, idx, flagged): value / idx [nq, k], the first min(k, |C_q|) candidates by (key, row id), then -1 and
    +Inf / -Inf; flagged: whether any query raises the range flag (codes >= K are not modelled here)"""
    s2 = np.atleast_2d(np.asarray(s, np.float32))
    nq, n = s2.shape
    out_v = np.full((nq, k), -np.inf if ip else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    b2 = None if bias is None else np.atleast_2d(np.asarray(bias, np.float32))
    flagged = False
    for q in range(nq):
        rows, f = candidates(ids, lims, q, n, row_list, 0 if b2 is None else b2.shape[1])
        flagged = flagged or f
        vals = among_values(s2[q], rows, ip, extra, row_list, None if b2 is None else b2[q])
        v, i = (ref_ip_search if ip else ref_search)(vals, k)
        live = i[0] >= 0
        out_v[q, live] = v[0, live]
        out_i[q, live] = rows[i[0, live]]
    return out_v, out_i, flagged
