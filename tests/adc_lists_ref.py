"""Reference of the ADC search over a partitioned code matrix (include/pqhip.h: pqhip_adc_search_lists_f32_dev,
pqhip_adc_ip_search_lists_f32_dev), composed from the oracle: the values of ALL rows come from orc.adc_scan (distances)
or adc_ip_ref.scores over orc.adc_scan of the inner-product tables (scores); query q keeps the rows of S_q, the rows of
the lists its probe row names, orders them by (key(value), position) -- key(-score) for the similarity search -- and
pads with index -1 and +Inf / -Inf.  List l is positions [list_off[l], list_off[l + 1])."""
import numpy as np


def probed_positions(list_off, probe_row, n):
    """positions of S_q in probe order: -1 and ids outside [0, n_lists) are skipped, ranges are clamped to [0, n] and
    an inverted range is empty (what the header declares for bad input)"""
    list_off = np.asarray(list_off, np.int64)
    n_lists = list_off.size - 1
    out = []
    for l in np.asarray(probe_row, np.int64).tolist():
        if 0 <= l < n_lists:
            lo, hi = int(np.clip(list_off[l], 0, n)), int(np.clip(list_off[l + 1], 0, n))
            if hi > lo:
                out.append(np.arange(lo, hi, dtype=np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def ref_lists_search(values, list_off, probes, k, ip=False):
    """values [nq, n] f32 (distances, or scores with ip=True) of every row; probes [nq, n_probe] -> (value, idx)
    [nq, k]: the first min(k, |S_q|) rows of S_q by (key, position), then -1 and +Inf (ip: -Inf).  Returned scores
    carry a zero as +0."""
    v2 = np.atleast_2d(np.asarray(values, np.float32))
    pr = np.atleast_2d(np.asarray(probes, np.int64))
    nq, n = v2.shape
    assert pr.shape[0] == nq
    out_v = np.full((nq, k), -np.inf if ip else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        pos = probed_positions(list_off, pr[q], n)
        v = v2[q, pos].astype(np.float64)
        nan = np.isnan(v)
        val = (-1.0 if ip else 1.0) * np.where(nan, 0.0, v) + 0.0       # -0 -> +0; NaN rows ordered by the flag
        order = np.lexsort((pos, val, nan))                              # last key is primary
        top = pos[order[:min(k, pos.size)]]
        out_i[q, :top.size] = top
        out_v[q, :top.size] = v2[q, top] + np.float32(0.0) if ip else v2[q, top]
    return out_v, out_i
