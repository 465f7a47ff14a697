"""Reference of the exact search in probed lists (include/pqhip.h: pqhip_flat_search_lists_f32_dev) in numpy: by
definition query q is flat_search_ref.ref_flat_search of that query alone with the mask "the row lies in a list that probe
row q names, and is allowed".  Also says whether the device raises the range flag: a probe id other than -1 outside
[0, n_lists), or a probed list whose offsets leave [0, n] or are inverted."""
import numpy as np

import flat_search_ref as fr
from flat_search_ref import assert_same, mask_words   # noqa: F401  (re-exported for the tests)


def probed_mask(list_off, probe_row, n):
    """(bool [n]: the row lies in a probed list, flag).  -1 is padding; any other id outside [0, n_lists) is skipped and
    flagged; a range is clamped to [0, n] and an inverted one is empty, both flagged."""
    off = np.asarray(list_off, np.int64)
    n_lists = off.size - 1
    mask = np.zeros(n, bool)
    flag = False
    for l in np.asarray(probe_row, np.int64).tolist():
        if l == -1:
            continue
        if not 0 <= l < n_lists:
            flag = True
            continue
        lo, hi = int(off[l]), int(off[l + 1])
        cl, ch = min(max(lo, 0), n), min(max(hi, 0), n)
        if cl != lo or ch != hi or hi < lo:
            flag = True
        if ch > cl:
            mask[cl:ch] = True
    return mask, flag


def ref_flat_search_lists(queries, vectors, list_off, probes, k, ip=False, allow=None):
    """queries [nq, d], vectors [n, d] f32 / f16 in list order, probes [nq, n_probe], allow None or bool [n] in position
    order -> (value [nq, k] f32, idx [nq, k] int64 positions, flag)"""
    q2 = np.atleast_2d(np.asarray(queries, np.float32))
    pr = np.atleast_2d(np.asarray(probes, np.int64))
    assert pr.shape[0] == q2.shape[0]
    n = np.asarray(vectors).shape[0]
    vals, idxs, flag = [], [], False
    for qi in range(q2.shape[0]):
        mask, bad = probed_mask(list_off, pr[qi], n)
        flag = flag or bad
        if allow is not None:
            mask &= np.asarray(allow, bool)
        v, i = fr.ref_flat_search(q2[qi:qi + 1], vectors, k, ip=ip, allow=mask)
        vals.append(v[0])
        idxs.append(i[0])
    return np.stack(vals), np.stack(idxs), flag


def offsets(lengths):
    """list lengths -> list_off int64 [n_lists + 1]"""
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return off
