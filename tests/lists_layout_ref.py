"""Reference of the list layout (include/pqhip.h: pqhip_lists_layout_dev), written element by element from its
definition: ids is the stable argsort of the assignments, list_off the prefix sums of the list sizes,
positions[ids[p]] = p, lists[p] = assign[ids[p]].  Plain Python loops over numpy arrays; pinned against
qmatrix.ivf_layout by tests/test_index_build.py.  Also the assignment patterns the tests share."""
import numpy as np


def ref_layout(assign, n_lists):
    """assign [n] -> (ids [n], list_off [n_lists + 1], positions [n], lists [n]), all int64"""
    a = np.asarray(assign).astype(np.int64)
    n = a.size
    if n and (a.min() < 0 or a.max() >= n_lists):
        raise ValueError("list ids must lie in [0, %d)" % n_lists)
    sizes = np.zeros(n_lists, np.int64)
    for v in a:
        sizes[v] += 1
    list_off = np.zeros(n_lists + 1, np.int64)
    for l in range(n_lists):
        list_off[l + 1] = list_off[l] + sizes[l]
    nxt = list_off[:-1].copy()              # the next free position of every list: rows are placed in row order
    ids = np.zeros(n, np.int64)
    positions = np.zeros(n, np.int64)
    lists = np.zeros(n, np.int64)
    for r in range(n):
        p = nxt[a[r]]
        nxt[a[r]] += 1
        ids[p], positions[r], lists[p] = r, p, a[r]
    return ids, list_off, positions, lists


PATTERNS = ("uniform", "one_list", "ascending", "descending", "runs64", "runs65", "alternating", "edges")


def pattern(kind, n, n_lists, rng):
    """n list ids in [0, n_lists) of one of the PATTERNS (int64)"""
    r = np.arange(n, dtype=np.int64)
    if kind == "uniform":
        return rng.integers(0, n_lists, n).astype(np.int64)
    if kind == "one_list":                       # every rank carries across waves, tiles and workgroups
        return np.full(n, int(rng.integers(0, n_lists)), np.int64)
    if kind == "ascending":
        return r * n_lists // max(n, 1)
    if kind == "descending":
        return n_lists - 1 - r * n_lists // max(n, 1)
    if kind in ("runs64", "runs65"):             # runs of exactly 64 / 65 equal ids, the id changing from run to run
        run = 64 if kind == "runs64" else 65
        return (r // run) * 7919 % n_lists
    if kind == "alternating":
        lo, hi = int(rng.integers(0, n_lists)), int(rng.integers(0, n_lists))
        return np.where(r % 2 == 0, lo, hi).astype(np.int64)
    if kind == "edges":                          # only the first and the last list are non-empty
        return np.where(rng.random(n) < 0.5, 0, n_lists - 1).astype(np.int64)
    raise ValueError(kind)
