"""Reference of the list merge (include/pqhip.h: pqhip_lists_merge_dev), by its definition: list l of the output is list l of
`a` followed by list l of `b`.  Pure numpy; pinned against ivf_layout by tests/test_lists_merge.py."""
import numpy as np


def ref_valid(off, n):
    """the validity rule of an offset array: off[0] == 0, non-decreasing, off[n_lists] == n"""
    off = np.asarray(off, dtype=np.int64)
    return bool(off.ndim == 1 and off.size >= 1 and off[0] == 0 and off[-1] == n and np.all(off[1:] >= off[:-1]))


def ref_merge(off_a, a, off_b, b):
    """a [n_a, ...] in list order under off_a [L + 1], b likewise under off_b -> (out [n_a + n_b, ...], off_out [L + 1])"""
    off_a = np.asarray(off_a, dtype=np.int64)
    off_b = np.asarray(off_b, dtype=np.int64)
    assert off_a.shape == off_b.shape and ref_valid(off_a, a.shape[0]) and ref_valid(off_b, b.shape[0])
    parts = []
    for l in range(off_a.size - 1):
        parts.append(a[off_a[l]:off_a[l + 1]])
        parts.append(b[off_b[l]:off_b[l + 1]])
    out = np.concatenate(parts) if parts else np.concatenate([a, b])
    return out, off_a + off_b


def random_offsets(rng, n, n_lists, shape="random"):
    """offsets [n_lists + 1] of n rows: "random" (multinomial over a random subset of the lists, so some are empty), "edges"
    (first and last list empty), "heavy" (one list holds 90 % of the rows)"""
    sizes = np.zeros(n_lists, np.int64)
    if n_lists == 1:
        sizes[0] = n
    elif shape == "heavy":
        big = int(rng.integers(n_lists))
        sizes[big] = (n * 9) // 10
        sizes += rng.multinomial(n - sizes[big], np.full(n_lists, 1.0 / n_lists))
    else:
        live = rng.random(n_lists) < 0.7
        if shape == "edges":
            live[0] = live[-1] = False
        if not live.any():
            live[n_lists // 2] = True
        p = live * rng.random(n_lists)
        sizes = rng.multinomial(n, p / p.sum()).astype(np.int64)
    off = np.zeros(n_lists + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    return off
