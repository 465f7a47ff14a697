"""Reference of the exact search over resident vectors (include/pqhip.h: pqhip_flat_search_f32_dev) in numpy: by
definition the call is the exact re-ranking (rerank_ref.ref_rerank) with the allowed rows of the matrix, in ascending
order, as every query's candidate list.  Also a numpy model of the kernel's tile reduction, the transposed butterfly of
kernels_flat_search.hip.h: which lane keeps, sends and adds what at each step."""
import numpy as np

import rerank_ref as rr
from rerank_ref import assert_same   # noqa: F401  (re-exported for the tests)

TILES = (16,)          # every tile size kernels_flat_search.hip.h instantiates (kFlatTile)


def mask_words(allow):
    """bool [n] -> the mask words of the searches' `allow=`: int32 [ceil(n / 32)], bit r & 31 of word r >> 5"""
    a = np.asarray(allow, bool)
    bits = np.zeros(-(-a.size // 32) * 32, np.uint8)
    bits[:a.size] = a
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32).view(np.int32)


def words_allow(words, n):
    """the inverse: mask words -> bool [n]; bits beyond n are ignored"""
    w = np.asarray(words).view(np.uint32)
    r = np.arange(n)
    return ((w[r >> 5] >> (r & 31).astype(np.uint32)) & 1).astype(bool)


def ref_flat_search(queries, vectors, k, ip=False, allow=None):
    """queries [nq, d] (or [d]), vectors [n, d] f32 / f16, allow None or bool [n] -> (value [nq, k] f32, idx [nq, k] int64)"""
    q2 = np.atleast_2d(np.asarray(queries, np.float32))
    x = np.asarray(vectors)
    n = x.shape[0]
    rows = np.arange(n, dtype=np.int64) if allow is None else np.flatnonzero(np.asarray(allow, bool)).astype(np.int64)
    if rows.size == 0:
        rows = np.array([-1], np.int64)              # padding only
    cand = np.broadcast_to(rows, (q2.shape[0], rows.size))
    v, i, flag = rr.ref_rerank(q2, x, cand, k, ip=ip)
    assert not flag
    return v, i


# ---- the kernel's reduction schedule ------------------------------------------------------------------------------------
def lane_partials(query, rows, ip=False):
    """[n, 64] f32: the 64 lane chains of every row, before the tree (the first half of rerank_ref.row_values)"""
    q = np.asarray(query, np.float32)
    x = rr.as_f32(rows)
    n, d = x.shape
    p = np.zeros((n, 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, d, 64):
            w = min(64, d - j0)
            if ip:
                term = q[j0:j0 + w] * x[:, j0:j0 + w]
            else:
                t = q[j0:j0 + w] - x[:, j0:j0 + w]
                term = t * t
            p[:, :w] = p[:, :w] + term
    return p


def _fold(a, b, s):
    """One transposed step on two registers a, b [64] (one value per lane): lanes with bit s clear keep a and receive a of
    lane l ^ s, the others keep b and receive b of lane l ^ s; then one add, keep + received."""
    lane = np.arange(64)
    hi = (lane & s) != 0
    keep = np.where(hi, b, a)
    send = np.where(hi, a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        return (keep + send[lane ^ s]).astype(np.float32)


def tile_reduce(p, tile=16):
    """p [tile, 64]: the lane partials of the tile's rows -> [64], what each lane holds after the kernel's reduction:
    log2(tile) transposed steps (register u folded with u + half at s = 32, 16, ..), then plain xor exchanges of the one
    register that is left."""
    assert tile in TILES and p.shape == (tile, 64)
    regs = [p[u].astype(np.float32) for u in range(tile)]
    s = 32
    while len(regs) > 1:
        half = len(regs) // 2
        regs = [_fold(regs[u], regs[u + half], s) for u in range(half)]
        s >>= 1
    v = regs[0]
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        while s >= 1:
            v = (v + v[lane ^ s]).astype(np.float32)
            s >>= 1
    return v


def tile_lane_of_row(u, tile=16):
    """the first lane that holds row u of the tile after tile_reduce: the lane that offers it"""
    return u * (64 // tile)


def model_row_values(query, rows, ip=False, tile=16):
    """[n] f32: the value of every row as the kernel forms it, tile by tile (rows past the end: zero partials)"""
    p = lane_partials(query, rows, ip=ip)
    n = p.shape[0]
    out = np.zeros(n, np.float32)
    for r0 in range(0, n, tile):
        t = np.zeros((tile, 64), np.float32)
        m = min(tile, n - r0)
        t[:m] = p[r0:r0 + m]
        v = tile_reduce(t, tile)
        group = 64 // tile
        for u in range(m):
            lanes = v[u * group:(u + 1) * group]
            assert lanes.view(np.uint32).tolist() == [lanes[:1].view(np.uint32)[0]] * group or np.isnan(lanes).all()
            out[r0 + u] = v[tile_lane_of_row(u, tile)]
    return out
