"""k_encode_mfma16<8, 20, *>: the two smallest from block and column minima.

The screen's loop keeps, per (lane, row block), the minimum of every 16 x 16 block and of every accumulator column v, and
builds the smallest key and a lower bound of every other value from them.  A lane holds the values of centroids
16 cb + 4 q + v (block cb, lane group q, v = 0 .. 3) of its row, so where the two nearest centroids c, c' of a row sit
decides which side of the rule sees the second one.  Rows are planted at the midpoint of c and c', and one f16 step
(of the largest component of c' - c) off it towards either, with

    c ^ c' in {1, 2, 3}            same block and lane group, another v: the column side
    c' = c + 16 j, j = 1 and far   same lane group and v, another block: the block side (far: 15, or 13 for K = 225,
                                   where block 15 is padding and block 14 holds one centroid)
    another lane group             the merge

every pair in all four lane groups, in both row blocks and in both tiles of a trip.  In the codebook c' lies beside c
(a quarter of the spread away), so that the two are the nearest centroids of their midpoint; a CPU test checks with the
oracle that every planted row's code is c or c' and that both occur.  A second codebook has duplicated
centroids (same block and lane group, same block, another block with the same and with another lane group): rows equal
to them tie exactly and the code is the lower index.  Rows equal to a centroid are planted under both codebooks.

n = 20,000 has rows_per_item 32 (one tile per wave, both running minima start fresh); n = 204,800 + 13 has 64, so a
wave's second tile must start its minima anew (test_gpu_encode_screen_trips.py has the formula).  Codes are compared with
the oracle's exactly, for both index widths; the output is pre-filled with a value no code can take and carries 64 rows
past n that must keep it."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

M, DSUB = 3, 20
N_SMALL, N_TRIP = 20_000, 204_800 + 13
SLOTS = [3, 19, 35, 51]                      # offsets in a trip of 64 rows: both row blocks of both tiles
DUPS = [(132, 134), (148, 156), (181, 197), (143, 207), (147, 200)]


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


def test_sizes():
    assert _rows_per_item(N_SMALL) == 32 and _rows_per_item(N_TRIP) == 64
    for lo, hi in DUPS:
        assert lo < hi < 225
    assert [(lo ^ hi) < 4 for lo, hi in DUPS] == [True, False, False, False, False]
    assert [lo >> 4 == hi >> 4 for lo, hi in DUPS] == [True, True, False, False, False]
    assert [(lo >> 2) & 3 == (hi >> 2) & 3 for lo, hi in DUPS] == [True, False, True, True, False]
    for K in (256, 225):
        used = [c for pair in _pairs(K) + DUPS for c in pair]
        assert len(set(used)) == len(used)


def test_planted_pairs_are_the_nearest():
    # the oracle's code of every row planted between c and c' is one of the two, and both occur
    for K in (256, 225):
        q, x, want, planted = _case(K, False, N_SMALL)
        pairs = _pairs(K)
        seen = set()
        for i, (c, c2) in enumerate(pairs):
            rows = [64 * (2 + 3 * i + o) + s for o in range(3) for s in SLOTS]
            assert np.isin(want[rows], (c, c2)).all(), (K, c, c2)
            seen |= set(want[rows].ravel().tolist())
        assert seen == {c for pair in pairs for c in pair}


def _pairs(K):
    """(c, c') by position, every kind in every lane group q, c the lower index or the higher one in turn; no centroid
    is in two pairs or in DUPS"""
    far = 15 if K == 256 else 13
    out = []
    for q in range(4):
        for kind in range(7):
            i = 7 * q + kind
            cb, v = 1 + kind, (i + q) % 4                        # blocks 1 .. 7, one per kind
            c = 16 * cb + 4 * q + v
            if kind < 3:
                c2 = c ^ (kind + 1)
            elif kind == 3:
                c2 = c + 16
            elif kind == 4:
                c, c2 = 4 * q + v, 4 * q + v + 16 * far          # block 0 and the last block with this centroid
            elif kind == 5:
                c, c2 = 16 * cb + 4 * q + q, 16 * cb + 4 * ((q + 1) % 4) + q      # same block, the next lane group
            else:
                c2 = 16 * (cb + 3) + 4 * ((q + 2) % 4) + (v + 1) % 4
            assert 0 <= c < K and 0 <= c2 < K and c != c2, (K, q, kind, c, c2)
            out.append((c, c2) if i % 2 == 0 else (c2, c))
    return out


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


_shared = {}


def _base(K, dup, n_rows):
    """codebook, shared rows and their reference codes, once per (K, codebook)"""
    if "x" not in _shared:
        _shared["x"] = synth.normalish(9102, (N_TRIP, M * DSUB))
        _shared["x"].setflags(write=False)
    key = (K, dup)
    if key not in _shared:
        q = np.ascontiguousarray(synth.normalish(9101, (M, 256, DSUB))[:, :K])
        near = synth.normalish(9103, (M, 256, DSUB)) * np.float32(0.25)
        for c, c2 in _pairs(K):                                  # c' beside c: the two nearest centroids of their midpoint
            q[:, c2] = q[:, c] + near[:, c2]
        if dup:
            for lo, hi in DUPS:
                q[:, hi] = q[:, lo]
        want = orc.quantize_batch(q, _shared["x"][:n_rows], n_threads=8)
        want.setflags(write=False)
        _shared[key] = (q, want)
    q, want = _shared[key]
    if len(want) < n_rows:                                       # the longer reference replaces the shorter one
        want = orc.quantize_batch(q, _shared["x"][:n_rows], n_threads=8)
        want.setflags(write=False)
        _shared[key] = (q, want)
    return q, want, _shared["x"]


def _f16_step(t):
    """one f16 step at |t| (normal range), exact in float32"""
    return np.float32(2.0 ** (int(np.floor(np.log2(abs(float(t))))) - 10))


def _plant(x, q):
    """writes the planted rows into x; returns their sorted positions"""
    K = q.shape[1]
    pos = []
    trip = 2                                                     # the planted trips start at row 128
    for c, c2 in _pairs(K):
        for off in (0, 1, -1):                                   # the midpoint, a step towards c', a step towards c
            for s in SLOTS:
                p = 64 * trip + s
                for m in range(M):
                    a, b = q[m, c], q[m, c2]
                    mid = (a + b) * np.float32(0.5)
                    j = int(np.argmax(np.abs(b - a)))
                    mid[j] += np.float32(off) * np.sign(b[j] - a[j]) * _f16_step(mid[j] if mid[j] != 0 else b[j])
                    x[p, m * DSUB:(m + 1) * DSUB] = mid
                pos.append(p)
            trip += 1
    cents = [c for pair in DUPS for c in pair] + [0, 15, 16, 131, 208, 224, K - 1]
    for c in cents:                                              # rows equal to a centroid, duplicated or not
        for s in SLOTS:
            p = 64 * trip + s
            for m in range(M):
                x[p, m * DSUB:(m + 1) * DSUB] = q[m, c]
            pos.append(p)
        trip += 1
    assert 64 * trip < N_SMALL - 64
    return np.array(sorted(pos), np.int64)


def _case(K, dup, n):
    q, want_base, x_base = _base(K, dup, N_TRIP if n > N_SMALL else N_SMALL)
    x = x_base[:n].copy()
    planted = _plant(x, q)
    want = want_base[:n].copy()
    want[planted] = orc.quantize_batch(q, np.ascontiguousarray(x[planted]))
    return q, x, want, planted


def _run(ra, K, dup, n):
    import torch
    q, x, want, planted = _case(K, dup, n)
    if dup:                                                      # the exact ties are there and go to the lower index
        hi = np.array([h for _, h in DUPS])
        assert not np.isin(want, hi).any()
        assert np.isin(want[planted], [lo for lo, _ in DUPS]).any()
    xd = torch.from_numpy(x).to("cuda:0")
    for dt in (torch.uint8, torch.int32):
        fill = 255 if dt == torch.uint8 else -1
        out = torch.full((n + 64, M), fill, dtype=dt, device=xd.device)
        pq = ra.Pq(None, q)
        pq.quantize_batch_device(xd, out=out[:n])
        torch.cuda.synchronize()
        assert pq.last_encode_kernel().startswith("k_encode_mfma16"), pq.last_encode_kernel()
        got = out.cpu().numpy()
        assert (got[n:] == fill).all(), "rows past n were written"
        codes = got[:n] if dt == torch.uint8 else got[:n].view(np.uint32)
        bad = np.argwhere(codes != want)
        assert bad.size == 0, (str(dt), len(bad), bad[:5].tolist(), codes[tuple(bad[0])], want[tuple(bad[0])],
                               np.isin(bad[:, 0], planted).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_SMALL, N_TRIP])
@pytest.mark.parametrize("K", [256, 225])
def test_planted_pairs(ra, K, n):
    _run(ra, K, False, n)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
def test_duplicated_centroids(ra, K):
    _run(ra, K, True, N_SMALL)
