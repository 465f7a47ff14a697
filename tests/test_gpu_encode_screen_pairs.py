"""k_encode_mfma16<8, 20, *>: the few-candidate rows, listed in the trip's merge and resolved one row per lane
(DESIGN.md §5, K1m16, round 10).

A row off the screen whose candidates sit in different lane groups (centroid j is in lane group (j >> 2) & 3) goes to a
per-wave list of 96 entries and is resolved by encode_rows_few from the merge's four keys; a row with two candidates in
one lane group, or one that finds the list full, keeps the candidate path.  Planted, in a codebook built for it:

    mid     the midpoint of centroids a and a + 4 (neighbouring lane groups), a chosen so that the oracle picks one of them
    tri     a point at the same distance (0.25 along three different axes) from centroids in lane groups 0, 1, 2
    quad    the same for four centroids, one per lane group
    near    tri / quad points moved by 2^-12 along one axis: nearly equidistant
    shared  three such centroids of which two share a lane group: the candidate path
    dup     a row equal to a centroid that exists twice, in different lane groups (10 / 197, and 14 / 96, where the
            lower index sits in the higher lane group): the exact tie goes to the lower index
    cen     a row equal to a centroid
    pad     the midpoint of centroid 224 and one of 220 .. 223 (a set of five, one unit from a centre along five axes,
            so that a midpoint has two candidates): with K = 225 every neighbour of 224 in its block and every later
            position is padding

at every row-block edge of both tiles of a trip in the first, a middle and the last whole wave, over the ragged end, and
in one case as a whole wave of 128 few-candidate rows (the list overflows and the rest falls back), once as the first
wave and once as the last, ragged one (109 rows).  Sizes as in test_gpu_encode_screen_trips.py: rows_per_item 32, 64 and
128.  The reference of the shared rows is computed once per K; the output is pre-filled and carries 64 guard rows."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

M, DSUB = 3, 20
SIZES = [(20_000, 32), (204_800 + 13, 64), (600_000 + 13, 128), (600_000 + 45, 128)]
N_MAX = 600_000 + 45
BLOCK_EDGES = [0, 15, 16, 31, 32, 47, 48, 63]
TRI = [16 * 2 + 4 * 0 + 1, 16 * 5 + 4 * 1 + 3, 16 * 9 + 4 * 2 + 0]
QUAD = [16 * 1 + 4 * 0 + 2, 16 * 7 + 4 * 1 + 0, 16 * 11 + 4 * 2 + 3, 16 * 12 + 4 * 3 + 1]
SHARED = [16 * 3 + 4 * 1 + 0, 16 * 8 + 4 * 1 + 2, 16 * 4 + 4 * 3 + 1]
PAD = [220, 221, 222, 223, 224]              # one unit from a centre of their own, along five axes
DUPS = [(10, 197), (14, 96)]
KINDS = ["mid", "tri", "quad", "near", "shared", "dup", "cen", "pad"]
FEW_KINDS = ["mid", "tri", "quad", "near", "dup", "pad"]


def _group(j):
    return (j >> 2) & 3


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


def _codebook(K):
    """the shared random codebook with the planted centroids; the centres of the tri / quad / shared sets"""
    q = np.ascontiguousarray(synth.normalish(8301, (M, 256, DSUB))[:, :K]).copy()
    centres = synth.normalish(8302, (4, M, DSUB))
    for s, idx in enumerate((TRI, QUAD, SHARED, PAD)):
        for i, j in enumerate(idx):
            q[:, j] = centres[s]
            q[:, j, 3 + 4 * i] += np.float32(1.0 if idx is PAD else 0.25)   # a different axis for every centroid of the set
    for lo, hi in DUPS:
        q[:, hi] = q[:, lo]
    return q, centres


_shared = {}


def _book(K):
    """codebook, centres and the good midpoints, once per K"""
    if ("q", K) not in _shared:
        q, centres = _codebook(K)
        # midpoints of a and a + 4 that the oracle gives to a or a + 4 in every sub-vector
        a = np.arange(K - 8)
        mids = ((q[:, a] + q[:, a + 4]) * np.float32(0.5)).transpose(1, 0, 2).reshape(len(a), M * DSUB)
        got = orc.quantize_batch(q, np.ascontiguousarray(mids))
        good = a[((got == a[:, None]) | (got == a[:, None] + 4)).all(axis=1)]
        assert len(good) >= 32, len(good)
        _shared["q", K] = (q, centres, good)
    return _shared["q", K]


def _base(K):
    """shared rows and their reference codes, once per K"""
    if K not in _shared:
        if "x" not in _shared:
            _shared["x"] = synth.normalish(8303, (N_MAX, M * DSUB))
            _shared["x"].setflags(write=False)
        want = orc.quantize_batch(_book(K)[0], _shared["x"], n_threads=8)
        want.setflags(write=False)
        _shared[K] = want
    return _shared[K], _shared["x"]


def _row(kind, p, q, centres, good):
    """the planted row number p of a kind: the row and, per sub-vector, the centroids it may be given to"""
    K = q.shape[1]
    x = np.empty((M, DSUB), np.float32)
    allowed = []
    for m in range(M):
        if kind == "mid":
            a = int(good[(5 * p + m) % len(good)])
            x[m], al = (q[m, a] + q[m, a + 4]) * np.float32(0.5), {a, a + 4}
        elif kind in ("tri", "quad", "shared", "near"):
            s = {"tri": 0, "quad": 1, "shared": 2, "near": (p + m) % 2}[kind]
            x[m], al = centres[s, m], set((TRI, QUAD, SHARED)[s])
            if kind == "near":
                x[m, 3 + 4 * (p % len(al))] += np.float32(2.0 ** -12)
        elif kind == "dup":
            lo, hi = DUPS[(p + m) % 2]
            x[m], al = q[m, lo], {lo}
        elif kind == "cen":
            j = (7 * p + m) % K
            x[m], al = q[m, j], {j} | {lo for lo, hi in DUPS if hi == j}
        else:
            b = 220 + (p + m) % 4
            x[m], al = (q[m, 224] + q[m, b]) * np.float32(0.5), {224, b}
        allowed.append(al)
    return x.reshape(M * DSUB), allowed


def _positions(n, rpi, overflow):
    """row -> kind"""
    offs = [o for o in BLOCK_EDGES if o < rpi]
    if rpi == 128:
        offs += [64 + o for o in BLOCK_EDGES]                  # the second trip
    waves = n // rpi
    pos = {}
    for w in (0, waves // 2 + 3, waves - 1):
        for i, o in enumerate(offs):
            for k in range(len(KINDS)):                        # every kind at every edge, over 8 neighbouring waves
                pos[((w + k) % waves) * rpi + o] = KINDS[(i + k) % len(KINDS)]
    for p in range(n - 70, n):                                 # the ragged end
        pos[p] = KINDS[p % len(KINDS)]
    if overflow == "first":
        for p in range(0, rpi):
            pos[p] = FEW_KINDS[p % len(FEW_KINDS)]
    elif overflow == "last":
        for p in range((n - 1) // rpi * rpi, n):
            pos[p] = FEW_KINDS[p % len(FEW_KINDS)]
    return pos


_cases = {}


def _planted(K, n, rpi, overflow):
    """the planted rows of a case: positions, rows, reference codes, allowed centroids"""
    key = (K, n, overflow)
    if key not in _cases:
        q, centres, good = _book(K)
        pos = _positions(n, rpi, overflow)
        rows = np.array(sorted(pos), np.int64)
        built = [_row(pos[p], p, q, centres, good) for p in rows]
        xr = np.stack([b[0] for b in built])
        _cases[key] = (rows, xr, orc.quantize_batch(q, np.ascontiguousarray(xr)), [b[1] for b in built])
    return _cases[key]


def _case(K, n, rpi, overflow):
    rows, xr, wr, _ = _planted(K, n, rpi, overflow)
    want_base, x_base = _base(K)
    x, want = x_base[:n].copy(), want_base[:n].copy()
    x[rows], want[rows] = xr, wr
    return _book(K)[0], x, want, rows


CASES = [(n, rpi, None) for n, rpi in SIZES] + [(600_000 + 13, 128, "first"), (600_000 + 45, 128, "last")]


def test_sizes_and_lane_groups():
    for n, rpi in SIZES:
        assert _rows_per_item(n) == rpi, n
    assert (600_000 + 45) % 128 == 109 and (600_000 + 13) % 128 == 77     # the ragged waves: above and below the list's 96
    assert sorted(_group(j) for j in TRI) == [0, 1, 2] and sorted(_group(j) for j in QUAD) == [0, 1, 2, 3]
    assert sorted(_group(j) for j in SHARED) == [1, 1, 3]
    assert [(_group(lo), _group(hi)) for lo, hi in DUPS] == [(2, 1), (3, 0)]
    assert max(TRI + QUAD + SHARED + [j for d in DUPS for j in d]) < 220 and len(set(TRI + QUAD + SHARED + PAD + [j for d in DUPS for j in d])) == 19
    assert _group(224) == 0 and all(_group(j) == 3 for j in range(220, 224))


@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n,rpi,overflow", [CASES[0], CASES[4], CASES[5]])
def test_planted_rows_go_to_their_centroids(n, rpi, overflow, K):
    # the oracle gives every planted row to one of its planted centroids, in every sub-vector
    rows, _, want, allowed = _planted(K, n, rpi, overflow)
    for r, w, al in zip(rows, want, allowed):
        for m in range(M):
            assert int(w[m]) in al[m], (int(r), m, int(w[m]), sorted(al[m]))
    assert len(rows) >= (100 if rpi == 32 else 128)


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n,rpi,overflow", CASES)
def test_pairs(ra, n, rpi, overflow, K):
    import torch
    q, x, want, rows = _case(K, n, rpi, overflow)
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
                               int(np.isin(bad[:, 0], rows).sum()))
