"""k_encode_mfma16<8, 20, *>: the trip of two tiles and its one merge.

The screen body walks a wave's rows in trips of 64 (two 32-row tiles) and merges the four lane groups once per trip, one
row per lane.  The other screen tests use 3 - 20 k rows, where rows_per_item is 32 and a wave has a single tile: the
second tile of a trip, the seam between trips and the odd tail tile never run there.  These sizes reach them
(rows_per_item = clamp(round_up(ceil(n M / 16384), 32), 32, 1024), launch_mfma in pqhip_encode.hip):

    n = 204,800 + r   rows_per_item  64   one full trip per wave
    n = 384,000 + r   rows_per_item  96   a trip and an odd tile
    n = 600,000 + r   rows_per_item 128   two trips

with r in {0, 13, 32 + 17, 64 + 5}, so that the ragged end falls in a first row block, in the second tile's second row
block, and (rows_per_item 96) in the odd tail tile.  Rows that leave the screen are planted at every offset modulo 64
that starts or ends a row block (0, 15, 16, 31, 32, 47, 48, 63), in the odd tail tile and in the second trip, and
over the last 70 rows: rows with a huge norm in one sub-vector (the exact path of rows outside the f16 range), rows
equal to a centroid and midpoints of two centroids (the candidate path).  Every lane-to-row mapping and both halves of
the 64-bit ballots are exercised.

The calls go through quantize_batch_device: one launch over all n rows, so n alone decides rows_per_item (the
host-buffer entry point encodes a large batch chunk by chunk).  The oracle encodes rows independently, so the
reference of the shared rows is computed once per K and only the planted rows are encoded again per case.  A 32-bit
code has the value of the 8-bit one (K <= 256), so one reference serves both index widths.  The output buffer is
pre-filled with a value no code can take (255 is a code only when K = 256 and the width is 8 bits), and carries 64
rows past n that must keep it."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

M, DSUB = 3, 20
N_MAX = 600_000 + 64 + 5
SIZES = [(204_800, 64), (384_000, 96), (600_000, 128)]
RAGGED = [0, 13, 32 + 17, 64 + 5]
BLOCK_EDGES = [0, 15, 16, 31, 32, 47, 48, 63]


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


def test_sizes_reach_the_trips():
    for base, rpi in SIZES:
        for r in RAGGED:
            assert _rows_per_item(base + r) == rpi, (base, r)
    assert _rows_per_item(20_000) == 32          # the other screen tests: one tile per wave


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


_shared = {}


def _base(K):
    """codebook, shared rows and their reference codes, once per K"""
    if K not in _shared:
        q = np.ascontiguousarray(synth.normalish(8101, (M, 256, DSUB))[:, :K])
        if "x" not in _shared:
            _shared["x"] = synth.normalish(8102, (N_MAX, M * DSUB))
            _shared["x"].setflags(write=False)
        want = orc.quantize_batch(q, _shared["x"], n_threads=8)
        want.setflags(write=False)
        _shared[K] = (q, want)
    return _shared[K] + (_shared["x"],)


def _plant(x, q, n, rpi):
    """writes the planted rows into x[:n]; returns their sorted positions"""
    K = q.shape[1]
    offs = list(BLOCK_EDGES)
    if rpi == 96:
        offs += [64, 79, 80, 95]                  # the odd tail tile
    if rpi == 128:
        offs += [64, 64 + 31, 64 + 32, 127]       # the second trip
    waves = n // rpi                              # waves with all their rows
    pos = {}
    i = 0
    for kind in range(3):
        for o in offs:
            w = (0, waves - 1)[i % 2] if i < 2 else (11 + 37 * i) % waves
            pos[w * rpi + o] = kind
            i += 1
    for p in range(n - 70, n):                    # the ragged end, both tiles of its trip
        pos[p] = p % 3
    for p, kind in pos.items():
        if kind == 0:                             # scaled norm beyond 2^30 in one sub-vector
            m = p % M
            x[p, m * DSUB:(m + 1) * DSUB] *= np.float32(2.0 ** 14)
        elif kind == 1:                           # a centroid
            for m in range(M):
                x[p, m * DSUB:(m + 1) * DSUB] = q[m, (7 * p + m) % K]
        else:                                     # the midpoint of two centroids
            for m in range(M):
                a, b = (5 * p + m) % K, (11 * p + 1) % K
                if a == b:
                    b = (b + 1) % K
                x[p, m * DSUB:(m + 1) * DSUB] = (q[m, a] + q[m, b]) * np.float32(0.5)
    return np.array(sorted(pos), np.int64)


def _case(K, n, rpi):
    q, want_base, x_base = _base(K)
    x = x_base[:n].copy()
    planted = _plant(x, q, n, rpi)
    want = want_base[:n].copy()
    want[planted] = orc.quantize_batch(q, np.ascontiguousarray(x[planted]))
    return q, x, want


def _encode(ra, torch, pq, xd, n, dt, make_out):
    fill = 255 if dt == torch.uint8 else -1
    full, out = make_out(n + 64, dt, fill)
    pq.quantize_batch_device(xd, out=out[:n])
    torch.cuda.synchronize()
    assert pq.last_encode_kernel().startswith("k_encode_mfma16"), pq.last_encode_kernel()
    got = out.cpu().numpy()
    assert (got[n:] == fill).all(), "rows past n were written"
    codes = got[:n] if dt == torch.uint8 else got[:n].view(np.uint32)
    return full, codes, fill


def _compare(codes, want, what):
    bad = np.argwhere(codes != want)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), codes[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 250])
@pytest.mark.parametrize("r", RAGGED)
@pytest.mark.parametrize("base,rpi", SIZES)
def test_trips(ra, base, rpi, r, K):
    import torch
    n = base + r
    q, x, want = _case(K, n, rpi)
    xd = torch.from_numpy(x).to("cuda:0")

    def make_out(rows, dt, fill):
        t = torch.full((rows, M), fill, dtype=dt, device=xd.device)
        return t, t

    for dt in (torch.uint8, torch.int32):
        for v in (0, 9):
            pq = ra.Pq(None, q)
            if v:
                pq.set_encode_variant(v)
            _, codes, _ = _encode(ra, torch, pq, xd, n, dt, make_out)
            _compare(codes, want, (str(dt), v))


@pytest.mark.gpu
def test_trips_column_sliced(ra):
    # x_rs > d and o_rs > M: a trip and an odd tile per wave, the ragged end in the second tile
    import torch
    base, rpi = SIZES[1]
    n = base + 32 + 17
    q, x, want = _case(256, n, rpi)
    d = M * DSUB
    xf = torch.zeros((n, d + 12), dtype=torch.float32, device="cuda:0")
    xf[:, 4:4 + d] = torch.from_numpy(x).to("cuda:0")
    xd = xf[:, 4:4 + d]
    assert xd.stride(0) == d + 12

    def make_out(rows, dt, fill):
        t = torch.full((rows, M + 5), fill, dtype=dt, device=xd.device)
        return t, t[:, 1:1 + M]

    for dt in (torch.uint8, torch.int32):
        for v in (0, 9):
            pq = ra.Pq(None, q)
            if v:
                pq.set_encode_variant(v)
            full, codes, fill = _encode(ra, torch, pq, xd, n, dt, make_out)
            _compare(codes, want, (str(dt), v))
            full = full.cpu().numpy()
            assert (full[:, :1] == fill).all() and (full[:, 1 + M:] == fill).all(), "columns outside the slice were written"
