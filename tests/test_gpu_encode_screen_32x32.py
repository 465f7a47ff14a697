"""k_encode_mfma16<8, 20, *>: the screen on v_mfma_f32_32x32x16_f16, d = 300, M = 15.

A lane (row n32 = lane & 31, half h = lane >> 5) holds, per block b of 32 centroids, the 16 values of centroids
32 b + 8 (i >> 2) + 4 h + (i & 3), i the accumulator register.  For centroid j that is

    half h = (j >> 2) & 1,   half-block j >> 4,   column 4 ((j >> 3) & 1) + (j & 3),   register i = 4 ((j & 31) >> 3) + (j & 3)

and where the two nearest centroids c, c' of a row sit decides which part of the rule sees the second one.  Rows are
planted at the midpoint of c and c' and one f16 step off it to either side, c' beside c in the codebook, with c, c' in

    the same half-block (another column: c ^ 1, c ^ 3, c ^ 8)             the column side
    the same column, the other half-block of the block (c ^ 16)           the block side, one keep2
    the same column in another block (c + 32, and the last block)         the block side
    the other lane half (c ^ 4, and another block as well)                the merge; two candidates: the list
    registers 7 / 8 and 15 / 0 of a half, across a half-block edge        neighbours in the register file

each with c in half 0 and in half 1, at rows 0, 15, 16 and 31 of both tiles of a trip and over the ragged end.  Three
centroids at one distance (two of them in one half) take the candidate path, as do midpoints within a half;
duplicated centroids -- in one half-block, in one half, across the halves with the lower index in the lower and in the
higher half -- tie exactly and go to the lower index.  A wave of 128 midpoints across the halves overflows the list of 96
entries; waves whose other rows are centroids (decided by the screen) hold exactly 1, 16 and 17 rows for the candidate
path.  A NaN row, rows whose scaled norm is beyond kScreenMaxXX and a codebook whose norms are all below kScreenMinCC leave through the
exact path.  Sizes: the n of SMALL have rows_per_item 32, N64 has 64 and N128 128 (the formula of
test_gpu_encode_screen_trips.py, asserted below).  Codes are compared with the oracle's bit for bit; the output is
pre-filled with a value no code takes and carries 64 rows past n that must keep it."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

M, DSUB = 15, 20
SMALL = [1, 31, 32, 33, 63, 64, 65, 127, 160, 4 * 128 + 109]
N64, N128 = 36_032 + 45, 104_960 + 109
N_MAX = N128
EDGES = [0, 15, 16, 31, 32, 47, 48, 63]
DUPS = [(129, 131), (70, 198), (72, 205), (77, 200)]
TRI = [(16, 100, 24), (141, 10, 149)]       # the first and the third share a half; the second sits in the other


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


def _half(j):
    return (j >> 2) & 1


def _column(j):
    return 4 * ((j >> 3) & 1) + (j & 3)


def _reg(j):
    return 4 * ((j & 31) >> 3) + (j & 3)


def _pairs(K):
    """(kind, c, c') by position; every kind with c in half 0 and in half 1, c the lower or the higher index in turn; no
    centroid is in two pairs, in DUPS or in TRI"""
    last = 32 * ((K - 1) // 32 - (0 if K % 32 == 0 else 1))      # the last block that is full
    out = []
    for h in range(2):
        o = 4 * h                                                # the same registers in the other half
        out += [("col1", 32 + o, 33 + o), ("col3", 64 + o, 67 + o), ("col8", 34 + o, 42 + o), ("hblk", 98 + o, 114 + o),
                ("blk1", 130 + o, 162 + o), ("blkfar", 1 + o, last + 1 + o), ("r7r8", 171 + o, 176 + o),
                ("r15r0", 155 + o, 160 + o)]
    out += [("half", 51, 55), ("half", 87, 83), ("halfblk", 88, 156), ("halfblk", 124, 184)]
    return [(k, c, c2) if i % 2 == 0 else (k, c2, c) for i, (k, c, c2) in enumerate(out)]


def test_positions():
    assert [_rows_per_item(n) for n in SMALL] == [32] * len(SMALL)
    assert _rows_per_item(N64) == 64 and _rows_per_item(N128) == 128
    assert N64 % 64 == 45 and N128 % 128 == 109 and (4 * 128 + 109) % 32 == 13
    for K in (256, 225):
        pairs = _pairs(K)
        used = [c for _, c, c2 in pairs for c in (c, c2)] + [c for d in DUPS for c in d] + [c for t in TRI for c in t]
        assert len(set(used)) == len(used) and max(used) < (K if K == 256 else 224), sorted(used)
        for kind, c, c2 in pairs:
            same_half, same_hb, same_col = _half(c) == _half(c2), c >> 4 == c2 >> 4, _column(c) == _column(c2)
            if kind.startswith("col"):
                assert same_half and same_hb and not same_col
            elif kind == "hblk":
                assert same_half and not same_hb and c >> 5 == c2 >> 5 and same_col
            elif kind.startswith("blk"):
                assert same_half and c >> 5 != c2 >> 5 and same_col
            elif kind.startswith("half"):
                assert not same_half and same_col and (c >> 5 == c2 >> 5) == (kind == "half")
            elif kind == "r7r8":
                assert same_half and c >> 5 == c2 >> 5 and sorted((_reg(c), _reg(c2))) == [7, 8]
            else:
                assert same_half and abs((c >> 5) - (c2 >> 5)) == 1 and sorted((_reg(c), _reg(c2))) == [0, 15]
        assert {_half(c) for k, c, _ in pairs if k == "col1"} == {0, 1}
    # duplicates: one half-block; one half, other blocks; across the halves, the lower index in half 0 and in half 1
    assert [(lo >> 4 == hi >> 4, _half(lo), _half(hi)) for lo, hi in DUPS] == [(True, 0, 0), (False, 1, 1), (False, 0, 1), (False, 1, 0)]
    for t in TRI:
        assert len({_half(c) for c in t}) == 2


_shared = {}


def _book(K, dup):
    """the codebook: c' beside c for every pair, three centroids around a centre, duplicates"""
    if (K, dup) not in _shared:
        q = np.ascontiguousarray(synth.normalish(12101, (M, 256, DSUB))[:, :K]).copy()
        near = synth.normalish(12103, (M, 256, DSUB)) * np.float32(0.25)
        for _, c, c2 in _pairs(K):
            q[:, c2] = q[:, c] + near[:, c2]
        centres = synth.normalish(12104, (len(TRI), M, DSUB))
        for s, t in enumerate(TRI):
            for i, j in enumerate(t):
                q[:, j] = centres[s]
                q[:, j, 3 + 4 * i] += np.float32(0.25)
        if dup:
            for lo, hi in DUPS:
                q[:, hi] = q[:, lo]
        _shared[K, dup] = (q, centres)
    return _shared[K, dup]


def _base(K, dup):
    """shared rows and their reference codes, once per codebook"""
    if ("want", K, dup) not in _shared:
        if "x" not in _shared:
            _shared["x"] = synth.normalish(12102, (N_MAX, M * DSUB))
            _shared["x"].setflags(write=False)
        want = orc.quantize_batch(_book(K, dup)[0], _shared["x"], n_threads=8)
        want.setflags(write=False)
        _shared["want", K, dup] = want
    return _shared["want", K, dup], _shared["x"]


def _f16_step(t):
    return np.float32(2.0 ** (int(np.floor(np.log2(abs(float(t))))) - 10))


def _mid(q, c, c2, off):
    """the midpoint of c and c' in every sub-vector, `off` f16 steps towards c'"""
    x = np.empty((M, DSUB), np.float32)
    for m in range(M):
        a, b = q[m, c], q[m, c2]
        mid = (a + b) * np.float32(0.5)
        j = int(np.argmax(np.abs(b - a)))
        mid[j] += np.float32(off) * np.sign(b[j] - a[j]) * _f16_step(mid[j] if mid[j] != 0 else b[j])
        x[m] = mid
    return x.reshape(-1)


def _kinds(K, dup):
    """the planted row kinds of a codebook, as functions p -> row"""
    q, centres = _book(K, dup)
    out = []
    for _, c, c2 in _pairs(K):
        for off in (0, 1, -1):
            out.append(lambda p, c=c, c2=c2, off=off: _mid(q, c, c2, off))
    for s in range(len(TRI)):
        out.append(lambda p, s=s: centres[s].reshape(-1))
    for lo, hi in DUPS:
        out.append(lambda p, lo=lo, hi=hi: q[:, (lo, hi)[p % 2]].reshape(-1))
    out.append(lambda p: q[np.arange(M), (7 * p + np.arange(M)) % K].reshape(-1))       # a centroid per sub-vector
    return out


def _listed(K, dup, p):
    """a row with one candidate in each half: the midpoint of a pair across the halves"""
    across = [(c, c2) for k, c, c2 in _pairs(K) if k.startswith("half")]
    c, c2 = across[p % len(across)]
    return _mid(_book(K, dup)[0], c, c2, 0)


def _in_half(K, dup, p):
    """a row with two candidates in one half: the candidate path"""
    within = [(c, c2) for k, c, c2 in _pairs(K) if not k.startswith("half")]
    c, c2 = within[p % len(within)]
    return _mid(_book(K, dup)[0], c, c2, 0)


def _decided(K, dup, p):
    """a row the screen decides: a centroid that exists once"""
    taken = {c for d in DUPS for c in d}
    j = [(11 * p + m) % K for m in range(M)]
    j = [(c + 1) % K if c in taken else c for c in j]
    j = [(c + 1) % K if c in taken else c for c in j]
    return _book(K, dup)[0][np.arange(M), j].reshape(-1)


def _case(K, dup, n, special=None):
    """rows, reference codes and the planted positions"""
    rpi = _rows_per_item(n)
    q = _book(K, dup)[0]
    want_base, x_base = _base(K, dup)
    x = x_base[:n].copy()
    kinds = _kinds(K, dup)
    pos = {}
    offs = [o for o in EDGES if o < rpi] + ([64 + o for o in EDGES] if rpi == 128 else [])
    waves = -(-n // rpi)
    i = 0
    for w in sorted({0, waves // 2, max(waves - 2, 0)}):
        for r in range(-(-len(kinds) // len(offs)) + 1):         # every kind at some edge, over neighbouring waves
            for o in offs:
                p = ((w + r) % waves) * rpi + o
                if p < n:
                    pos[p] = kinds[i % len(kinds)]
                    i += 1
    for p in range(max(n - 70, 0), n):                           # the ragged end, both tiles of its trip
        pos[p] = kinds[(i + p) % len(kinds)]
    if special == "overflow":                                    # a whole wave of listed rows, the first and the last
        for p in list(range(0, rpi)) + list(range((n - 1) // rpi * rpi, n)):
            pos[p] = lambda p: _listed(K, dup, p)
    elif special == "counts":                                    # waves with exactly 1, 16 and 17 rows for the candidate path
        for w, k in ((3, 1), (5, 16), (7, 17)):
            chosen = [(5 * t + 2) % rpi for t in range(k)]
            assert len(set(chosen)) == k
            for r in range(rpi):
                p = w * rpi + r
                pos[p] = (lambda p: _in_half(K, dup, p)) if r in chosen else (lambda p: _decided(K, dup, p))
    elif special == "exact":                                     # a NaN row, rows beyond kScreenMaxXX
        for t, p in enumerate(sorted({0, 15, 16, 31, n // 2, n - 1} & set(range(n)))):
            if t % 2 == 0:
                pos[p] = lambda p: x_base[p] * np.float32(2.0 ** 14)
            else:
                def nan_row(p):
                    r = x_base[p].copy()
                    r[(p % M) * DSUB + p % DSUB] = np.float32(np.nan)
                    return r
                pos[p] = nan_row
    rows = np.array(sorted(pos), np.int64)
    if len(rows):
        x[rows] = np.stack([pos[p](int(p)) for p in rows])
    want = want_base[:n].copy()
    if len(rows):
        want[rows] = orc.quantize_batch(q, np.ascontiguousarray(x[rows]))
    return q, x, want, rows


def test_planted_rows_on_the_host():
    # the oracle gives every midpoint to one of its two centroids, both occur, and the exact ties go to the lower index
    for K in (256, 225):
        q = _book(K, True)[0]
        for kind, c, c2 in _pairs(K):
            got = orc.quantize_batch(q, np.stack([_mid(q, c, c2, off) for off in (0, 1, -1)]))
            assert np.isin(got, (c, c2)).all(), (K, kind, c, c2)
            assert {c, c2} <= set(got.ravel().tolist()), (K, kind, c, c2)
        for lo, hi in DUPS:
            got = orc.quantize_batch(q, np.stack([q[:, lo].reshape(-1), q[:, hi].reshape(-1)]))
            assert (got == lo).all()
        for s, t in enumerate(TRI):
            got = orc.quantize_batch(q, _book(K, True)[1][s].reshape(1, -1))
            assert np.isin(got, t).all()


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _run(ra, q, x, want, rows, dtypes, kernel="k_encode_mfma16"):
    import torch
    n = len(x)
    xd = torch.from_numpy(x).to("cuda:0")
    for dt in dtypes:
        fill = 255 if dt == torch.uint8 else -1
        out = torch.full((n + 64, M), fill, dtype=dt, device=xd.device)
        pq = ra.Pq(None, q)
        pq.quantize_batch_device(xd, out=out[:n])
        torch.cuda.synchronize()
        assert pq.last_encode_kernel().startswith(kernel), pq.last_encode_kernel()
        got = out.cpu().numpy()
        assert (got[n:] == fill).all(), "rows past n were written"
        codes = got[:n] if dt == torch.uint8 else got[:n].view(np.uint32)
        bad = np.argwhere(codes != want)
        assert bad.size == 0, (str(dt), len(bad), bad[:5].tolist(), codes[tuple(bad[0])], want[tuple(bad[0])],
                               int(np.isin(bad[:, 0], rows).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n", SMALL + [N64, N128])
def test_planted_pairs(ra, n, K):
    import torch
    _run(ra, *_case(K, False, n), dtypes=(torch.uint8,))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n", [4 * 128 + 109, N64, N128])
def test_duplicated_centroids(ra, n, K):
    import torch
    q, x, want, rows = _case(K, True, n)
    assert not np.isin(want, [hi for _, hi in DUPS]).any()
    assert np.isin(want[rows], [lo for lo, _ in DUPS]).any()
    _run(ra, q, x, want, rows, dtypes=(torch.uint8,))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n,special", [(N128, "overflow"), (N128, "counts"), (N64, "counts"), (4 * 128 + 109, "counts"),
                                       (N64, "exact"), (65, "exact")])
def test_lists_and_candidate_rows(ra, n, special, K):
    import torch
    _run(ra, *_case(K, False, n, special), dtypes=(torch.uint8,))


@pytest.mark.gpu
def test_u32_codes(ra):
    import torch
    _run(ra, *_case(256, True, N64), dtypes=(torch.int32,))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 4 * 128 + 109])
def test_codebook_below_the_screens_range(ra, n):
    # every norm of the codebook below kScreenMinCC: the screen does not apply and no row may be decided by it
    import torch
    s = np.float32(2.0 ** -54)
    q = _book(256, False)[0] * s
    assert max(float(orc.dot_unrolled(c, c)) for m in range(M) for c in q[m]) < 2.0 ** -100
    x = _base(256, False)[1][:n] * s
    x[n // 2] = _mid(_book(256, False)[0], 32, 33, 0) * s
    want = orc.quantize_batch(q, np.ascontiguousarray(x))
    _run(ra, q, np.ascontiguousarray(x), want, np.array([n // 2]), dtypes=(torch.uint8, torch.int32))
