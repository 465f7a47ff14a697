"""k_encode_mfma16<8, 20, *>: the rows with several candidates in one lane, resolved by encode_rows_cand_f16 sixteen at a
time in two passes of the f16 screen and a walk that evaluates two candidates per trip.

Centroid j sits in lane group (j >> 2) & 3, and one lane holds a row's 64 values of its lane group.  A row with two or more
values within the threshold in one lane cannot go to the few-candidate list and takes this path.  Planted, in a codebook
built as in test_gpu_encode_screen_pairs.py (a set's centroids are one centre moved by 0.25 along different axes, so a row
at the centre is equally far from all of them):

    c2 c3 c5 c6   2, 3, 5 and 6 candidates in ONE lane (lane group 2): the odd counts leave the walk's second slot empty on
                  the last trip
    c1+2, c3+1    a lane with a single candidate beside a lane with two or three
    dup           a row equal to a centroid that exists twice in one lane group: the exact tie goes to the lower index
    pad           centroids 220 .. 223 (one lane, lane group 3) and 224: with K = 225 the rest of 224's block and every later
                  block is padding
    cen           a row equal to an ordinary centroid: one candidate, decided by the screen; the filler of the batch waves

Counts are mixed over the sixteen rows of a batch, the kinds stand at every row-block edge of both tiles of a trip in the
first, a middle and the last whole wave and over the ragged end, and three waves hold exactly 1, 16 and 17 such rows among
cen rows (one batch with a single row, one full batch, one full batch and a second with a single row).

A second codebook has coordinates that are multiples of 1/4, exact in f16 at the screen's scale: a row x = c / 2 makes the
screening value of c exactly zero, as small as that of the all-zero centroid 2 (a tie at zero, below the threshold that keeps
a key's index bits out of the subnormal range), and an all-zero row does the same with centroid 2 alone.

The CPU test emulates the screen in numpy (as test_screen_f16_bound.py does) and counts the values within the threshold per
lane group, at half and at twice the threshold's margin, so that the rows are what they claim on any summation order; the
oracle's code must be among the planted centroids.  n = 20,000 gives rows_per_item 32, n = 204,813 gives 64 and a ragged
end; u8 and i32 codes; codes bit for bit against the oracle."""
import numpy as np
import pytest

import synth
import test_screen_f16_bound as fb
from oracle import pq_oracle as orc

M, DSUB = 3, 20
SIZES = [(20_000, 32), (204_813, 64)]
N_MAX = 204_813
BLOCK_EDGES = [0, 15, 16, 31, 32, 47, 48, 63]


def _j(cb, g, v):
    return 16 * cb + 4 * g + v


SETS = {
    "c2": [_j(1, 2, 0), _j(9, 2, 3)],
    "c3": [_j(0, 2, 1), _j(0, 2, 2), _j(12, 2, 0)],
    "c5": [_j(2, 2, 0), _j(2, 2, 3), _j(5, 2, 1), _j(8, 2, 2), _j(11, 2, 0)],
    "c6": [_j(3, 2, 0), _j(3, 2, 1), _j(3, 2, 2), _j(3, 2, 3), _j(7, 2, 2), _j(13, 2, 1)],
    "c1+2": [_j(4, 0, 1), _j(6, 1, 0), _j(10, 1, 3)],
    "c3+1": [_j(1, 3, 0), _j(4, 3, 3), _j(9, 3, 2), _j(12, 1, 1)],
    "pad": [220, 221, 222, 223, 224],
}
DUP = (_j(6, 2, 1), _j(10, 2, 2))
# values within the threshold per lane group
COUNTS = {"c2": [0, 0, 2, 0], "c3": [0, 0, 3, 0], "c5": [0, 0, 5, 0], "c6": [0, 0, 6, 0], "c1+2": [1, 2, 0, 0],
          "c3+1": [0, 1, 0, 3], "pad": [1, 0, 0, 4], "dup": [0, 0, 2, 0], "cen": None}
CAND_KINDS = ["c2", "c3", "c5", "c6", "c1+2", "c3+1", "pad", "dup"]
PLANTED = sorted(j for s in SETS.values() for j in s) + list(DUP)


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


_shared = {}


def _book(K):
    """the random codebook with the planted sets, and the sets' centres, once per K"""
    if ("q", K) not in _shared:
        q = np.ascontiguousarray(synth.normalish(9201, (M, 256, DSUB))[:, :K]).copy()
        centres = synth.normalish(9202, (len(SETS), M, DSUB))
        for s, idx in enumerate(SETS.values()):
            for i, j in enumerate(idx):
                q[:, j] = centres[s]
                q[:, j, 3 * i + 1] += np.float32(0.25)
        q[:, DUP[1]] = q[:, DUP[0]]
        _shared["q", K] = (q, centres)
    return _shared["q", K]


def _row(kind, p, q, centres):
    """planted row number p of a kind: the row and, per sub-vector, the centroids it may be given to"""
    K = q.shape[1]
    x = np.empty((M, DSUB), np.float32)
    allowed = []
    for m in range(M):
        if kind in SETS:
            x[m], al = centres[list(SETS).index(kind), m], set(SETS[kind])
        elif kind == "dup":
            x[m], al = q[m, DUP[0]], {DUP[0]}
        else:
            j = (7 * p + 3 * m) % K
            while j in PLANTED:
                j = (j + 1) % K
            x[m], al = q[m, j], {j}
        allowed.append(al)
    return x.reshape(M * DSUB), allowed


def _positions(n, rpi):
    """row -> kind"""
    waves = n // rpi
    pos = {}
    offs = [o for o in BLOCK_EDGES if o < rpi]
    for w in (0, waves // 2 + 3, waves - 1):
        for i, o in enumerate(offs):
            for k in range(len(CAND_KINDS)):                   # every kind at every edge, over 8 neighbouring waves
                pos[((w + k) % waves) * rpi + o] = CAND_KINDS[(i + k) % len(CAND_KINDS)]
    for p in range(n - 70, n):                                 # the ragged end
        pos[p] = CAND_KINDS[p % len(CAND_KINDS)]
    # three waves of cen rows with exactly 1, 16 and 17 rows for this path, the counts mixed over a batch
    for w, count in ((100, 1), (101, 16), (102, 17)):
        for o in range(rpi):
            pos[w * rpi + o] = "cen"
        for i in range(count):
            pos[w * rpi + (5 * i + 2) % rpi] = CAND_KINDS[(3 * i + w) % len(CAND_KINDS)]
    return pos


_cases = {}


def _planted(K, n, rpi):
    key = (K, n)
    if key not in _cases:
        q, centres = _book(K)
        pos = _positions(n, rpi)
        rows = np.array(sorted(pos), np.int64)
        kinds = [pos[p] for p in rows]
        built = [_row(k, int(p), q, centres) for k, p in zip(kinds, rows)]
        xr = np.stack([b[0] for b in built])
        _cases[key] = (rows, kinds, xr, orc.quantize_batch(q, np.ascontiguousarray(xr)), [b[1] for b in built])
    return _cases[key]


def _base(K):
    if K not in _shared:
        if "x" not in _shared:
            _shared["x"] = synth.normalish(9203, (N_MAX, M * DSUB))
            _shared["x"].setflags(write=False)
        _shared[K] = orc.quantize_batch(_book(K)[0], _shared["x"], n_threads=8)
    return _shared[K], _shared["x"]


def _case(K, n, rpi):
    rows, _, xr, wr, _ = _planted(K, n, rpi)
    want_base, x_base = _base(K)
    x, want = x_base[:n].copy(), want_base[:n].copy()
    x[rows], want[rows] = xr, wr
    return _book(K)[0], x, want, rows


@np.errstate(all="ignore")
def _screen(qm, xm):
    """the screen's values of rows xm against the sub-codebook qm, exact sums of the f16 operands' products: the values,
    and per row the threshold's margin"""
    zero = np.zeros((1, DSUB), np.float32)
    cc, xx = orc.sqdist(qm, zero)[:, 0], orc.sqdist(xm, zero)[:, 0]
    s, s2 = fb._scale(float(cc.max()))
    cct = (s2 * cc).astype(np.float32)
    hi = cct.astype(np.float16).astype(np.float32)
    lo = (cct - hi).astype(np.float32)
    a = fb._f16((np.float32(-2) * s) * qm, False)
    b = fb._f16(s * xm, False)
    A = b @ a.T + (fb._f16(hi, False) + fb._f16(lo, False))[None, :]
    margin = fb.REL * (float(s2) * xx.astype(np.float64) + float(s2) * float(cc.max())) + fb.ABS
    return A, margin


def _counts(A, margin, f):
    """values within min + f * margin per lane group, [rows, 4]"""
    within = A <= (A.min(axis=1) + f * margin)[:, None]
    g = (np.arange(A.shape[1]) >> 2) & 3
    return np.stack([within[:, g == k].sum(axis=1) for k in range(4)], axis=1)


def test_sets_and_sizes():
    for n, rpi in SIZES:
        assert _rows_per_item(n) == rpi
    assert N_MAX % 64 != 0 and len(set(PLANTED)) == len(PLANTED) and max(PLANTED) == 224
    for kind, idx in SETS.items():
        assert [sum(((j >> 2) & 3) == g for j in idx) for g in range(4)] == COUNTS[kind], kind
    assert ((DUP[0] >> 2) & 3, (DUP[1] >> 2) & 3) == (2, 2) and DUP[0] < DUP[1]
    for n, rpi in SIZES:                                       # the batch waves: 1, 16 and 17 rows for this path
        pos = _positions(n, rpi)
        assert [sum(pos[w * rpi + o] != "cen" for o in range(rpi)) for w in (100, 101, 102)] == [1, 16, 17]


@pytest.mark.parametrize("K", [256, 225])
def test_planted_rows_are_what_they_claim(K):
    q, _ = _book(K)
    rows, kinds, xr, want, allowed = _planted(K, *SIZES[0])
    assert set(kinds) == set(COUNTS)
    for m in range(M):
        A, margin = _screen(q[m], np.ascontiguousarray(xr.reshape(-1, M, DSUB)[:, m]))
        lo, hi = _counts(A, margin, 0.5), _counts(A, margin, 2.0)
        assert (lo == hi).all(), "a value near the threshold"
        for r, kind in enumerate(kinds):
            expect = COUNTS[kind]
            if expect is None:                                 # cen: a single value within the threshold
                assert lo[r].sum() == 1, (int(rows[r]), m, lo[r].tolist())
            else:
                assert lo[r].tolist() == expect, (int(rows[r]), kind, m, lo[r].tolist())
            assert int(want[r, m]) in allowed[r][m], (int(rows[r]), kind, m, int(want[r, m]))


# ---- smallest screening value exactly zero
ZERO_J = 2


def _zero_book(K):
    """coordinates k / 4, |k| <= 8, centroid 2 all zero; the centroids c whose half c / 2 the oracle gives to c or to 2"""
    if ("z", K) not in _shared:
        h = synth.uniform01(9301, (M, 256, DSUB))[:, :K]
        q = np.ascontiguousarray((np.floor(h * 17) - 8) * np.float32(0.25)).astype(np.float32)
        q[:, ZERO_J] = 0
        a = np.array([j for j in range(K) if j != ZERO_J])
        halves = np.ascontiguousarray((q[:, a] * np.float32(0.5)).transpose(1, 0, 2).reshape(len(a), M * DSUB))
        got = orc.quantize_batch(q, halves)
        good = a[((got == a[:, None]) | (got == ZERO_J)).all(axis=1)]
        _shared["z", K] = (q, good)
    return _shared["z", K]


def _zero_case(K, n):
    if ("zc", K) not in _shared:
        q, good = _zero_book(K)
        x = (np.floor(synth.uniform01(9302, (n, M * DSUB)) * 17) - 8).astype(np.float32) * np.float32(0.25)
        rows = sorted({w * 32 + o for w in (0, 311, n // 32 - 1) for o in BLOCK_EDGES[:4]} | set(range(n - 40, n)))
        for i, p in enumerate(rows):
            if i % 3 == 2:
                x[p] = 0                                        # the all-zero row
            else:
                j = good[(5 * i) % len(good)]
                x[p] = (q[:, j] * np.float32(0.5)).reshape(M * DSUB)
        _shared["zc", K] = (q, x, orc.quantize_batch(q, x, n_threads=8), np.array(rows))
    return _shared["zc", K]


@pytest.mark.parametrize("K", [256, 225])
def test_zero_rows_are_what_they_claim(K):
    q, good = _zero_book(K)
    assert len(good) >= 8, len(good)
    _, x, want, rows = _zero_case(K, SIZES[0][0])
    for m in range(M):
        A, margin = _screen(q[m], np.ascontiguousarray(x[rows].reshape(-1, M, DSUB)[:, m]))
        assert (A.min(axis=1) == 0.0).all() and (A[:, ZERO_J] == 0.0).all()      # exact: every operand is exact in f16
        assert (margin > 0).all()


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _encode_and_check(ra, q, x, want, rows):
    import torch
    n = x.shape[0]
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


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("n,rpi", SIZES)
def test_many_candidates_in_one_lane(ra, n, rpi, K):
    _encode_and_check(ra, *_case(K, n, rpi))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
def test_smallest_value_exactly_zero(ra, K):
    _encode_and_check(ra, *_zero_case(K, SIZES[0][0]))
