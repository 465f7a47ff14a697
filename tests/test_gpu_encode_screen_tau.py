"""k_encode_mfma16<8, 20, *>: the screen's threshold from the codebook's measured rounding error (DESIGN.md §5, K1m16,
round 13).

k_build_screen_image writes two coefficients a, b per subquantizer behind max cc, and the loop accepts a row when
S > M + (a X + b); tests/test_screen_codebook_bound.py states how they are derived and that the screening value stays
within them.  Here, d = 300, M = 15, K = 256 and 225, codes bit for bit against the oracle:

    gap     rows on the line through two centroids one unit apart, the nearer one ahead by g 2^-16 (X + C) in the exact
            distance, g from a quarter of the new threshold to twice the round-7 one (144) and on either side of both;
            the pair in one lane half (centroid j is in lane half (j >> 2) & 1: the candidate path when not decided) and
            in opposite halves (the few-candidate list), either centroid the nearer one
    c2 c3   two candidates in one half, three over both halves (a centre 0.25 from each of its centroids)
    few     one candidate in each half
    dup     a row equal to a centroid that exists twice in one half: the tie goes to the lower index
    cen     a row equal to an ordinary centroid: decided by the screen

in batches of n = 1, 33, 128 + 109 and 4 * 128 + 109 rows (rows_per_item 32) and one of 104,960 + 109 (rows_per_item
128) that also holds waves of cen rows with exactly 0, 1, 16, 17 and 64 candidate-path rows and a NaN row and a row beyond
kScreenMaxXX between candidate rows; u8 and i32 codes, the output pre-filled and with 64 guard rows.  The CPU test emulates
the screen with each sub-codebook's own a and b: the smallest gaps are never decided, the largest always, and in between
the new threshold decides rows that the round-7 one does not.

Codebooks at the ends of the measure: coordinates exact in f16 (delta = 0, the smallest threshold) and coordinates half an
f16 ulp off everywhere (the round-7 threshold, the caps), each with near-ties; two handles with different coefficients
alternating on one context; and an OPQ training step from f16-exact centroids, whose encode screens with the header of
the moved ones."""
import numpy as np
import pytest

import synth
import test_gpu_encode_screen_cand as tc
import test_screen_codebook_bound as cbb
import test_screen_f16_bound as fb
from oracle import pq_oracle as orc

M, DSUB = 15, 20
SMALL = [1, 33, 128 + 109, 4 * 128 + 109]
N_BIG, RPI_BIG = 104_960 + 109, 128
SETS = {
    "c2": [16 * 1 + 0, 16 * 9 + 3],                       # lane half 0, twice
    "c3": [16 * 2 + 1, 16 * 5 + 4 + 3, 16 * 11 + 12 + 2],   # halves 0, 1, 1
    "few": [16 * 2 + 8, 16 * 6 + 4],                      # halves 0 and 1
}
DUP = (16 * 6 + 4 + 1, 16 * 10 + 12 + 2)                   # lane half 1, twice
GAP_PAIRS = [(16 * 3 + 2, 16 * 12 + 1), (16 * 4 + 3, 16 * 7 + 4 + 2)]   # one half; opposite halves
COUNTS = {"c2": [2, 0], "c3": [1, 2], "few": [1, 1], "dup": [0, 2]}     # values within the threshold per lane half
KINDS = ["c2", "c3", "few", "dup", "cen", "gap"]
CAND = ["c2", "c3", "dup"]
PLANTED = sorted(j for s in SETS.values() for j in s) + list(DUP) + [j for p in GAP_PAIRS for j in p]
OLD_UNITS = fb.REL * 2.0 ** 16


def _half(j):
    return (j >> 2) & 1


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


_shared = {}


def _book(K):
    """the random codebook with the planted sets; the sets' centres; per sub-codebook (a, b, C, max cc)"""
    if ("q", K) not in _shared:
        q = np.ascontiguousarray(synth.normalish(9401, (M, 256, DSUB))[:, :K]).copy()
        centres = synth.normalish(9402, (len(SETS), M, DSUB))
        for s, idx in enumerate(SETS.values()):
            for i, j in enumerate(idx):
                q[:, j] = centres[s]
                q[:, j, 3 * i + 1] += np.float32(0.25)
        q[:, DUP[1]] = q[:, DUP[0]]
        for i, (lo, hi) in enumerate(GAP_PAIRS):
            q[:, hi] = q[:, lo]
            q[:, hi, 5 + i] += np.float32(1.0)
        coef = []
        for m in range(M):
            a, b, _, C = cbb.coefficients(q[m])
            coef.append((a, b, C, float(orc.sqdist(q[m], np.zeros((1, DSUB), np.float32)).max())))
        _shared["q", K] = (q, centres, coef)
    return _shared["q", K]


def _gaps(a_units):
    """g, in units of 2^-16 (X + C): from far inside the new threshold to far outside the round-7 one"""
    return [0.25 * a_units, 0.9 * a_units, 1.1 * a_units, 0.5 * (a_units + OLD_UNITS), 0.9 * OLD_UNITS, 1.1 * OLD_UNITS,
            2.0 * OLD_UNITS]


def _gap_row(q, coef, m, p):
    """row p's sub-vector m on the line through a planted pair: the nearer centroid ahead by gap number p % 7"""
    lo, hi = GAP_PAIRS[(p // 7) % 2]
    near, far = (lo, hi) if (p // 14) % 2 == 0 else (hi, lo)
    a, _, _, maxcc = coef[m]
    g = _gaps(a * 2.0 ** 16)[p % 7]
    c1, c2 = q[m, near].astype(np.float64), q[m, far].astype(np.float64)
    d = c2 - c1                                                  # one unit long
    x = (c1 + c2) / 2
    for _ in range(3):                                           # the gap depends on ||x||^2: a fixed point
        G = g * 2.0 ** -16 * (float(x @ x) + maxcc)
        x = (c1 + c2) / 2 - G / (2 * float(d @ d)) * d          # D(far) - D(near) = G
    return x.astype(np.float32)


def _row(kind, p, K):
    q, centres, coef = _book(K)
    x = np.empty((M, DSUB), np.float32)
    for m in range(M):
        if kind in SETS:
            x[m] = centres[list(SETS).index(kind), m]
        elif kind == "dup":
            x[m] = q[m, DUP[0]]
        elif kind == "gap":
            x[m] = _gap_row(q, coef, m, p + m)
        else:
            j = (7 * p + 3 * m) % K
            while j in PLANTED:
                j = (j + 1) % K
            x[m] = q[m, j]
    return x.reshape(M * DSUB)


def _base(K):
    """the shared random rows and their reference codes, once per K"""
    if K not in _shared:
        if "x" not in _shared:
            _shared["x"] = synth.normalish(9403, (N_BIG, M * DSUB))
            _shared["x"].setflags(write=False)
        want = orc.quantize_batch(_book(K)[0], _shared["x"], n_threads=8)
        want.setflags(write=False)
        _shared[K] = want
    return _shared[K], _shared["x"]


WAVE_COUNTS = {100: 0, 101: 1, 102: 16, 103: 17, 104: 64}
WAVE_EXACT = 300


def _positions(n):
    """row -> kind"""
    rpi = _rows_per_item(n)
    pos = {}
    waves = -(-n // rpi)
    for w in sorted({0, waves // 2, waves - 1}):
        for o in range(min(rpi, 72)):                            # every kind at every position modulo 8, both trips
            p = w * rpi + o
            if p < n:
                pos[p] = KINDS[(o + o // 8 + w) % len(KINDS)]
    for p in range(max(n - 70, 0), n):                           # the ragged end, both tiles of its trip
        pos[p] = KINDS[(p + 2) % len(KINDS)]
    if n == N_BIG:
        for p in range(50 * rpi, 52 * rpi):                      # every gap, pair and order many times over
            pos[p] = "gap"
        for w, count in WAVE_COUNTS.items():                     # exactly count rows for the candidate path
            chosen = {(7 * i + 2) % rpi for i in range(count)}
            assert len(chosen) == count
            for o in range(rpi):
                pos[w * rpi + o] = CAND[(o + w) % len(CAND)] if o in chosen else "cen"
        for o in range(rpi):                                     # the exact path's rows between candidate rows
            pos[WAVE_EXACT * rpi + o] = ("c3" if o % 2 else "c2") if o % 16 < 3 else "cen"
        for o, kind in ((1, "nan"), (17, "big"), (65, "nan"), (81, "big")):
            pos[WAVE_EXACT * rpi + o] = kind
    return pos


_cases = {}


def _case(K, n):
    if (K, n) not in _cases:
        assert _rows_per_item(n) == (RPI_BIG if n == N_BIG else 32)
        want_base, x_base = _base(K)
        q = _book(K)[0]
        pos = _positions(n)
        rows = np.array(sorted(pos), np.int64)
        x, want = x_base[:n].copy(), want_base[:n].copy()
        for p in rows:
            kind = pos[p]
            if kind == "nan":
                x[p] = _row("cen", int(p), K)
                x[p, (p % M) * DSUB + p % DSUB] = np.float32(np.nan)
            elif kind == "big":
                x[p] = x_base[p] * np.float32(2.0 ** 14)         # beyond kScreenMaxXX after the scale
            else:
                x[p] = _row(kind, int(p), K)
        want[rows] = orc.quantize_batch(q, np.ascontiguousarray(x[rows]))
        _cases[K, n] = (q, x, want, rows)
    return _cases[K, n]


def test_sets_and_waves():
    assert [_rows_per_item(n) for n in SMALL] == [32] * len(SMALL) and _rows_per_item(N_BIG) == RPI_BIG
    assert len(set(PLANTED)) == len(PLANTED) and max(PLANTED) < 220
    for kind, idx in SETS.items():
        assert [sum(_half(j) == g for j in idx) for g in range(2)] == COUNTS[kind], kind
    assert (_half(DUP[0]), _half(DUP[1])) == (1, 1) and DUP[0] < DUP[1]
    assert [(_half(lo), _half(hi)) for lo, hi in GAP_PAIRS] == [(0, 0), (0, 1)]
    pos = _positions(N_BIG)
    for w, count in WAVE_COUNTS.items():
        assert sum(pos[w * RPI_BIG + o] in CAND for o in range(RPI_BIG)) == count


def _emulated(qm, xm, a, b):
    """per row: the screen's smallest value, the second smallest, the threshold a X + b and the round-7 one"""
    A, old = tc._screen(qm, xm)
    zero = np.zeros((1, DSUB), np.float32)
    s, s2 = fb._scale(float(orc.sqdist(qm, zero).max()))
    X = float(s2) * orc.sqdist(xm, zero)[:, 0].astype(np.float64)
    two = np.sort(A, axis=1)[:, :2]
    return two[:, 0], two[:, 1], a * X + b, old


@pytest.mark.parametrize("K", [256, 225])
def test_planted_rows_are_what_they_claim(K):
    q, _, coef = _book(K)
    kinds = KINDS[:5]
    xr = np.stack([_row(kind, 5 + i, K) for i, kind in enumerate(kinds)])
    gaps = np.stack([_row("gap", p, K) for p in range(28 * 4)])
    want, want_gap = orc.quantize_batch(q, xr), orc.quantize_batch(q, gaps)
    half = (np.arange(K) >> 2) & 1
    new_only = 0
    for m in range(M):
        a, b, _, _ = coef[m]
        assert cbb.RELX < a < fb.REL                             # a measured threshold, below the round-7 one
        A, _ = tc._screen(q[m], np.ascontiguousarray(xr.reshape(-1, M, DSUB)[:, m]))
        _, _, thr, _ = _emulated(q[m], np.ascontiguousarray(xr.reshape(-1, M, DSUB)[:, m]), a, b)
        for f in (0.5, 2.0):
            within = A <= (A.min(axis=1) + f * thr)[:, None]
            got = np.stack([within[:, half == g].sum(axis=1) for g in range(2)], axis=1)
            for r, kind in enumerate(kinds):
                if kind == "cen":
                    assert got[r].sum() == 1, (kind, m, f, got[r].tolist())
                else:
                    assert got[r].tolist() == COUNTS[kind], (kind, m, f, got[r].tolist())
        assert int(want[3, m]) == DUP[0]
        for r, kind in enumerate(kinds[:3]):
            assert int(want[r, m]) in SETS[kind], (kind, m, int(want[r, m]))
        # the gap rows: row p's sub-vector m is gap number (p + m) % 7
        gm = np.ascontiguousarray(gaps.reshape(-1, M, DSUB)[:, m])
        lo, second, thr, old = _emulated(q[m], gm, a, b)
        which = (np.arange(len(gm)) + m) % 7
        decided, decided_old = second - lo > thr, second - lo > old
        assert not decided[which == 0].any() and decided[which == 6].all() and decided_old[which == 6].all()
        assert not (decided_old & ~decided).any()                # the new threshold is never the looser one
        new_only += int((decided & ~decided_old).sum())
        pairs = [set(pr) for pr in GAP_PAIRS]
        assert all({int(np.argsort(D)[0]), int(np.argsort(D)[1])} in pairs for D in orc.sqdist(gm, q[m]))
        assert all(int(c) in GAP_PAIRS[0] + GAP_PAIRS[1] for c in want_gap[:, m])
    assert new_only >= 4 * M, new_only                           # rows between the two thresholds


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _run(ra, pq, xd, want, rows=()):
    import torch
    n = xd.shape[0]
    for dt in (torch.uint8, torch.int32):
        fill = 255 if dt == torch.uint8 else -1
        out = torch.full((n + 64, M), fill, dtype=dt, device=xd.device)
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
@pytest.mark.parametrize("n", SMALL + [N_BIG])
def test_gaps_and_candidate_rows(ra, n, K):
    import torch
    q, x, want, rows = _case(K, n)
    _run(ra, ra.Pq(None, q), torch.from_numpy(x).to("cuda:0"), want, rows)


# ---- codebooks at the two ends of the measured error
N_EXT = 4 * 128 + 109


def _extreme(kind, K):
    """an f16-exact codebook or one half an f16 ulp off everywhere, rows with near-ties, the reference codes"""
    if ("e", kind, K) not in _shared:
        rng = np.random.RandomState(9501 + K)
        if kind == "exact":
            q = rng.uniform(-2.0, 2.0, (M, K, DSUB)).astype(np.float16).astype(np.float32)
        else:
            q = (np.float32(1.0 + 2.0 ** -11) * rng.choice([-1, 1], (M, K, DSUB))).astype(np.float32)
        x = synth.normalish(9502, (N_EXT, M * DSUB)).reshape(N_EXT, M, DSUB).copy()
        for r in range(0, N_EXT, 2):                             # every other row: between two centroids, g units ahead
            for m in range(M):
                i, j = rng.choice(K, 2, replace=False)
                c1, c2 = q[m, i].astype(np.float64), q[m, j].astype(np.float64)
                d = c2 - c1
                if not d.any():
                    continue
                mid = (c1 + c2) / 2
                g = [20.0, 70.0, 90.0, 130.0, 160.0][(r // 2) % 5]
                G = g * 2.0 ** -16 * (float(mid @ mid) + float(c1 @ c1))
                x[r, m] = (mid - G / (2 * float(d @ d)) * d).astype(np.float32)
        x = np.ascontiguousarray(x.reshape(N_EXT, M * DSUB))
        _shared["e", kind, K] = (np.ascontiguousarray(q), x, orc.quantize_batch(np.ascontiguousarray(q), x, n_threads=8))
    return _shared["e", kind, K]


def test_extreme_codebooks_on_the_host():
    for K in (256, 225):
        a, b, delta, C = cbb.coefficients(_extreme("exact", K)[0][0])
        assert delta == 0.0 and a == cbb.RELX
        a, b, delta, C = cbb.coefficients(_extreme("half-ulp", K)[0][0])
        assert a == fb.REL and delta > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("kind", ["exact", "half-ulp"])
def test_extreme_codebooks(ra, kind, K):
    import torch
    q, x, want = _extreme(kind, K)
    _run(ra, ra.Pq(None, q), torch.from_numpy(x).to("cuda:0"), want)


@pytest.mark.gpu
def test_two_handles_with_different_coefficients_alternate(ra):
    import torch
    qa, xa, wa = _extreme("exact", 256)
    qb, xb, wb = _extreme("half-ulp", 256)
    qc, xc, wc, _ = _case(256, SMALL[-1])
    hs = [(ra.Pq(None, q), torch.from_numpy(x).to("cuda:0"), w) for q, x, w in ((qa, xa, wa), (qb, xb, wb), (qc, xc, wc))]
    for i in (0, 1, 2, 1, 0, 0, 2):
        _run(ra, *hs[i])
    for pq, _, _ in hs:
        pq.close()


@pytest.mark.gpu
def test_training_step_from_f16_exact_centroids(ra):
    """the OPQ training step moves centroids that were exact in f16 (the smallest threshold) to ones that are not: the
    encode that follows must screen with the moved centroids' image and coefficients"""
    import torch
    n, Mt = 20_000, 3
    x = synth.normalish(9601, (n, Mt * DSUB))
    q0 = np.ascontiguousarray(x[:256].reshape(256, Mt, DSUB).transpose(1, 0, 2)).astype(np.float16).astype(np.float32)
    P = synth.orthonormal(9602, Mt * DSUB)
    want_q, want_cross = orc.opq_train_step(q0, P, x, n_threads=8)
    assert cbb.coefficients(q0[0])[2] == 0.0 and cbb.coefficients(want_q[0])[2] > 0.0
    ra.launch_log(reset=True)
    q, cross = ra.opq_train_step(q0, P, torch.from_numpy(x).to("cuda:0"))
    log = ra.launch_log(reset=True)
    assert "k_encode_mfma16" in log and log.count("k_build_screen_image") == 1, log
    assert q.tobytes() == want_q.tobytes(), "centroids differ from the oracle"
    assert cross.tobytes() == want_cross.tobytes(), "cross product differs from the oracle"
