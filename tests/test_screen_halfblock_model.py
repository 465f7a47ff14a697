"""The half-block / column rule of the screen on v_mfma_f32_32x32x16_f16, as a numpy
model on the host.

A row of k_encode_mfma16<8, 20, *> has 256 screening values, 128 per lane half h: a[h][j][c], half-block j = 0..15
(registers 0..7 and 8..15 of block j >> 1), column c = 0..7; the value of centroid 16 j + 8 (c >> 2) + 4 h + (c & 3).
Per half the loop keeps

    block side    kb[j] = (bits(min_c a[j][c]) & ~15) | j,  (mB, sB) = the two smallest kb
    column side   kv[c] = (bits(min_j a[j][c]) & ~7) | c,   (mA, sA) = the two smallest kv
    mk = (mB & ~127) | ((mB & 15) << 3) | (mA & 7),         sk = min(sA, sB)

and the merge of the two halves takes M = min(m0, m1), S = min(max(m0, m1), s0, s1), tau = M + thr with
thr = kScreenRel (xx~ + max cc~) + kScreenAbs.  A row is decided when |M| > kScreenTiny and S > tau, its centroid decoded
from M's low seven bits and the half that holds M; it is listed for encode_rows_few when it is not decided, |M| >
kScreenTiny, both sk > tau, and tau < -kScreenTiny or M > kScreenTiny, with the halves whose mk <= tau as candidates.

One unit below is 2^-16 (xx~ + max cc~).  A 7-bit key moves a value by less than 2^-16 |A| <= 2.02 units (|A| <= 2.02
(xx~ + max cc~)); kScreenRel is 144 units, of which 132.6 are the bound's 2 E_r and 4.04 two key perturbations.
Asserted on random sets and on sets with a second value planted 0, 1 and 2 ulps to either side of the smallest value, of
tau and of the edge of the needed set, in the smallest value's half-block, in its column in another half-block, and in
the other half of the row, with negative, positive and tiny values:

  * sk never exceeds the second smallest value of its half by more than a key's perturbation (and never the smallest
    of the other values by more than that);
  * when S > tau the decoded centroid is the position of the row's first minimum;
  * a listed row's two keys name every position whose value is within thr - 4.04 units of the smallest value;
  * no candidate of a listed row is within kScreenTiny of zero.

The constants are read from the kernel header."""
import os
import re

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(__file__), "..", "reductive_amd", "csrc", "kernels_mfma16_screen.hip.h")
_SRC = open(HDR).read()


def _const(name):
    return float.fromhex(re.search(r"constexpr\s+float\s+%s\s*=\s*([-0-9a-fA-FxXpP.]+?)f?;" % name, _SRC).group(1))


REL, ABS, TINY = _const("kScreenRel"), _const("kScreenAbs"), _const("kScreenTiny")
KEY7_MASK = np.uint32(int(re.search(r"kKey7Mask\s*=\s*(0x[0-9a-fA-F]+)u", _SRC).group(1), 16))
HALF_MASK, COL_MASK = np.uint32(0xfffffff0), np.uint32(0xfffffff8)
F32 = np.float32
PERTURB = 2.02                                       # units: one 7-bit key on |A| <= 2.02 (xx~ + max cc~)


def _bits(f):
    return np.ascontiguousarray(f, F32).view(np.uint32)


def _flt(u):
    return np.ascontiguousarray(u, np.uint32).view(F32)


def _two_smallest(k):
    order = np.argsort(k, axis=-1, kind="stable")
    s = np.take_along_axis(k, order[..., :2], axis=-1)
    return s[..., 0], s[..., 1]


def _half(a):
    """(mk, sk) of one lane half: a is [n, 16, 8]"""
    kb = _flt((_bits(a.min(axis=2)) & HALF_MASK) | np.arange(16, dtype=np.uint32))
    mB, sB = _two_smallest(kb)
    kv = _flt((_bits(a.min(axis=1)) & COL_MASK) | np.arange(8, dtype=np.uint32))
    mA, sA = _two_smallest(kv)
    mb = _bits(mB)
    mk = _flt((mb & KEY7_MASK) | ((mb & np.uint32(15)) << np.uint32(3)) | (_bits(mA) & np.uint32(7)))
    return mk, np.minimum(sA, sB)


def _merge(a, X):
    """the merge of a row: a is [n, 2, 16, 8], X = xx~ + max cc~ per row"""
    n = a.shape[0]
    mq, sq = np.empty((n, 2), F32), np.empty((n, 2), F32)
    for h in range(2):
        mq[:, h], sq[:, h] = _half(a[:, h])
    Mk = mq.min(axis=1)
    S2 = sq.min(axis=1)
    S = np.minimum(mq.max(axis=1), S2)
    thr = (F32(REL) * X.astype(F32) + F32(ABS)).astype(F32)
    tau = (Mk + thr).astype(F32)
    plain = np.abs(Mk) > F32(TINY)
    one = plain & (S > tau)
    listed = plain & ~one & (S2 > tau) & ((tau < -F32(TINY)) | (Mk > F32(TINY)))
    return mq, sq, tau, thr, one, listed


def _position(key):
    """(half-block, column) named by a key's low seven bits"""
    kb = _bits(key) & np.uint32(127)
    return (kb >> np.uint32(3)).astype(np.int64), (kb & np.uint32(7)).astype(np.int64)


def _centroid(j, c, h):
    return 16 * j + 8 * (c >> 2) + 4 * h + (c & 3)


def _check(a, X):
    a = np.ascontiguousarray(a, F32)
    n = a.shape[0]
    r = np.arange(n)
    mq, sq, tau, thr, one, listed = _merge(a, X)
    flat = a.reshape(n, 2, 128).astype(np.float64)
    unit = 2.0 ** -16 * X.astype(np.float64)
    # sk is a lower bound of every value of its half but the smallest, up to a key's perturbation
    for h in range(2):
        second = np.sort(flat[:, h], axis=1)[:, 1]
        assert (sq[:, h].astype(np.float64) <= second + PERTURB * unit).all(), h
    S = np.minimum(mq.max(axis=1), sq.min(axis=1)).astype(np.float64)
    assert (S <= np.sort(flat.reshape(n, 256), axis=1)[:, 1] + PERTURB * unit).all()
    # a decided row: the decoded centroid is the first minimum
    y1 = flat.min(axis=(1, 2))
    hw = np.where(mq[:, 0] <= mq[:, 1], 0, 1)
    j, c = _position(mq[r, hw])
    by_centroid = np.empty((n, 256), np.float64)
    for h in range(2):
        for jj in range(16):
            for cc in range(8):
                by_centroid[:, _centroid(jj, cc, h)] = flat[:, h, 8 * jj + cc]
    first = by_centroid.argmin(axis=1)
    got = _centroid(j, c, hw)
    assert (got[one] == first[one]).all(), (int((got[one] != first[one]).sum()), np.flatnonzero(one & (got != first))[:3])
    # a listed row: the two keys name every needed position
    cand = mq <= tau[:, None]
    needed = flat <= (y1 + thr.astype(np.float64) - 2 * PERTURB * unit)[:, None, None]          # [n, 2, 128]
    decoded = np.zeros((n, 2, 128), bool)
    for h in range(2):
        jh, ch = _position(mq[:, h])
        decoded[r, h, 8 * jh + ch] = cand[:, h]
    missed = (needed & ~decoded).any(axis=(1, 2))
    assert not (missed & listed).any(), (int((missed & listed).sum()), np.flatnonzero(missed & listed)[:3])
    tiny = (cand & (np.abs(mq) <= F32(TINY))).any(axis=1)
    assert not (tiny & listed).any()
    return int(one.sum()), int(listed.sum())


def _sets(rng, n, kind):
    """[n, 2, 16, 8] values of rows with X = xx~ + max cc~: |A| <= cc~ + 2 sqrt(cc~ xx~) <= 2 X"""
    X = (2.0 ** rng.uniform(12, 31, n)).astype(F32)
    a = (rng.uniform(-1.0, 1.0, (n, 2, 16, 8)) * 2.0 * X[:, None, None, None].astype(np.float64)).astype(F32)
    if kind == "negative":
        a = -np.abs(a)
    elif kind == "positive":
        a = np.abs(a) + F32(1.0)
    elif kind == "around_zero":                  # the smallest a little below zero, so that tau is above it
        low = a.reshape(n, -1).min(axis=1)
        a = (a - (low + F32(0.25 * REL) * X)[:, None, None, None]).astype(F32)
    return a, X


def _step(x, ulps):
    x = np.ascontiguousarray(x, F32).copy()
    for _ in range(abs(ulps)):
        x = np.nextafter(x, F32(np.inf if ulps > 0 else -np.inf)).astype(F32)
    return x


def _plant(a, X, rng, where, level, ulps, value=None):
    """a second value for every row: at the smallest value ("tie"), at tau ("tau") or at the edge of the needed set
    ("edge"), `ulps` steps off, in the smallest value's half-block, in its column in another half-block, or in the
    other half of the row"""
    n = a.shape[0]
    r = np.arange(n)
    flat = a.reshape(n, 256)
    p = flat.argmin(axis=1)
    h, j, c = p // 128, (p % 128) // 8, p % 8
    if where == "same_halfblock":
        h2, j2, c2 = h, j, (c + rng.randint(1, 8, n)) % 8
    elif where == "same_column":
        h2, j2, c2 = h, (j + rng.randint(1, 16, n)) % 16, c
    else:
        h2, j2, c2 = 1 - h, rng.randint(0, 16, n), rng.randint(0, 8, n)
    _, _, tau, thr, _, _ = _merge(a, X)
    if value is not None:
        y = np.full(n, value, F32)
    elif level == "tie":
        y = flat[r, p]
    elif level == "tau":
        y = tau
    else:
        y = (flat[r, p].astype(np.float64) + thr.astype(np.float64) - 2 * PERTURB * 2.0 ** -16 * X.astype(np.float64)).astype(F32)
    a[r, h2, j2, c2] = _step(y, ulps)
    return a


KINDS = ["mixed", "negative", "positive", "around_zero"]
WHERE = ["same_halfblock", "same_column", "other_half"]


def test_constants():
    # 4.04 of kScreenRel's 144 units pay for two key perturbations of 2^-16 |A| <= 2.02 units each; the bound takes 132.6
    assert REL == 144 * 2.0 ** -16 and 132.6 + 2 * PERTURB <= 144 and int(KEY7_MASK) == 0xffffff80
    assert ABS <= TINY == 2.0 ** -100
    # the decoding covers every centroid once
    assert sorted(_centroid(j, c, h) for h in range(2) for j in range(16) for c in range(8)) == list(range(256))


@pytest.mark.parametrize("kind", KINDS)
def test_random_sets(kind):
    rng = np.random.RandomState(1201)
    a, X = _sets(rng, 20000, kind)
    one, listed = _check(a, X)
    if kind != "around_zero":
        assert one > 1000 and listed > 200                        # both cases occur


@pytest.mark.parametrize("ulps", [-2, -1, 0, 1, 2])
@pytest.mark.parametrize("level", ["tie", "tau", "edge"])
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("kind", KINDS)
def test_planted_near_ties(kind, where, level, ulps):
    rng = np.random.RandomState(1202 + ulps)
    a, X = _sets(rng, 3000, kind)
    a = _plant(a, X, rng, where, level, ulps)
    one, listed = _check(a, X)
    if level == "tie":
        assert one == 0                                           # a value this near the smallest is never screened out
    if where == "other_half" and level == "edge" and kind in ("mixed", "negative"):
        assert listed > 1000                                      # one candidate per half: the listed case
    if where != "other_half" and level == "edge":
        assert listed == 0                                        # two candidates in one half: the other path


@pytest.mark.parametrize("value", [0.0, -0.0, 2.0 ** -120, -2.0 ** -120, 2.0 ** -140])
@pytest.mark.parametrize("where", ["same_halfblock", "other_half"])
def test_tiny_values(where, value):
    # a tiny value inside [M, tau] is a candidate whose index bits cannot be trusted: such rows are never listed
    rng = np.random.RandomState(1203)
    a, X = _sets(rng, 3000, "around_zero")
    a = _plant(a, X, rng, where, None, 0, value=value)
    assert _check(a, X)[1] == 0
    # and with the tiny value as the smallest of all (|M| tiny): neither decided nor listed
    a, X = _sets(rng, 3000, "positive")
    a = _plant(a, X, rng, where, None, 0, value=value)
    assert _check(a, X) == (0, 0)


def test_exact_ties_across_the_halves():
    # the same smallest value in both halves: both are decoded, and the row is never decided by the screen
    rng = np.random.RandomState(1204)
    a, X = _sets(rng, 4000, "negative")
    n = a.shape[0]
    r = np.arange(n)
    low = (F32(-2.01) * X).astype(F32)                            # below every other value, |A| <= 2.02 X
    for h in range(2):
        a[r, h, rng.randint(0, 16, n), rng.randint(0, 8, n)] = low
    mq, _, tau, _, one, listed = _merge(a, X)
    assert _check(a, X)[1] > 3000 and not one.any()
    assert ((mq <= tau[:, None]).sum(axis=1)[listed] == 2).all()
