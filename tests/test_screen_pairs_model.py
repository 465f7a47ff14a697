"""The few-candidate rows of the screen, as a numpy model on the host.

A row of k_encode_mfma16<8, 20, *> has 256 screening values, 64 per lane group g: a[g][cb][v], the value of centroid
16 cb + 4 g + v.  Round 9's rule hands the merge, per lane group, the smallest 6-bit key mk[g] and a lower bound sk[g] of
every other value.  With M = min mk, tau = M + thr and thr = kScreenRel (xx~ + max cc~) + kScreenAbs, the merge lists a
row for encode_rows_few when

    it is off the screen,  |M| > kScreenTiny,  every sk[g] > tau,  and  tau < -kScreenTiny or M > kScreenTiny,

and encode_rows_few takes as candidates the lane groups with mk[g] <= tau, centroid 16 (kb >> 2) + 4 g + (kb & 3) from
the key's low six bits kb.  One unit below is 2^-16 (xx~ + max cc~): kScreenRel is 144 units, of which 2.0 are for the
keys' perturbation.  Asserted on random sets and on sets with values planted at tau and at the edge of the needed set
(zero, one and two ulps to either side; in the smallest value's block, in its column, in another lane group), with
negative, positive and tiny values:

  * a listed row's decoded set holds every position whose value is <= the smallest + (thr - 2.02 units): the first
    minimum of the exact distance is among those (|A - s^2 (D - xx)| <= E_r, 2 E_r <= 132.6 units);
  * a lane group whose decoded index is not the position of its smallest value holds no needed position: a wrong index
    only ever adds a centroid;
  * no key taken as a candidate of a listed row is within kScreenTiny of zero.

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
KEY_MASK = np.uint32(int(re.search(r"kKeyMask\s*=\s*(0x[0-9a-fA-F]+)u", _SRC).group(1), 16))
BLOCK_MASK = np.uint32(0xfffffff0)
F32 = np.float32


def _bits(f):
    return np.ascontiguousarray(f, F32).view(np.uint32)


def _flt(u):
    return np.ascontiguousarray(u, np.uint32).view(F32)


def _two_smallest(k):
    order = np.argsort(k, axis=-1, kind="stable")
    s = np.take_along_axis(k, order[..., :2], axis=-1)
    return s[..., 0], s[..., 1]


def _lane_group(a):
    """round 9's (mk, sk) of one lane group: a is [n, 16, 4]"""
    b = a.min(axis=2)
    kb = _flt((_bits(b) & BLOCK_MASK) | np.arange(16, dtype=np.uint32))
    mB, sB = _two_smallest(kb)
    mv = a.min(axis=1)
    mA, sA = _two_smallest(mv)
    vs = np.where(mv[:, 1] == mA, 1, 0)
    vs = np.where(mv[:, 2] == mA, 2, vs)
    vs = np.where(mv[:, 3] == mA, 3, vs).astype(np.uint32)
    mb = _bits(mB)
    mk = _flt((mb & KEY_MASK) | ((mb & np.uint32(15)) << np.uint32(2)) | vs)
    return mk, np.minimum(sA, sB)


def _merge(a, X):
    """the merge of a row: a is [n, 4, 16, 4], X = xx~ + max cc~ per row.  Returns mq, tau, listed."""
    n = a.shape[0]
    mq, sq = np.empty((n, 4), F32), np.empty((n, 4), F32)
    for g in range(4):
        mq[:, g], sq[:, g] = _lane_group(a[:, g])
    lo01, hi01 = np.minimum(mq[:, 0], mq[:, 1]), np.maximum(mq[:, 0], mq[:, 1])
    lo23, hi23 = np.minimum(mq[:, 2], mq[:, 3]), np.maximum(mq[:, 2], mq[:, 3])
    Mk = np.minimum(lo01, lo23)
    S2 = sq.min(axis=1)
    S = np.minimum(np.minimum(np.maximum(lo01, lo23), np.minimum(hi01, hi23)), S2)
    thr = (F32(REL) * X.astype(F32) + F32(ABS)).astype(F32)
    tau = (Mk + thr).astype(F32)
    plain = np.abs(Mk) > F32(TINY)
    one = plain & (S > tau)
    listed = plain & ~one & (S2 > tau) & ((tau < -F32(TINY)) | (Mk > F32(TINY)))
    return mq, tau, thr, listed


def _decode(mq, tau):
    """per lane group: is it a candidate, and the position (cb, v) its key names"""
    kb = _bits(mq) & np.uint32(63)
    return mq <= tau[:, None], (kb >> np.uint32(2)).astype(np.int64), (kb & np.uint32(3)).astype(np.int64)


def _check(a, X):
    a = np.ascontiguousarray(a, F32)
    n = a.shape[0]
    mq, tau, thr, listed = _merge(a, X)
    cand, dcb, dv = _decode(mq, tau)
    flat = a.reshape(n, 4, 64).astype(np.float64)
    y1 = flat.min(axis=(1, 2))
    unit = 2.0 ** -16 * X.astype(np.float64)
    needed = flat <= (y1 + thr.astype(np.float64) - 2.02 * unit)[:, None, None]          # [n, 4, 64]
    decoded = np.zeros((n, 4, 64), bool)
    r = np.arange(n)
    for g in range(4):
        decoded[r, g, 4 * dcb[:, g] + dv[:, g]] = cand[:, g]
    missed = (needed & ~decoded).any(axis=(1, 2))
    assert not (missed & listed).any(), (int((missed & listed).sum()), np.flatnonzero(missed & listed)[:3])
    # a lane group whose decoded index is not where its smallest value is holds no needed position
    for g in range(4):
        low = flat[:, g].min(axis=1)
        wrong = cand[:, g] & (flat[r, g, 4 * dcb[:, g] + dv[:, g]] != low) & listed
        assert not (wrong & needed[:, g].any(axis=1)).any(), (g, int(wrong.sum()))
    tiny = (cand & (np.abs(mq) <= F32(TINY))).any(axis=1)
    assert not (tiny & listed).any()
    return int(listed.sum())


def _sets(rng, n, kind):
    """[n, 4, 16, 4] values of rows with X = xx~ + max cc~: |A| <= cc~ + 2 sqrt(cc~ xx~) <= 2 X"""
    X = (2.0 ** rng.uniform(12, 31, n)).astype(F32)
    a = (rng.uniform(-1.0, 1.0, (n, 4, 16, 4)) * 2.0 * X[:, None, None, None].astype(np.float64)).astype(F32)
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
    """a second value for every row: at tau ("tau") or at the edge of the needed set ("edge"), `ulps` steps off, in the
    smallest value's block, in its column in another block, or in another lane group"""
    n = a.shape[0]
    r = np.arange(n)
    flat = a.reshape(n, 256)
    p = flat.argmin(axis=1)
    g, cb, v = p // 64, (p % 64) // 4, p % 4
    if where == "same_block":
        g2, cb2, v2 = g, cb, (v + rng.randint(1, 4, n)) % 4
    elif where == "same_column":
        g2, cb2, v2 = g, (cb + rng.randint(1, 16, n)) % 16, v
    else:
        g2, cb2, v2 = (g + rng.randint(1, 4, n)) % 4, rng.randint(0, 16, n), rng.randint(0, 4, n)
    mq, tau, thr, _ = _merge(a, X)
    if value is not None:
        y = np.full(n, value, F32)
    elif level == "tau":
        y = tau
    else:
        y = (flat[r, p].astype(np.float64) + thr.astype(np.float64) - 2.02 * 2.0 ** -16 * X.astype(np.float64)).astype(F32)
    a[r, g2, cb2, v2] = _step(y, ulps)
    return a


KINDS = ["mixed", "negative", "positive", "around_zero"]


def test_constants():
    # 2.0 of kScreenRel's 144 units pay for two key perturbations of 2^-17 |A| <= 1 unit each; the bound takes 132.6
    assert REL == 144 * 2.0 ** -16 and 132.6 + 2 * 1.01 <= 144 and int(KEY_MASK) == 0xffffffc0
    assert ABS <= TINY == 2.0 ** -100


@pytest.mark.parametrize("kind", KINDS)
def test_random_sets(kind):
    rng = np.random.RandomState(1001)
    a, X = _sets(rng, 20000, kind)
    listed = _check(a, X)
    if kind != "around_zero":
        assert listed > 200                                       # the listed case occurs


@pytest.mark.parametrize("ulps", [-2, -1, 0, 1, 2])
@pytest.mark.parametrize("level", ["tau", "edge"])
@pytest.mark.parametrize("where", ["same_block", "same_column", "other_group"])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_near_ties(kind, where, level, ulps):
    rng = np.random.RandomState(1002 + ulps)
    a, X = _sets(rng, 3000, kind)
    a = _plant(a, X, rng, where, level, ulps)
    listed = _check(a, X)
    if where == "other_group" and kind in ("mixed", "negative"):
        assert listed > 1000                                      # two candidates in two lane groups: the listed case
    if where != "other_group" and level == "edge":
        assert listed == 0                                        # two candidates in one lane group: the other path


@pytest.mark.parametrize("value", [0.0, -0.0, 2.0 ** -120, -2.0 ** -120, 2.0 ** -140])
@pytest.mark.parametrize("where", ["same_block", "other_group"])
def test_tiny_values(where, value):
    # a tiny value inside [M, tau] is a candidate whose index bits cannot be trusted: such rows are never listed
    rng = np.random.RandomState(1003)
    a, X = _sets(rng, 3000, "around_zero")
    a = _plant(a, X, rng, where, None, 0, value=value)
    assert _check(a, X) == 0
    # and with the tiny value as the smallest of all (|M| tiny)
    a, X = _sets(rng, 3000, "positive")
    a = _plant(a, X, rng, where, None, 0, value=value)
    assert _check(a, X) == 0


def test_exact_ties_across_lane_groups():
    # the same smallest value in two, three and four lane groups: every one of them is decoded
    rng = np.random.RandomState(1004)
    a, X = _sets(rng, 4000, "negative")
    n = a.shape[0]
    r = np.arange(n)
    low = (a.reshape(n, -1).min(axis=1) * F32(1.5)).astype(F32)
    copies = 2 + r % 3
    for g in range(4):
        on = g < copies
        cb, v = rng.randint(0, 16, n), rng.randint(0, 4, n)
        a[r[on], g, cb[on], v[on]] = low[on]
    mq, tau, thr, listed = _merge(a, X)
    cand, _, _ = _decode(mq, tau)
    assert _check(a, X) > 3000
    assert (cand[listed].sum(axis=1) >= copies[listed]).all()
