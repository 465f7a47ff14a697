"""The screen's selection rule, as a numpy model on the host.

Per (lane, row block) a tile of k_encode_mfma16<8, 20, *> yields 64 screening values a[cb][v] (16 blocks of 4).  The
loop keeps, without a key on every value,

    block side    b[cb] = min_v a[cb][v] (raw), kb[cb] = (bits(b[cb]) & ~15) | cb, (mB, sB) = the two smallest kb
    column side   mv[v] = min_cb a[cb][v] (raw)
    end of tile   (mA, sA) = the two smallest mv, v* = the column of mA,
                  mk = (mB & ~63) | ((mB & 15) << 2) | v*,   sk = min(sA, sB)

and hands (mk, sk) to the merge in the place of the two smallest per-value keys (bits & ~63) | (4 cb + v).  What the
merge needs of them, and what is asserted here on random sets and on sets with planted ties and one-ulp neighbours:

  * sk is never above the second smallest value by more than the perturbation of a 4-bit key (15 ulp), and never below
    the smallest by more than that: every value but one is >= sk less that perturbation;
  * when the second smallest value is above the smallest by more than the perturbation of the keys, the index in mk is
    the position of the smallest value and mk is, bit for bit, its per-value key;
  * sk is within the two perturbations (63 + 15 ulp) of the second smallest per-value key.

The key mask and the screen's relative constant are read from the kernel header."""
import os
import re

import numpy as np
import pytest

HDR = os.path.join(os.path.dirname(__file__), "..", "reductive_amd", "csrc", "kernels_mfma16_screen.hip.h")
_SRC = open(HDR).read()
KEY_MASK = np.uint32(int(re.search(r"kKeyMask\s*=\s*(0x[0-9a-fA-F]+)u", _SRC).group(1), 16))
REL = float.fromhex(re.search(r"constexpr\s+float\s+kScreenRel\s*=\s*([-0-9a-fA-FxXpP.]+?)f?;", _SRC).group(1))
BLOCK_MASK = np.uint32(0xfffffff0)           # the rule's 4 index bits
KEY_ULPS, BLOCK_ULPS = 63, 15


def _bits(f):
    return np.ascontiguousarray(f, np.float32).view(np.uint32)


def _flt(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _two_smallest(k):
    """(smallest, second smallest) along the last axis, compared as floats, returned with their bits kept"""
    order = np.argsort(k, axis=-1, kind="stable")
    s = np.take_along_axis(k, order[..., :2], axis=-1)
    return s[..., 0], s[..., 1]


def _old_rule(a):
    n = a.shape[0]
    idx = np.arange(64, dtype=np.uint32)
    keys = _flt((_bits(a.reshape(n, 64)) & KEY_MASK) | idx)
    return _two_smallest(keys)


def _new_rule(a):
    b = a.min(axis=2)                                            # [n, 16]
    kb = _flt((_bits(b) & BLOCK_MASK) | np.arange(16, dtype=np.uint32))
    mB, sB = _two_smallest(kb)
    mv = a.min(axis=1)                                           # [n, 4]
    mA, sA = _two_smallest(mv)
    vs = np.where(mv[:, 1] == mA, 1, 0)
    vs = np.where(mv[:, 2] == mA, 2, vs)
    vs = np.where(mv[:, 3] == mA, 3, vs).astype(np.uint32)
    mb = _bits(mB)
    mk = _flt((mb & KEY_MASK) | ((mb & np.uint32(15)) << np.uint32(2)) | vs)
    sk = np.minimum(sA, sB)
    return mk, sk


def _check(a):
    a = np.ascontiguousarray(a, np.float32)
    n = a.shape[0]
    flat = a.reshape(n, 64)
    order = np.argsort(flat, axis=1, kind="stable")
    y1 = flat[np.arange(n), order[:, 0]].astype(np.float64)
    y2 = flat[np.arange(n), order[:, 1]].astype(np.float64)
    ulp1, ulp2 = np.spacing(np.abs(y1).astype(np.float32)).astype(np.float64), np.spacing(np.abs(y2).astype(np.float32)).astype(np.float64)
    mk, sk = _new_rule(a)
    mk_old, sk_old = _old_rule(a)
    sk64 = sk.astype(np.float64)
    over = (sk64 - y2) / ulp2
    assert (over <= BLOCK_ULPS).all(), float(over.max())
    assert (sk64 >= y1 - BLOCK_ULPS * ulp1).all()
    assert (np.abs(sk64 - sk_old.astype(np.float64)) <= (KEY_ULPS + BLOCK_ULPS) * ulp2).all()
    # a margin: more than the keys can move the two values towards each other
    margin = (y2 - y1) > 2 * (KEY_ULPS + 1) * np.maximum(ulp1, ulp2)
    want = (_bits(flat[np.arange(n), order[:, 0]]) & KEY_MASK) | order[:, 0].astype(np.uint32)
    assert (_bits(mk)[margin] == want[margin]).all()
    assert (_bits(mk)[margin] == _bits(mk_old)[margin]).all()
    return int(margin.sum()), n


def _plant(a, rng, kind, ulps):
    """the smallest value of every set twice: at a random position and at one chosen by `kind`, `ulps` steps apart"""
    n = a.shape[0]
    cb, v = rng.randint(0, 16, n), rng.randint(0, 4, n)
    if kind == "same_block":
        cb2, v2 = cb, (v + rng.randint(1, 4, n)) % 4
    elif kind == "same_column":
        cb2, v2 = (cb + rng.randint(1, 16, n)) % 16, v
    else:
        cb2, v2 = (cb + rng.randint(1, 16, n)) % 16, (v + rng.randint(1, 4, n)) % 4
    r = np.arange(n)
    low = a.reshape(n, 64).min(axis=1)
    low = low - np.abs(low) * np.float32(rng.choice([0.0, 1e-6, 0.5], n)).astype(np.float32)
    other = low.copy()
    for _ in range(ulps):
        other = np.nextafter(other, np.float32(np.inf)).astype(np.float32)
    swap = rng.randint(0, 2, n).astype(bool)
    a[r, cb, v] = np.where(swap, other, low)
    a[r, cb2, v2] = np.where(swap, low, other)
    return a


SCALES = [1.0, -1.0, 3.7e3, -2.0 ** 20, 2.0 ** 30, 2.0 ** -120, -2.0 ** -120, 2.0 ** -140, 65504.0 ** 2]


def _sets(rng, n, scale):
    a = rng.standard_normal((n, 16, 4)).astype(np.float32)
    if scale < 0:
        a = -np.abs(a)                                           # all negative
    elif scale in (2.0 ** 30, 65504.0 ** 2):
        a = np.abs(a) + np.float32(0.5)                          # all positive, beside the padding value
    return (a * np.float32(abs(scale))).astype(np.float32)


def test_key_perturbation_fits_the_screen_constant():
    # kScreenRel's share for two key perturbations is 2.0 * 2^-16 above the 132.6 * 2^-16 of the bound (header); a 6-bit
    # key moves a value by less than 2^-17 of it and a 4-bit key by less than 2^-19
    assert 2 * (KEY_ULPS + 1) * 2.0 ** -23 <= 2.0 * 2.0 ** -16 <= REL - 132.6 * 2.0 ** -16
    assert int(KEY_MASK) == 0xffffffc0 and (BLOCK_ULPS + 1) * 2.0 ** -23 <= 2.0 ** -19


@pytest.mark.parametrize("scale", SCALES)
def test_random_sets(scale):
    rng = np.random.RandomState(901)
    with_margin, n = _check(_sets(rng, 20000, scale))
    if abs(scale) > 2.0 ** -126:
        assert with_margin > n // 2                              # the margin case is the common one


@pytest.mark.parametrize("ulps", [0, 1, 2])
@pytest.mark.parametrize("kind", ["same_block", "same_column", "both"])
@pytest.mark.parametrize("scale", SCALES)
def test_planted_ties(scale, kind, ulps):
    rng = np.random.RandomState(902 + ulps)
    a = _plant(_sets(rng, 4000, scale), rng, kind, ulps)
    _check(a)


def test_ties_everywhere():
    # few distinct values: ties within blocks, within columns and across both at once; all equal; zeros of both signs
    rng = np.random.RandomState(903)
    a = rng.randint(-3, 4, (20000, 16, 4)).astype(np.float32)
    _check(a)
    _check(a * np.float32(2.0 ** -130))
    _check(np.full((4, 16, 4), 7.25, np.float32))
    z = np.zeros((64, 16, 4), np.float32)
    z[np.arange(64), np.arange(64) // 4, np.arange(64) % 4] = np.float32(-0.0)
    _check(z)
