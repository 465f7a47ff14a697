"""The f16 screen's threshold with the centroids' rounding error measured per codebook,
checked on the host.

k_build_screen_image measures, per subquantizer, delta >= max over the centroids of || fl16(-2 s c) - (-2 s c) ||_2 and
derives the row threshold's coefficients from it,

    a = kScreenRelX + (1 + 2^-11) (1 + 2^-20) delta / sqrt(C),   b = a C + kScreenAbs,   C = s^2 max cc,

each rounded up to float32, and both replaced by the round-7 values kScreenRel and kScreenRel C + kScreenAbs when either
reaches its own; the screen accepts a row when S > M + (a X + b), X = s^2 xx.  This test computes a and b the same way and
emulates the screening value as test_screen_f16_bound.py does; for every (row, centroid) pair |A - s^2 (D - xx)| must stay
within (a X + b) / 2 less the allowance of one key's perturbation, kScreenKeyUnits 2^-16 (X + C).  Five input sets, each
with f16 subnormals kept and flushed, and the sum both exact and as a float32 chain with truncating adds."""
import numpy as np
import pytest

import synth
import test_screen_f16_bound as fb
from oracle import pq_oracle as orc

DSUB = fb.DSUB
RELX, KEY_UNITS = fb._const("kScreenRelX"), fb._const("kScreenKeyUnits")
U = 2.0 ** -11


def _up32(v):
    """the smallest float32 >= v (v > 0)"""
    f = np.float32(v)
    return f if float(f) >= v else np.nextafter(f, np.float32(np.inf))


def coefficients(q):
    """(a, b, delta, C) of a sub-codebook, as k_build_screen_image computes them"""
    q = np.ascontiguousarray(q, np.float32)
    cc = orc.sqdist(q, np.zeros((1, DSUB), np.float32))[:, 0]
    maxcc = float(cc.max())
    s, s2 = fb._scale(maxcc)
    C = float(np.float32(s2 * np.float32(maxcc)))
    v = (np.float32(-2) * s) * q                                 # exact: a power of two
    e = v.astype(np.float16).astype(np.float64) - v.astype(np.float64)
    delta = float(np.sqrt((e * e).sum(axis=1).max()))
    a = _up32(RELX + ((1.0 + U) * (1.0 + 2.0 ** -20)) * delta / np.sqrt(C))
    b = _up32(float(a) * C + fb.ABS)
    cap_a = np.float32(fb.REL)
    cap_b = np.float32(np.float32(cap_a * np.float32(C)) + np.float32(fb.ABS))
    if not (a < cap_a and b < cap_b):
        a, b = cap_a, cap_b
    return float(a), float(b), delta, C


@np.errstate(all="ignore")
def _check(q, x):
    """the largest error seen, as a fraction of the allowance"""
    q = np.ascontiguousarray(q, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    a_thr, b_thr, _, C = coefficients(q)
    assert a_thr <= fb.REL and b_thr <= float(np.float32(fb.REL) * np.float32(C)) + fb.ABS
    cc = orc.sqdist(q, np.zeros((1, DSUB), np.float32))[:, 0]
    xx = orc.sqdist(x, np.zeros((1, DSUB), np.float32))[:, 0]
    D = orc.sqdist(x, q).astype(np.float64)
    s, s2 = fb._scale(float(cc.max()))
    X = float(s2) * xx.astype(np.float64)
    keep = X < fb.MAX_XX
    assert keep.any()
    cct = (s2 * cc).astype(np.float32)
    hi = cct.astype(np.float16).astype(np.float32)
    lo = (cct - hi).astype(np.float32)
    want = float(s2) * (D - xx.astype(np.float64)[:, None])
    E = (a_thr * X + b_thr) / 2 - KEY_UNITS * 2.0 ** -16 * (X + C)
    worst = 0.0
    for flush in (False, True):
        a = fb._f16((np.float32(-2) * s) * q, flush)
        b = fb._f16(s * x, flush)
        prods = b[:, None, :] * a[None, :, :]
        terms = np.concatenate([prods, np.broadcast_to(fb._f16(hi, flush)[None, :, None], prods.shape[:2] + (1,)),
                                np.broadcast_to(fb._f16(lo, flush)[None, :, None], prods.shape[:2] + (1,))], axis=2)
        for A in (terms.sum(axis=2), fb._sum_rtz_f32(terms)):
            err = np.abs(A - want)[keep]
            ratio = err / E[keep][:, None]
            worst = max(worst, float(ratio.max()))
            assert (err <= E[keep][:, None]).all(), (flush, float(ratio.max()))
    return worst


def test_bench_like_data():
    q = synth.normalish(43, (1, 256, DSUB))[0]
    x = synth.normalish(44, (2000, DSUB))
    a, b, delta, C = coefficients(q)
    # random mantissas: the largest centroid error is well under the worst case 2 u sqrt(C), and so is the threshold
    assert 0 < delta < 0.7 * 2 * U * np.sqrt(C) and RELX < a < 0.85 * fb.REL
    assert _check(q, x) < 0.75


def test_rows_on_and_opposite_centroids():
    q = synth.normalish(45, (256, DSUB))
    x = np.concatenate([q, -q, q * np.float32(0.5), q[::-1] + q]).astype(np.float32)
    _check(q, x)


def _aligned(rng, n, frac):
    base = rng.uniform(1.0, 2.0, (n, DSUB)).astype(np.float16).astype(np.float32)
    return base + np.float32(2.0 ** -10) * np.float32(frac)


def test_rounding_errors_aligned():
    # every component of x and of c half an f16 ulp (less a little) off a representable value, with signs that make the
    # errors add up in the product
    rng = np.random.RandomState(46)
    q = _aligned(rng, 256, 0.499) * rng.choice([-1, 1], (256, DSUB)).astype(np.float32)
    x = _aligned(rng, 512, 0.499) * np.sign(q[rng.randint(0, 256, 512)])
    x = np.concatenate([x, q, -q]).astype(np.float32)
    _check(q, x)


def test_codebook_exact_in_f16():
    # delta = 0: a and b fall to the rows' half and the floor terms, not to zero
    rng = np.random.RandomState(52)
    q = (rng.uniform(-2.0, 2.0, (256, DSUB)).astype(np.float16).astype(np.float32))
    a, b, delta, C = coefficients(q)
    assert delta == 0.0 and a == RELX and b == float(_up32(RELX * C + fb.ABS))
    x = np.concatenate([_aligned(rng, 512, 0.499) * np.sign(q[rng.randint(0, 256, 512)]), q, -q,
                        synth.normalish(53, (500, DSUB))]).astype(np.float32)
    _check(q, x)


def test_codebook_half_an_ulp_off_everywhere():
    # every coordinate +-(1 + 2^-11) 2^e: half an f16 ulp off at the largest relative error, delta at its maximum
    # 2 u sqrt(C) / (1 + u): a and b equal the caps, the round-7 threshold
    rng = np.random.RandomState(54)
    q = (np.float32(1.0 + 2.0 ** -11) * rng.choice([-1, 1], (256, DSUB))).astype(np.float32)
    a, b, delta, C = coefficients(q)
    assert a == fb.REL and b == float(np.float32(np.float32(fb.REL) * np.float32(C)) + np.float32(fb.ABS))
    assert delta == pytest.approx(2 * U * np.sqrt(C) / (1 + U), rel=1e-6)
    x = np.concatenate([(np.float32(1.0 + 2.0 ** -11) * rng.choice([-1, 1], (512, DSUB))).astype(np.float32), q, -q,
                        _aligned(rng, 256, 0.499) * np.sign(q)]).astype(np.float32)
    _check(q, x)
