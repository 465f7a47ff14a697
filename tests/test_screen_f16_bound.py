"""The f16 screen's error bound, checked on the host.

The screening value of k_encode_mfma16<8, 20, *> is emulated the way the kernel builds it: one power-of-two scale s per
subquantizer from max cc, A operand RNE_f16(-2 s c) and the hi / lo f16 split of s^2 cc, B operand RNE_f16(s x) with the
[1 1] tail, and the 22 products summed.  For every (row, centroid) pair |A - s^2 (D - xx)| must stay within
E = kScreenRel / 2 * (s^2 xx + s^2 max cc) + kScreenAbs / 2, D and xx the CANON-F32 values of the oracle, the constants
read from the kernel header.  f16 operands in the subnormal range are checked both kept and flushed to zero, and the
sum both exactly and as a float32 chain with truncating adds."""
import os
import re

import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

HDR = os.path.join(os.path.dirname(__file__), "..", "reductive_amd", "csrc", "kernels_mfma16_screen.hip.h")
DSUB = 20


def _const(name):
    src = open(HDR).read()
    mt = re.search(r"constexpr\s+(float|int)\s+%s\s*=\s*([-0-9a-fA-FxXpP.]+)f?;" % name, src)
    assert mt, name
    v = mt.group(2)
    if mt.group(1) == "float" and v[-1] in "fF" and "p" in v.lower():
        v = v[:-1]                                               # the literal's suffix, not a hex digit
    return int(v) if mt.group(1) == "int" else float.fromhex(v) if "x" in v.lower() else float(v)


REL, ABS = _const("kScreenRel"), _const("kScreenAbs")
SCALE_LO, MAX_XX, MIN_CC = _const("kScreenScaleLo"), _const("kScreenMaxXX"), _const("kScreenMinCC")
F16_MIN_NORMAL = 2.0 ** -14


def _scale(maxcc):
    e_cc = int(np.frexp(np.float32(maxcc))[1]) - 1           # floor(log2 maxcc), as the exponent bits give it
    e = (SCALE_LO + 1 - e_cc) >> 1
    return np.float32(2.0 ** e), np.float32(2.0 ** (2 * e))


def _f16(v, flush):
    h = np.asarray(v, np.float32).astype(np.float16).astype(np.float64)
    if flush:
        h = np.where(np.abs(h) < F16_MIN_NORMAL, 0.0, h)
    return h


def _sum_rtz_f32(terms):
    """Sequential float32 sum whose every add truncates (one order of the many the matrix core may take)."""
    acc = np.zeros(terms.shape[:-1], np.float64)
    for k in range(terms.shape[-1]):
        s = acc + terms[..., k]                                  # exact enough in f64 for 22 f32-sized terms
        r = s.astype(np.float32).astype(np.float64)
        over = np.abs(r) > np.abs(s)
        r = np.where(over, np.nextafter(r.astype(np.float32), np.float32(0)).astype(np.float64), r)
        acc = r
    return acc


@np.errstate(all="ignore")
def _check(q, x):
    q = np.ascontiguousarray(q, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    cc = orc.sqdist(q, np.zeros((1, DSUB), np.float32))[:, 0]   # rule-1 norms, as the codebook handle holds them
    xx = orc.sqdist(x, np.zeros((1, DSUB), np.float32))[:, 0]
    D = orc.sqdist(x, q).astype(np.float64)
    maxcc = float(cc.max())
    assert MIN_CC <= maxcc < 2.0 ** 100
    s, s2 = _scale(maxcc)
    C = float(s2) * maxcc
    assert 2.0 ** SCALE_LO <= C < 2.0 ** (SCALE_LO + 2)
    X = float(s2) * xx.astype(np.float64)
    keep = X < MAX_XX                                            # the others take the exact path
    assert keep.any()
    cct = (s2 * cc).astype(np.float32)
    hi = cct.astype(np.float16).astype(np.float32)
    lo = (cct - hi).astype(np.float32)
    want = float(s2) * (D - xx.astype(np.float64)[:, None])
    E = REL / 2 * (X + C) + ABS / 2
    worst = 0.0
    for flush in (False, True):
        a = _f16((np.float32(-2) * s) * q, flush)                # [K, 20]
        b = _f16(s * x, flush)                                   # [n, 20]
        tail = _f16(hi, flush) + _f16(lo, flush)
        prods = b[:, None, :] * a[None, :, :]                    # exact: 11 x 11 significand bits
        terms = np.concatenate([prods, np.broadcast_to(_f16(hi, flush)[None, :, None], prods.shape[:2] + (1,)),
                                np.broadcast_to(_f16(lo, flush)[None, :, None], prods.shape[:2] + (1,))], axis=2)
        for A in (prods.sum(axis=2) + tail[None, :], _sum_rtz_f32(terms)):
            err = np.abs(A - want)[keep]
            ratio = err / E[keep][:, None]
            worst = max(worst, float(ratio.max()))
            assert (err <= E[keep][:, None]).all(), (flush, float(ratio.max()))
    return worst


def test_normal_rows_bench_codebook():
    q = synth.normalish(43, (1, 256, DSUB))[0]
    x = synth.normalish(44, (2000, DSUB))
    assert _check(q, x) < 0.75


def test_rows_on_and_opposite_centroids():
    q = synth.normalish(45, (256, DSUB))
    x = np.concatenate([q, -q, q * np.float32(0.5), q[::-1] + q]).astype(np.float32)
    _check(q, x)


def test_rounding_errors_aligned():
    # every component half an f16 ulp (less a little) off a representable value, with signs that make the errors of
    # x and c add up in the product: the worst case of the operand term
    rng = np.random.RandomState(46)
    base = rng.uniform(1.0, 2.0, (256, DSUB)).astype(np.float16).astype(np.float32)
    ulp = np.float32(2.0 ** -10)
    q = (base + ulp * np.float32(0.499)) * rng.choice([-1, 1], (256, DSUB)).astype(np.float32)
    xb = rng.uniform(1.0, 2.0, (512, DSUB)).astype(np.float16).astype(np.float32)
    x = (xb + ulp * np.float32(0.499)) * np.sign(q[rng.randint(0, 256, 512)])
    x = np.concatenate([x, q, -q]).astype(np.float32)
    _check(q, x)


@pytest.mark.parametrize("scale", [2.0 ** -48, 1e-12, 1e-3, 1.0, 37.0, 1e6, 2.0 ** 40])
def test_extreme_ranges(scale):
    sc = np.float32(scale)
    q = synth.normalish(47, (256, DSUB)) * sc
    x = synth.normalish(48, (600, DSUB)) * sc
    x[:100] *= np.float32(1e-4)                                 # components in and below f16's subnormal range
    x[100:200, ::2] = np.float32(0)
    x[200:300] *= np.float32(2.0 ** 9)                          # scaled norms beside the f16 range limit
    q[:32, 1:] *= np.float32(1e-6)                               # centroids with one big and 19 tiny components
    q[32:40] = np.float32(0)
    _check(q.astype(np.float32), x.astype(np.float32))


def test_spread_centroid_norms():
    rng = np.random.RandomState(49)
    q = synth.normalish(50, (256, DSUB)) * (np.float32(10.0) ** rng.uniform(-3, 3, (256, 1))).astype(np.float32)
    x = synth.normalish(51, (800, DSUB)) * (np.float32(10.0) ** rng.uniform(-3, 3, (800, 1))).astype(np.float32)
    _check(q.astype(np.float32), x.astype(np.float32))
