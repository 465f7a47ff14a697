"""CPU tests of the u8 table screen's model (tests/adc_screen_ref.py): the proof by enumeration over every
code combination of two tiny quantizers against adversarial tables, thresholds and scales; the stated tightness; and the
composition of Pq.adc_search_batch_device against the exhaustive reference, bit for bit."""
import itertools

import numpy as np
import pytest

import adc_screen_ref as asr

F = np.float32
UP = lambda v: np.nextafter(F(v), F(np.inf))      # noqa: E731
DOWN = lambda v: np.nextafter(F(v), F(-np.inf))   # noqa: E731


def _tables(M, K, seed):
    """adversarial [M, K] tables by name"""
    rng = np.random.default_rng(seed)
    base = (rng.random((M, K)) * 2 - 1).astype(F)
    out = {"random": base, "constant": np.full((M, K), F(0.37)), "zero": np.zeros((M, K), F)}
    for name, (at, v) in {"huge": ((0, 1), 3e37), "inf": ((1, 2), np.inf), "-inf": ((0, 0), -np.inf), "nan": ((1, 0), np.nan),
                          "subnormal": ((0, 2), 1e-42)}.items():
        out[name] = base.copy()
        out[name][at] = v
    out["subnormals"] = (base * F(1e-40)).astype(F)
    out["cancel"] = np.where(np.arange(K)[None, :] % 2 == 0, F(1e7), F(-1e7)) + base      # sums that cancel
    out["ulp"] = np.full((M, K), F(1.0))
    out["ulp"][:, 1] = UP(1.0)
    out["ulp"][:, 2] = DOWN(1.0)
    return out


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,K", [(3, 5), (2, 16)])
def test_no_admitted_row_is_excluded_and_every_excluded_row_misses(M, K, ip, scaled):
    codes = np.array(list(itertools.product(range(K), repeat=M)), np.int64)
    n = codes.shape[0]
    scale_sets = [None]
    if scaled:
        rng = np.random.default_rng(5)
        mixed = (rng.random(n) * 2).astype(F)
        mixed[::7] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38, -0.0], F), len(mixed[::7]))
        scale_sets = [mixed, np.ones(n, F), np.zeros(n, F)]
    for name, t in _tables(M, K, 100 * M + K).items():
        for sc in scale_sets:
            v = asr.values(t, codes, ip, sc)
            exact = t.astype(np.float64)[np.arange(M)[None, :], codes].sum(1) * (1.0 if sc is None else sc.astype(np.float64))
            fin = np.sort(v[np.isfinite(v)])
            picks = [fin[0], fin[fin.size // 2], fin[-1]] if fin.size else []
            thrs = [x for p in picks for x in (p, UP(p), DOWN(p))] + [F(0), F(np.inf), F(-np.inf), F(np.nan), F(-3e38), F(3e38)]
            for thr in thrs:
                keep, p = asr.screen(t, codes, thr, ip, sc)
                with np.errstate(invalid="ignore"):
                    admitted = (v >= thr) if ip else (v <= thr)
                    misses = (exact < float(thr)) if ip else (exact > float(thr))
                assert not (admitted & ~keep).any(), (name, float(thr))
                assert misses[~keep].all(), (name, float(thr))            # a NaN exact value is never excluded
                if sc is None and p["ulim"] not in (asr.KEEP_ALL, -1) and name not in ("inf", "-inf", "nan"):
                    over = (float(thr) - v.astype(np.float64)) if ip else (v.astype(np.float64) - float(thr))
                    assert (over[keep] <= asr.slack(p, M)).all(), (name, float(thr))   # the stated tightness
                    assert p["ulim"] <= 254 and p["step"] > 0
                elif sc is not None and p["ulim"] == asr.PER_ROW:
                    reg = keep & np.isfinite(sc) & (sc >= 0)
                    ch, c64 = asr.chain(t, codes).astype(np.float64)[reg], sc.astype(np.float64)[reg]
                    assert (float(thr) - ch * c64 <= asr.slack(p, M, ch, c64)).all(), (name, float(thr))


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_composition_equals_the_exhaustive_reference(ip, scaled):
    from reductive_amd import pq
    rng = np.random.default_rng(31)
    M, K, n, nq = 4, 16, 3000, 5
    tables = ((rng.random((nq, M, K)) * 2).astype(F) + (0 if ip else 1)) * F(-1 if ip else 1)
    tables[:, :, :3] *= F(0.05)
    codes = np.where(rng.random((n, M)) < 0.3, rng.integers(0, 3, (n, M)), rng.integers(0, K, (n, M))).astype(np.int64)
    sc = (rng.random(n) + 0.5).astype(F) if scaled else None
    for allow, k in ((None, 3), (rng.random(n) < 0.5, 3), (np.arange(n) % 397 == 1, 5)):     # the last one: a thin sample
        val, idx, plain, want = asr.ref_adc_search_batch(tables, codes, k, pq.flat_batch_sample, pq.flat_batch_falls_back, ip, sc, allow)
        assert val.tobytes() == want[0].tobytes() and np.array_equal(idx, want[1])
        assert plain.all() == (allow is not None and allow.sum() < 20)
