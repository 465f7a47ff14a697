"""CPU tests of the 16-bit table screen (pqhip_adc_screen16_f32_dev): the name is registered everywhere, bad
arguments are refused before the library, and the model of tests/adc_screen16_ref.py is sound and as tight as stated on
every code combination of two tiny quantizers against the adversarial tables of test_adc_screen.py."""
import itertools
import os

import numpy as np
import pytest

import adc_screen16_ref as a16
from test_adc_screen import DOWN, UP, F, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_name_is_registered_everywhere():
    import inspect
    from reductive_amd import _lib, pq
    header = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    assert "int32_t %s(" % a16.NAME in header and "%s and %s" % ("pqhip_adc_screen_f32_dev", a16.NAME) in header   # the option list
    assert a16.NAME in _lib.EXPORTS and _lib.SIGNATURES[a16.NAME] == _lib.SIGNATURES["pqhip_adc_screen_f32_dev"]
    assert callable(getattr(_lib.lib(), a16.NAME))
    assert "pub fn %s(" % a16.NAME in open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    for fn in (pq.Pq.adc_screen_device, pq.Pq.adc_search_batch_device):
        assert inspect.signature(fn).parameters["image_bits"].default == 8


@pytest.mark.parametrize("what", [4, 32, "16", None, "codes", "tables", "scales", "capacity", "k"])
def test_bad_arguments_are_refused_before_the_library(what, monkeypatch):
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    a = dict(codes=torch.zeros((8, 3), dtype=torch.uint8), tables=torch.zeros((2, 3, 16)))
    bad = dict(codes=a["codes"].to(torch.int32), tables=a["tables"][:, :, :8])
    bad_bits = what in (4, 32, "16", None)
    if not bad_bits and what in bad:
        a[what] = bad[what]
    bits = what if bad_bits else 16
    calls = [lambda: pq.adc_screen_device(a["codes"], a["tables"], 0.5, capacity=-1 if what == "capacity" else None,
                                          scales=torch.ones(8) if what == "scales" else None, image_bits=bits),
             lambda: pq.adc_search_batch_device(a["codes"], a["tables"], 0 if what == "k" else 1, image_bits=bits)]
    for call in calls[1:] if what == "k" else calls[:1] if what in ("capacity", "scales") else calls:
        # whatever passes the shape checks is refused as a host tensor, still before the library
        with pytest.raises(ra.PanicError, match="image_bits" if bad_bits else None):
            call()


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,K", [(3, 5), (2, 16)])
def test_the_model_is_sound_and_tight_on_every_code_combination(M, K, ip, scaled):
    codes = np.array(list(itertools.product(range(K), repeat=M)), np.int64)
    n, L = codes.shape[0], a16.levels(M)
    scale_sets = [None]
    if scaled:
        mixed = (np.random.default_rng(5).random(n) * 2).astype(F)
        mixed[::7] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38, -0.0], F), len(mixed[::7]))
        scale_sets = [mixed, np.ones(n, F)]
    for name, t in _tables(M, K, 100 * M + K).items():
        for sc in scale_sets:
            v = a16.values(t, codes, ip, sc)
            exact = t.astype(np.float64)[np.arange(M)[None, :], codes].sum(1) * (1.0 if sc is None else sc.astype(np.float64))
            fin = np.sort(v[np.isfinite(v)])
            picks = [fin[0], fin[fin.size // 2], fin[-1]] if fin.size else []
            thrs = [x for p in picks for x in (p, UP(p), DOWN(p))] + [F(0), F(np.inf), F(-np.inf), F(np.nan), F(-3e38), F(3e38)]
            for thr in thrs:
                keep, p, U = a16.screen16(t, codes, thr, ip, sc)
                with np.errstate(invalid="ignore"):
                    admitted = (v >= thr) if ip else (v <= thr)
                    misses = (exact < float(thr)) if ip else (exact > float(thr))
                assert not (admitted & ~keep).any(), (name, float(thr))   # no row whose f32 chain meets the threshold is excluded
                assert misses[~keep].all(), (name, float(thr))            # a NaN exact value is never excluded
                assert p["img"].max() <= L and U.max() <= M * L <= 65535
                if sc is None and p["ulim"] not in (a16.KEEP_ALL, -1) and name not in ("inf", "-inf", "nan"):
                    over = (float(thr) - v.astype(np.float64)) if ip else (v.astype(np.float64) - float(thr))
                    assert (over[keep] <= a16.slack16(p, M)).all(), (name, float(thr))   # the stated tightness
                    assert p["ulim"] <= L - 1 and p["step"] > 0
                elif sc is not None and p["ulim"] == a16.PER_ROW:
                    reg = keep & np.isfinite(sc) & (sc >= 0)
                    ch, c64 = a16.chain(t, codes).astype(np.float64)[reg], sc.astype(np.float64)[reg]
                    assert (float(thr) - ch * c64 <= a16.slack16(p, M, ch, c64)).all(), (name, float(thr))


@pytest.mark.parametrize("M,K", [(3, 5), (2, 16), (100, 16), (48, 256), (1, 256)])
def test_saturated_entries_sum_to_M_L_within_16_bits(M, K):
    t = np.full((M, K), F(1e6))
    t[:, 0] = F(0.25)                                   # every other entry saturates at any threshold near the minimum row
    codes = np.stack([np.zeros(M, np.int64), np.full(M, K - 1, np.int64), np.arange(M) % K])
    keep, p, U = a16.screen16(t, codes, F(0.25 * M + 1.0))
    L = a16.levels(M)
    assert p["img"].max() == L and U[1] == M * L <= 65535 and M * (L + 1) > 65535
    assert keep.tolist() == [True, False, M == 1]       # row 2 has one minimal entry (and only that one at M = 1)
