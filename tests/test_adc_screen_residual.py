"""CPU tests of the u8 table screen over residual codes in probed lists (pqhip_adc_screen_lists_residual_f32_dev): the
symbol is registered everywhere, bad arguments are refused before the library is reached, and the model of
tests/adc_screen_residual_ref.py is sound and as tight as the header states, by enumeration."""
import itertools
import os
import re

import numpy as np
import pytest

import adc_screen_ref as asr
import adc_screen_residual_ref as rr
from adc_residual_ref import residual_values
from test_adc_screen import DOWN, UP, F, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_registered_in_the_header_the_wrapper_and_the_rust_file():
    from reductive_amd import _lib
    lists, res = _lib.SIGNATURES["pqhip_adc_screen_lists_f32_dev"][1], _lib.SIGNATURES[rr.NAME][1]
    assert rr.NAME in _lib.EXPORTS and res == lists[:14] + [lists[0], lists[3], lists[0]] + lists[14:]   # bias, stride, terms before ip
    header = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    assert re.search(r"int32_t %s\(.*?d_probe_bias, int64_t bias_row_stride,\s+const float \*d_row_terms[^,]*,\s+int32_t ip" % rr.NAME, header, re.S)
    assert "pub fn %s(" % rr.NAME in open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()


@pytest.mark.parametrize("what,message", [("codes", "codes must be a uint8"), ("tables", "lookup tables must be"), ("row_terms with ip", "row terms belong"),
                                          ("row_terms", "needs the row terms"), ("probe_bias", "needs a probe bias"),
                                          ("capacity", "capacity must not be negative"), ("k", "k must be between")])
def test_bad_arguments_are_refused_before_the_library(what, message, monkeypatch):
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    a = dict(codes=torch.zeros((8, 3), dtype=torch.uint8), tables=torch.zeros((2, 3, 16)), list_off=torch.tensor([0, 4, 8]),
             probes=torch.zeros((2, 1), dtype=torch.int64), probe_bias=torch.zeros((2, 1)), row_terms=torch.zeros(8), threshold=0.5)
    a.update({"codes": dict(codes=a["codes"].to(torch.int32)), "tables": dict(tables=a["tables"][:, :, :8]), "row_terms": dict(row_terms=None),
              "probe_bias": dict(probe_bias=None)}.get(what, {}))
    with pytest.raises(ra.PanicError, match=message):
        if what == "k":
            pq.adc_search_lists_residual_batch_device(*list(a.values())[:6], torch.zeros(8, dtype=torch.int64), 0)
        else:
            pq.adc_screen_lists_residual_device(*a.values(), ip=what == "row_terms with ip", capacity=-1 if what == "capacity" else None)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,K", [(2, 4), (3, 3)])
def test_no_row_is_left_out_unless_its_exact_value_misses_and_returned_rows_lie_within_the_slack(M, K, ip, scaled):
    codes, n, rng = np.array(list(itertools.product(range(K), repeat=M)), np.int64), K ** M, np.random.default_rng(17 * M + K)
    if ip:                                                                 # x: the scales, or ones
        mixed = (rng.random(n) * 2).astype(F)
        mixed[::5] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38, -0.0], F), len(mixed[::5]))
        xs = [mixed, np.zeros(n, F), np.full(n, F(0.5))] if scaled else [np.ones(n, F)]
    else:                                                                  # x: the row terms, both signs, far below and above the tables
        xs = [((rng.random(n) * 2 - 1) * mag).astype(F) for mag in (1e-6, 1.0, 1e6)]
        xs[1][::6] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0], F), len(xs[1][::6]))
    bias_pairs = [(0.0, 0.25), (-0.5, 3.0), (1e6, -1e6), (1e-6, -1e-6), (3e5, 3e5 + 1), (np.nan, 1.0), (-np.inf, 0.0)]
    one_list = (np.array([0, n]), np.zeros((1, 1), np.int64))
    for name, t in _tables(M, K, 100 * M + K).items():
        s = asr.chain(t, codes)
        for x, pair in itertools.product(xs, bias_pairs):
            tmin, cmax = rr.call_wide(None if ip else x, x if scaled else None)
            kw = dict(scales=x if scaled else None, ip=True) if ip else dict(terms=x)
            for b in pair:
                v = residual_values(s[None], *one_list, np.array([[b]], F), **kw)[0]
                fin = np.sort(v[np.isfinite(v)])
                picks = [fin[0], fin[fin.size // 2], fin[-1]] if fin.size else []
                for thr in [y for p in picks for y in (p, UP(p), DOWN(p))] + [F(0), F(np.inf), F(-np.inf), F(np.nan), F(3e38)]:
                    p = rr.prep(t, rr.threshold(thr, ip), rr.floor_sum(rr.threshold(thr, ip), pair, ip, tmin, cmax))
                    keep = rr.keep(p, codes, F(b), x, ip)
                    with np.errstate(invalid="ignore", over="ignore"):   # over, ip: the product before its rounding, which may overflow
                        admitted = (v >= thr) if ip else (v <= thr)
                        over = (float(thr) - (F(b) + s).astype(np.float64) * x) if ip else (v.astype(np.float64) - float(thr))
                    assert not (admitted & ~keep).any(), (name, pair, b, float(thr))     # left out: the exact f32 value misses
                    reg = keep & np.isfinite(x) & ((x >= 0) | (not ip))
                    if p["ulim"] == asr.PER_ROW and np.isfinite(b) and np.isfinite(thr):
                        lim = rr.slack(p, M, s.astype(np.float64), float(b), x.astype(np.float64), ip)
                        assert (over[reg] <= lim[reg]).all(), (name, pair, b, float(thr))
