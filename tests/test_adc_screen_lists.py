"""CPU tests of the u8 table screen in probed lists (pqhip_adc_screen_lists_f32_dev) and of the batch list search built
on it (Pq.adc_search_lists_batch_device): the names exist, bad arguments are refused before the library is reached, and
the composition -- sample, model screen, resolve -- over the numpy references equals the plain list reference."""
import os

import numpy as np
import pytest

import adc_screen_ref as asr
from adc_among_ref import ref_among
from adc_lists_ref import probed_positions, ref_lists_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_adc_screen_lists_f32_dev"


def ref_adc_search_lists_batch(tables, codes, list_off, probes, k, rules, ip=False, scales=None, allow=None):
    """(value, idx, plain, share): the composition of Pq.adc_search_lists_batch_device over the references; plain: the
    queries that took the plain call; share: candidates over the expected probed rows, what the fallback rule reads"""
    nq, n, n_lists, n_probe = tables.shape[0], codes.shape[0], len(list_off) - 1, probes.shape[1]
    flags = np.ones(n, bool) if allow is None else np.asarray(allow, bool)
    s = np.stack([asr.chain(tq, codes) for tq in tables])
    rows_of = lambda pr: [(lambda p: p[flags[p]])(probed_positions(list_off, pr[q], n)) for q in range(nq)]
    csr = lambda rows: (np.concatenate(rows) if rows else np.zeros(0, np.int64),
                        np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64))
    among = lambda rows: ref_among(s, *csr(rows)[:1], k, lims=csr(rows)[1], ip=ip, extra=scales)[:2]
    want = among(rows_of(probes))
    slots = rules.flat_lists_batch_sample(n, n_lists, n_probe, k)
    sv, si = among(rows_of(probes[:, :slots]))
    srt = np.sort(probes, axis=1)
    thin = (si[:, k - 1] < 0) | np.isnan(sv[:, k - 1]) | ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any(1)
    # the scaled step reads the largest scale of the CALL, so the model screens every row and the probed ones are picked
    keep = [r[asr.screen(tables[q], codes, sv[q, k - 1], ip, scales)[0][r] & ~thin[q]] for q, r in enumerate(rows_of(probes))]
    total = sum(r.size for r in keep)
    plain = thin | rules.flat_lists_batch_falls_back(total, n, n_lists, n_probe, nq)
    val, idx = among(keep)
    val[plain], idx[plain] = want[0][plain], want[1][plain]
    return val, idx, plain, total / (float(nq) * n * min(n_probe, n_lists) / n_lists), want


def test_names_exist_in_the_wrapper_and_the_header():
    from reductive_amd import _lib, pq, qmatrix
    for name in ("adc_screen_lists_device", "adc_search_lists_batch_device", "_adc_screen_lists"):
        assert callable(getattr(pq.Pq, name))
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 21
    header = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    assert "int32_t %s(" % NAME in header
    for option in ("adc_screen_lists_wgs", "adc_screen_lists_unit_rows", "adc_screen_lists_chunk_queries"):
        assert '"%s"' % option in header
    import inspect
    for fn in (qmatrix.PartitionedMatrix.nearest, qmatrix.PartitionedMatrix.most_similar):
        assert inspect.signature(fn).parameters["screen"].default is False


@pytest.mark.parametrize("what", ["codes", "tables", "scales", "list_off", "probes", "host tensors", "capacity", "k"])
def test_bad_arguments_are_refused_before_the_library(what, monkeypatch):
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    a = dict(codes=torch.zeros((8, 3), dtype=torch.uint8), tables=torch.zeros((2, 3, 16)), list_off=torch.tensor([0, 4, 8]),
             probes=torch.zeros((2, 1), dtype=torch.int64), threshold=0.5)
    bad = dict(codes=a["codes"].to(torch.int32), tables=a["tables"][:, :, :8], list_off=a["list_off"].to(torch.int32), probes=a["probes"][:1])
    if what in bad:
        a[what] = bad[what]
    with pytest.raises(ra.PanicError):          # whatever passes the shape checks is refused as a host tensor, still before the library
        if what == "k":
            pq.adc_search_lists_batch_device(a["codes"], a["tables"], a["list_off"], a["probes"], 0)
        else:
            pq.adc_screen_lists_device(*a.values(), capacity=-1 if what == "capacity" else None, scales=torch.ones(8) if what == "scales" else None)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_the_composition_over_the_references_equals_the_plain_list_reference(ip, scaled):
    from reductive_amd import pq as rules
    rng = np.random.default_rng(11)
    M, K, n, nq = 5, 16, 900, 9
    list_off = np.array([0, 0, 200, 450, 451, 900], np.int64)
    codes = rng.integers(0, 3, (n, M)).astype(np.int64)                    # 3^5 distinct rows: ties everywhere
    t = rng.integers(-2, 3, (nq, M, K)).astype(np.float32)
    t[1] *= np.float32(-0.0)                                               # every value a zero: -0 in the scores, all tied
    t[2, 1, 2] = np.nan                                                    # NaN values among the rows of one query
    probes = np.array([[4, 2], [2, 4], [1, 3], [3, 3], [4, -1], [0, 1], [2, 3], [4, 9], [2, 4]], np.int64)
    scales = np.where(rng.random(n) < 0.1, 0.0, rng.random(n) + 0.5).astype(np.float32) if scaled else None
    for k in (1, 7, 300):
        val, idx, plain, _, _ = ref_adc_search_lists_batch(t, codes, list_off, probes, k, rules, ip, scales)
        v = np.stack([asr.values(tq, codes, ip, scales) for tq in t])
        wv, wi = ref_lists_search(v, list_off, probes, k, ip=ip)         # the doubled probe has its rows twice in both
        assert np.array_equal(idx, wi) and val.tobytes() == wv.tobytes(), k
        assert plain[3]
