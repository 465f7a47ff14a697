"""GPU tests of pqhip_adc_screen_lists_residual_f32_dev, Pq.adc_search_lists_residual_batch_device and screen=True on
ResidualPartitionedMatrix: the screen equals the model of tests/adc_screen_residual_ref.py, the searches the plain ones."""
import functools

import numpy as np
import pytest

import adc_screen_ref as asr
import adc_screen_residual_ref as rr
import synth
from adc_residual_ref import probe_slots, residual_values
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
MODES = [(False, False), (True, False), (True, True)]                      # (ip, scaled)
# (M, K, list lengths, queries): 32 slots with two groups on the long list; 8 slots; the M of the usual index
SHAPES = {"m5": (5, 16, [0, 1, 63, 64, 65, 507], 35), "m48": (48, 256, [0, 1, 63, 64, 65, 107], 9), "m15": (15, 256, [0, 1, 63, 64, 65, 107], 3)}
OPTIONS = ("adc_screen_lists_wgs", "adc_screen_lists_unit_rows", "adc_screen_lists_chunk_queries")


def cuda(a):
    import torch
    return None if a is None else torch.from_numpy(a).cuda()


def build(M, K, lens, probes, bias, ip, scaled, seed):
    """random codes (ten equal rows) and tables over lists of `lens` rows, terms (distances) or scales (scaled), a mask, the list of
    every row: host arrays and their device copies"""
    rng, n, nq = np.random.default_rng(seed), sum(lens), len(probes)
    w = dict(M=M, K=K, n=n, nq=nq, off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), probes=probes, bias=bias.astype(np.float32),
             codes=rng.integers(0, K, (n, M)), t=(rng.random((nq, M, K)) * 2 - 1).astype(np.float32), allow=rng.random(n) < 0.75,
             terms=None if ip else (rng.standard_normal(n) * M / 4).astype(np.float32), scales=(rng.random(n) + 0.5).astype(np.float32) if scaled else None)
    w["codes"][n // 2:n // 2 + 10] = w["codes"][n // 2]
    return dict(w, cd=cuda(w["codes"].astype(np.uint8)), td=cuda(w["t"]), od=cuda(w["off"]), pd=cuda(probes), bd=cuda(w["bias"]), xd=cuda(w["terms"]),
                sd=cuda(w["scales"]), wd=dev_words(w["allow"]), ld=cuda(np.repeat(np.arange(len(lens)), lens)))


@functools.lru_cache(maxsize=None)
def world(shape, ip, scaled):
    """every query probes the long list and two others (-1 pads in two); biases further apart than the table span; thresholds at a
    quantile of the exact values; codes of unprobed and disallowed rows poisoned (K = 16: reading one raises the flag)"""
    M, K, lens, nq = SHAPES[shape]
    rng, long_list = np.random.default_rng(4200 + M), len(lens) - 1
    probes = np.stack([np.roll(np.concatenate([[long_list], rng.permutation(long_list)[:2]]), q % 3) for q in range(nq)])
    probes[1, (np.flatnonzero(probes[1] != long_list))[0]], probes[2, (np.flatnonzero(probes[2] != long_list))] = -1, -1
    w = build(M, K, lens, probes, rng.standard_normal((nq, 3)) * 3 * M, ip, scaled, 4300 + M)
    v = residual_values(np.stack([asr.chain(tq, w["codes"]) for tq in w["t"]]), w["off"], probes, w["bias"], terms=w["terms"], scales=w["scales"], ip=ip)
    thr, probed, mixed = np.zeros(nq, np.float32), np.zeros(w["n"], bool), 0
    for q in range(nq):
        on = (probe_slots(w["off"], probes[q], w["n"]) >= 0) & w["allow"]
        probed |= on
        thr[q] = np.quantile(v[q, on], 0.7 if ip else 0.3, method="nearest")
        mixed += 0 < int(((v[q, on] >= thr[q]) if ip else (v[q, on] <= thr[q])).sum()) < int(on.sum())
    assert 2 * mixed >= nq                                                 # the exact result is neither empty nor everything
    return dict(w, thr=thr, cd=cuda(np.where(probed[:, None], w["codes"], 255).astype(np.uint8)))


def screen(pq, w, ip, s=slice(None), check=False, thr=None):
    return pq.adc_screen_lists_residual_device(w["cd"], w["td"][s], w["od"], w["pd"][s], w["bd"][s], w["xd"], (w["thr"] if thr is None else thr)[s], ip=ip,
                                               scales=w["sd"], allow=w["wd"], check=check)


def equals_model(got, w, ip, thr=None):
    want = rr.ref_screen(w["t"], w["codes"], w["off"], w["probes"], w["bias"], w["thr"] if thr is None else thr, ip, w["terms"], w["scales"], w["allow"])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    return want


@pytest.mark.parametrize("ip,scaled", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_residual_screen_model_superset_capacity_and_one_result_for_every_split(ra, shape, ip, scaled):
    import torch
    pq, w = make_pq(ra, *SHAPES[shape][:2]), world(shape, ip, scaled)
    try:
        ra.set_option("adc_screen_lists_unit_rows", 128)                   # the long list of m5 spans four units
        lims, idx = screen(pq, w, ip, check=True)                          # check=True: no poisoned row was read
        want = equals_model((lims, idx), w, ip)
        rng_call = pq.adc_ip_range_lists_residual_device if ip else pq.adc_range_lists_residual_device
        rl, _, ri = (a.cpu().numpy() for a in rng_call(w["cd"], w["td"], w["od"], w["pd"], w["bd"], *(() if ip else (w["xd"],)), w["thr"],
                                                       allow=w["wd"], **(dict(scales=w["sd"]) if ip else {})))
        for q in range(w["nq"]):                                           # a superset, in the range call's order
            mine, exact = want[1][want[0][q]:want[0][q + 1]], ri[rl[q]:rl[q + 1]]
            assert np.array_equal(mine[np.isin(mine, exact)], exact), q
        total = int(lims[-1])
        for cap in (0, total // 2, total):                                 # counts always, a valid prefix when short
            l2, i2, t2, _ = pq._adc_screen_lists_residual(w["cd"], w["td"], w["od"], w["pd"], w["bd"], w["xd"], w["thr"], ip, w["sd"],
                                                          w["wd"], cap, None, False)
            assert t2 == total and torch.equal(l2, lims) and torch.equal(i2, idx[:cap])
        for values in ((1, 64, 1), (3, 128, 4), (0, 64, 0)):               # grid, unit rows, chunk queries
            for name, v in zip(OPTIONS, values):
                ra.set_option(name, v)
            same(screen(pq, w, ip), (lims, idx))
        a, b = screen(pq, w, ip, slice(0, 2)), screen(pq, w, ip, slice(2, None))
        same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), (lims, idx))
    finally:
        for name in OPTIONS:
            ra.set_option(name, 0)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, True)])
def test_gpu_residual_screen_pairs_beyond_the_hit_word_budget(ra, ip, scaled):
    # a list of 4,000 rows probed by every query, 8 budgeted words against a pair's 125: the same rows spread over 63 lists, and the model
    rng, nq, one = np.random.default_rng(6), 33, np.zeros((33, 1), np.int64)
    b, even_off = rng.standard_normal(nq), np.concatenate([np.arange(0, 4000, 64), [4000, 4099]]).astype(np.int64)
    w = build(15, 256, [4000] + [2] * 36 + [1] * 27, one, b[:, None], ip, scaled, 7)
    v = residual_values(np.stack([asr.chain(tq, w["codes"]) for tq in w["t"]]), w["off"], one, w["bias"], terms=w["terms"], scales=w["scales"], ip=ip)
    w["thr"] = np.sort(v[:, :4000][:, w["allow"][:4000]], axis=1)[:, -40 if ip else 40].copy()
    spread = dict(w, od=cuda(even_off), pd=cuda(np.tile(np.arange(63), (nq, 1))), bd=cuda(np.repeat(w["bias"], 63, axis=1)))
    got = screen(make_pq(ra, 15, 256), w, ip, check=True)
    same(got, screen(make_pq(ra, 15, 256), spread, ip, check=True))
    equals_model(got, w, ip)


@pytest.mark.parametrize("ip,scaled", MODES)
def test_gpu_residual_screen_returns_what_the_proof_does_not_cover_and_raises_the_flag(ra, ip, scaled):
    pq, w = make_pq(ra, 5, 16), dict(world("m5", ip, scaled))
    w.update(t=w["t"].copy(), bias=w["bias"].copy(), thr=w["thr"].copy(), scales=None if not scaled else w["scales"].copy())
    w["t"][0, 2, 3], w["bias"][3, 1], w["thr"][4] = np.nan, np.nan, np.nan  # a table entry, the bias of one slot, a threshold
    if scaled:
        w["scales"][::9] = -1.0                                            # a negative scale: returned wherever it is probed
    w.update(td=cuda(w["t"]), bd=cuda(w["bias"]), sd=cuda(w["scales"]))
    lims, idx = equals_model(screen(pq, w, ip), w, ip)
    every = equals_model(screen(pq, w, ip, thr=np.full(w["nq"], -np.inf if ip else np.inf, np.float32)), w, ip, np.full(w["nq"], -np.inf if ip else np.inf))
    for q in (0, 4):                                                       # every allowed probed row
        assert np.array_equal(idx[lims[q]:lims[q + 1]], every[1][every[0][q]:every[0][q + 1]]), q
    bad_codes, allowed, bad_probes = w["cd"].clone(), w["allow"].copy(), w["probes"].copy()
    bad_codes[-1, 0], allowed[-1], bad_probes[5, 0] = 200, True, 99        # the last row of the long list, allowed; a list id out of range
    for w2 in (dict(w, cd=bad_codes, wd=dev_words(allowed)), dict(w, pd=cuda(bad_probes))):
        screen(pq, w2, ip)                                                 # served: entry 0 resp. the slot skipped
        with pytest.raises(ra.PanicError, match="out of"):
            screen(pq, w2, ip, check=True)


@pytest.mark.parametrize("k,masked", [(1, False), (10, True), (64, True)])
@pytest.mark.parametrize("ip,scaled", MODES)
def test_gpu_residual_batch_search_equals_the_plain_search(ra, ip, scaled, k, masked):
    # 39 lists of 200 rows and one of 5; biases 200 apart in probe order; query 3 names a list twice, query 4 probes the short list alone
    rng, n_probe = np.random.default_rng(77), 12
    probes = np.stack([rng.permutation(39)[:n_probe] for _ in range(24)])
    probes[3, 5], probes[4] = probes[3, 1], [39] + [-1] * (n_probe - 1)
    w = build(15, 256, [200] * 39 + [5], probes, (-200.0 if ip else 200.0) * np.arange(n_probe)[None, :] + rng.standard_normal((24, n_probe)), ip, scaled, 78)
    pq, wd, stats, kw = make_pq(ra, 15, 256), (w["wd"] if masked else None), {}, (dict(scales=w["sd"]) if ip else {})
    plain = pq.adc_ip_search_lists_residual_device if ip else pq.adc_search_lists_residual_device
    want = plain(w["cd"], w["td"], w["od"], w["pd"], w["bd"], *(() if ip else (w["xd"],)), k, allow=wd, **kw)
    same(pq.adc_search_lists_residual_batch_device(w["cd"], w["td"], w["od"], w["pd"], w["bd"], w["xd"], w["ld"], k, ip=ip, allow=wd, stats=stats,
                                                   check=True, **kw), want)
    assert stats["fallback_queries"] == (2 if k > 5 else 1), stats       # the doubled probe (and the short list): the rest was screened


def test_gpu_screen_route_of_the_residual_partitioned_matrix(ra):
    from reductive_amd import qmatrix
    n, rng, x = 4000, np.random.default_rng(9), synth.normalish(91, (4000, 32))
    flat = ra.train_pq(8, 4, 3, 1, x, rng=np.random.default_rng(1))
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x), norms=(rng.random(n) + 0.5).astype(np.float32))
    rm = qm.partition_residual(16, n_iterations=3, pq_iterations=3, vectors=x, rng=np.random.default_rng(2)).attach_vectors(x)
    q = cuda(x[:40] * np.float32(1.01))
    for a, refine in ((None, None), (rng.random(n) < 0.7, None), (None, 20), (rng.random(n) < 0.7, 20)):
        same(rm.nearest(q, 3, 5, refine=refine, allow=a, screen=True), rm.nearest(q, 3, 5, refine=refine, allow=a))
        for use_norms in (True, False):
            same(rm.most_similar(q, 3, 5, use_norms=use_norms, refine=refine, allow=a, screen=True),
                 rm.most_similar(q, 3, 5, use_norms=use_norms, refine=refine, allow=a))
