"""GPU tests of the u8 table screen over resident codes (include/pqhip.h: pqhip_adc_screen_f32_dev) through
Pq.adc_screen_device, and of the batch search built on it (Pq.adc_search_batch_device, screen=True on QuantizedMatrix).
The screen against the f32-chain reference of tests/adc_screen_ref.py and the device's own range calls: ascending,
allowed rows only, a superset, within the stated slack; the capacity protocol; one result for every grid and grouping.
The batch search against the plain calls, bit for bit."""
import functools

import numpy as np
import pytest

import adc_screen_ref as asr
import synth
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
N = 4099            # 65 hit words, the last of 3 rows; 5 workgroups' worth of 1,024 rows
SHAPES = [(1, 256, 33), (15, 256, 70), (48, 256, 33), (7, 16, 1)]     # 32 and 8 slots per pass, an M that is no multiple of 4


@functools.lru_cache(maxsize=None)
def world(M, K, nq, ip):
    """skewed codes in rows M + 1 bytes apart, tables with a few small entries per subquantizer, thresholds near the 2 %
    quantile of each query with the special ones behind, scales and a mask; host copies beside the device tensors"""
    import torch
    rng = np.random.default_rng(7000 + M)
    codes = np.where(rng.random((N, M)) < 0.5, rng.integers(0, min(K, 4), (N, M)), rng.integers(0, K, (N, M))).astype(np.uint8)
    t = (rng.random((nq, M, K)) + 0.5).astype(np.float32)
    t[:, :, : min(K, 4)] *= np.float32(0.1)
    if ip:
        t = -t
    scales = (rng.random(N) + 0.5).astype(np.float32)
    allow = rng.random(N) < 0.7
    v = np.stack([asr.values(tq, codes.astype(np.int64), ip) for tq in t])
    thr = np.sort(v, axis=1)[:, -80 if ip else 80].copy()
    for q, s in zip(range(3, nq, 6), (np.nan, np.inf, -np.inf, v[0, 0] if nq > 21 else 0)):
        thr[q] = s
    buf = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")
    buf[:, :M] = torch.from_numpy(codes).cuda()
    return dict(codes=codes.astype(np.int64), t=t, scales=scales, allow=allow, thr=thr, cd=buf[:, :M], td=torch.from_numpy(t).cuda(),
                sd=torch.from_numpy(scales).cuda(), wd=dev_words(allow))


def check_screen(pq, w, ip, scaled, thr, got):
    """the contract of one call: per query ascending, allowed, a superset of the range call's ids, within the slack"""
    lims, idx = (a.cpu().numpy() for a in got)
    rng_call = pq.adc_ip_range_device if ip else pq.adc_range_device
    kw = {"scales": w["sd"]} if scaled else {}
    rl, _, ri = (a.cpu().numpy() for a in rng_call(w["cd"], w["td"], thr, allow=w["wd"], **kw))
    for q in range(w["t"].shape[0]):
        mine, want = idx[lims[q]:lims[q + 1]], ri[rl[q]:rl[q + 1]]
        assert (np.diff(mine) > 0).all() and w["allow"][mine].all()
        assert np.isin(want, mine).all(), q
        v = asr.values(w["t"][q], w["codes"], ip, w["scales"] if scaled else None)
        assert np.array_equal(want, np.flatnonzero(w["allow"] & ((v >= thr[q]) if ip else (v <= thr[q]))))   # the reference agrees
        M, p = w["t"].shape[1], asr.screen(w["t"][q], w["codes"], thr[q], ip, w["scales"] if scaled else None)[1]
        if not scaled and p["ulim"] not in (asr.KEEP_ALL, -1):
            over = (thr[q] - v[mine].astype(np.float64)) if ip else (v[mine].astype(np.float64) - thr[q])
            assert (over <= asr.slack(p, M) * (1 + 1e-9)).all(), q
        elif scaled and p["ulim"] == asr.PER_ROW:                          # the epilogue is no looser than stated
            c = w["scales"].astype(np.float64)[mine]
            ch, c = asr.chain(w["t"][q], w["codes"][mine]).astype(np.float64)[(c >= 0) & np.isfinite(c)], c[(c >= 0) & np.isfinite(c)]
            assert (float(thr[q]) - ch * c <= asr.slack(p, M, ch, c) * (1 + 1e-9)).all(), q


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,K,nq", SHAPES)
def test_gpu_adc_screen_contract_grids_and_capacity(ra, M, K, nq, ip, scaled):
    import torch
    pq, w = make_pq(ra, M, K), world(M, K, nq, ip)
    kw = dict(ip=ip, scales=w["sd"] if scaled else None, allow=w["wd"])
    thr = w["thr"]
    results = []
    try:
        for wgs in (1, 3):
            ra.set_option("adc_screen_wgs", wgs)
            results.append(pq.adc_screen_device(w["cd"], w["td"], thr, check=True, **kw))
    finally:
        ra.set_option("adc_screen_wgs", 0)
    check_screen(pq, w, ip, scaled, thr, results[0])
    same(results[1], results[0])                                          # the grid
    lims, idx = results[0]
    assert scaled or int(lims[1]) < N // 4                                # 80 rows qualify: the screen is selective here
    if nq > 40:                                                           # the grouping into passes
        a, b = (pq.adc_screen_device(w["cd"], w["td"][s], thr[s], **kw) for s in (slice(0, 40), slice(40, nq)))
        same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), (lims, idx))
    total = int(lims[-1])
    for cap in (0, total // 2):                                           # counts always, a valid prefix when short
        l2, i2, t2, _ = pq._adc_screen(w["cd"], w["td"], thr, ip, kw["scales"], w["wd"], cap, None, False)
        assert t2 == total and torch.equal(l2, lims) and torch.equal(i2, idx[:cap])


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_gpu_adc_screen_special_tables_scales_and_the_range_flag(ra, ip, scaled):
    import torch
    M, K, nq = 7, 16, 12
    from test_adc_screen import _tables
    pq, base = make_pq(ra, M, K), world(M, K, 1, ip)
    w = dict(base)
    t = np.stack([base["t"][0]] + list(_tables(M, K, 9).values()))         # the CPU test's adversarial tables
    sc = base["scales"].copy()
    sc[::5] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38], np.float32), sc[::5].size)
    v0 = asr.values(t[0], base["codes"], ip, sc if scaled else None)
    thr = np.full(nq, np.sort(v0[np.isfinite(v0)])[100], np.float32)
    thr[8:] = [np.nextafter(thr[0], np.float32(np.inf)), np.nextafter(thr[0], np.float32(-np.inf)), np.inf, -np.inf]
    w.update(t=t, td=torch.from_numpy(t).cuda(), scales=sc, sd=torch.from_numpy(sc).cuda())
    got = pq.adc_screen_device(w["cd"], w["td"], thr, ip=ip, scales=w["sd"] if scaled else None, allow=w["wd"], check=True)
    check_screen(pq, w, ip, scaled, thr, got)
    bad = w["cd"].clone()
    bad[N - 2, 3] = K                                                     # a code >= K in an allowed or disallowed row
    flags = torch.from_numpy(np.ones((N + 31) // 32, np.int32) * -1).cuda()
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.adc_screen_device(bad, w["td"], thr, ip=ip, allow=flags, check=True)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_gpu_adc_search_batch_equals_the_plain_search(ra, ip, scaled):
    import torch
    from reductive_amd import pq as rules
    M, K, nq = 15, 256, 70
    pq, w = make_pq(ra, M, K), world(M, K, nq, ip)
    kw = {"scales": w["sd"] if scaled else None} if ip else {}
    plain = pq.adc_ip_search_device if ip else pq.adc_search_device
    thin = np.zeros(N, bool)
    thin[[5, 17, 140, 2001]] = True
    for k, wd, fell in ((1, None, 0), (1, w["wd"], 0), (100, None, None), (1024, w["wd"], None), (3, dev_words(thin), nq)):
        stats = {}
        got = pq.adc_search_batch_device(w["cd"], w["td"], k, ip=ip, allow=wd, stats=stats, check=True, **kw)
        same(got, plain(w["cd"], w["td"], k, allow=wd, **kw))
        assert fell is None or stats["fallback_queries"] == fell, stats
    # the input meant for the screen route stays under the fallback share on the CPU model as well
    _, _, took_plain, _ = asr.ref_adc_search_batch(w["t"][:8], w["codes"], 1, rules.flat_batch_sample, rules.flat_batch_falls_back, ip,
                                                   w["scales"] if scaled else None)
    assert not took_plain.any()
    flat = torch.full_like(w["td"], 0.25) + w["td"] * 1e-9               # near-constant tables (and scales): the chunk falls back
    kwf = {"scales": torch.ones_like(w["sd"])} if scaled else kw
    stats = {}
    same(pq.adc_search_batch_device(w["cd"], flat, 5, ip=ip, stats=stats, **kwf), plain(w["cd"], flat, 5, **kwf))
    assert stats["fallback_queries"] == nq
    wide = make_pq(ra, 101, 4)                                            # no instantiation: PQHIP_EUNSUPPORTED, the plain call
    cd = torch.from_numpy(np.random.default_rng(3).integers(0, 4, (N, 101)).astype(np.uint8)).cuda()
    td = torch.from_numpy(synth.normalish(71, (9, 101, 4))).cuda()
    kw2 = {"scales": w["sd"] if scaled else None} if ip else {}
    with pytest.raises(ra.PqHipError, match="unsupported"):
        wide.adc_screen_device(cd, td, 0.0, ip=ip)
    same(wide.adc_search_batch_device(cd, td, 4, ip=ip, **kw2), (wide.adc_ip_search_device if ip else wide.adc_search_device)(cd, td, 4, **kw2))


def test_gpu_screen_route_of_the_quantized_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    M, K = 15, 256
    pq, w = make_pq(ra, M, K), world(M, K, 70, False)
    x = synth.normalish(72, (N, 4 * M))
    qm = qmatrix.QuantizedMatrix(pq, w["codes"].astype(np.uint8), norms=w["scales"]).attach_vectors(x)
    q = torch.from_numpy(x[:40] * np.float32(1.01)).cuda()
    for allow in (None, w["allow"]):
        same(qm.nearest(q, 1, allow=allow, screen=True), qm.nearest(q, 1, allow=allow))
        for use_norms in (True, False):
            same(qm.most_similar(q, 2, use_norms=use_norms, allow=allow, screen=True), qm.most_similar(q, 2, use_norms=use_norms, allow=allow))
    same(qm.nearest(q, 3, refine=20, screen=True), qm.nearest(q, 3, refine=20))
    same(qm.most_similar(q, 3, refine=20, screen=True), qm.most_similar(q, 3, refine=20))
    with pytest.raises(ra.PanicError, match="unpack4"):
        qmatrix.QuantizedMatrix(make_pq(ra, 7, 16), np.zeros((8, 7), np.uint8)).pack4().nearest(np.zeros(28, np.float32), 1, screen=True)
