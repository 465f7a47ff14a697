"""GPU tests of the u8 table screen in probed lists (pqhip_adc_screen_lists_f32_dev) through Pq.adc_screen_lists_device,
and of the batch list search built on it (Pq.adc_search_lists_batch_device, screen=True on PartitionedMatrix).  The screen
against the f32-chain reference of tests/adc_screen_ref.py and the device's own list range calls: probe slot first then
position, allowed probed rows only, a superset, within the stated slack; the capacity protocol; one result for every
grid, unit size, chunk and split of the queries; pairs beyond the hit-word budget.  The batch search against the plain
calls, bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import adc_screen_ref as asr
import synth
from adc_lists_ref import probed_positions
from test_adc_screen_lists import ref_adc_search_lists_batch
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
LENS = [0, 1, 63, 64, 65, 700, 2100, 228]     # empty, one row, both sides of a 64-row step, tiles at every bit offset of the mask
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N = int(OFF[-1])
SHAPES = [(1, 256), (15, 256), (48, 256), (7, 16)]                         # 32 and 8 slots per group, an M that is no multiple of 4
BATCHES = [(1, 1), (33, 3), (70, 7)]                                       # list 6 has more pairs than a group of 32 / of 8 holds
OPTIONS = ("adc_screen_lists_wgs", "adc_screen_lists_unit_rows", "adc_screen_lists_chunk_queries")


@functools.lru_cache(maxsize=None)
def world(M, K, nq, n_probe, ip):
    """skewed codes in rows M + 1 bytes apart, tables with a few small entries per subquantizer, every query probing the
    long list and n_probe - 1 others in a rotated order, thresholds at the 21st best probed allowed row with the special
    ones behind, scales and a mask; the codes of unprobed and of disallowed rows are poisoned where a byte can be >= K"""
    import torch
    rng = np.random.default_rng(7100 + M)
    codes = np.where(rng.random((N, M)) < 0.5, rng.integers(0, min(K, 4), (N, M)), rng.integers(0, K, (N, M))).astype(np.uint8)
    t = (rng.random((nq, M, K)) + 0.5).astype(np.float32)
    t[:, :, : min(K, 4)] *= np.float32(0.1)
    if ip:
        t = -t
    scales = (rng.random(N) + 0.5).astype(np.float32)
    allow = rng.random(N) < 0.7
    others = [l for l in range(len(LENS)) if l != 6]
    probes = np.stack([np.roll(np.concatenate([[6], rng.permutation(others)[: n_probe - 1]]), q % n_probe) for q in range(nq)])
    if nq > 2 and n_probe > 1:
        probes[2, -1] = -1                                                 # padding
    v = np.stack([asr.values(tq, codes.astype(np.int64), ip) for tq in t])
    thr = np.zeros(nq, np.float32)
    probed = np.zeros(N, bool)
    for q in range(nq):
        pos = probed_positions(OFF, probes[q], N)
        probed[pos] = True
        thr[q] = np.sort(v[q, pos[allow[pos]]])[-21 if ip else 20]
    for q, s in zip(range(3, nq, 6), (np.nan, np.inf, -np.inf, np.nextafter(thr[0], np.float32(np.inf)), np.nextafter(thr[0], np.float32(-np.inf)))):
        thr[q] = s
    poisoned = codes.copy()
    poisoned[~(probed & allow)] = 255                                      # K = 16: reading one of them raises the range flag
    buf = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")
    buf[:, :M] = torch.from_numpy(poisoned).cuda()
    return dict(codes=codes.astype(np.int64), t=t, scales=scales, allow=allow, thr=thr, probes=probes, cd=buf[:, :M],
                td=torch.from_numpy(t).cuda(), sd=torch.from_numpy(scales).cuda(), wd=dev_words(allow), od=torch.from_numpy(OFF).cuda(),
                pd=torch.from_numpy(probes).cuda())


def check_screen(pq, w, ip, scaled, thr, got, off=OFF, od=None):
    """the contract of one call: per query a subsequence of the allowed probed rows in probe order, a superset of the
    list range call's positions, within the slack"""
    lims, idx = (a.cpu().numpy() for a in got)
    rng_call = pq.adc_ip_range_lists_device if ip else pq.adc_range_lists_device
    kw = {"scales": w["sd"]} if scaled else {}
    rl, _, ri = (a.cpu().numpy() for a in rng_call(w["cd"], w["td"], w["od"] if od is None else od, w["pd"], thr, allow=w["wd"], **kw))
    for q in range(w["t"].shape[0]):
        mine, want = idx[lims[q]:lims[q + 1]], ri[rl[q]:rl[q + 1]]
        pos = probed_positions(off, w["probes"][q], N)
        S = pos[w["allow"][pos]]
        v = asr.values(w["t"][q], w["codes"], ip, w["scales"] if scaled else None)
        keep, p = asr.screen(w["t"][q], w["codes"], thr[q], ip, w["scales"] if scaled else None)
        assert np.array_equal(want, S[(v[S] >= thr[q]) if ip else (v[S] <= thr[q])]), q        # the reference agrees
        assert np.array_equal(mine, S[keep[S]]), q                         # order, allowed probed rows only, the model's integers
        assert np.isin(want, mine).all(), q
        M = w["t"].shape[1]
        if not scaled and p["ulim"] not in (asr.KEEP_ALL, -1):
            over = (thr[q] - v[mine].astype(np.float64)) if ip else (v[mine].astype(np.float64) - thr[q])
            assert (over <= asr.slack(p, M) * (1 + 1e-9)).all(), q
        elif scaled and p["ulim"] == asr.PER_ROW:
            c = w["scales"].astype(np.float64)[mine]
            ch, c = asr.chain(w["t"][q], w["codes"][mine]).astype(np.float64)[(c >= 0) & np.isfinite(c)], c[(c >= 0) & np.isfinite(c)]
            assert (float(thr[q]) - ch * c <= asr.slack(p, M, ch, c) * (1 + 1e-9)).all(), q


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("nq,n_probe", BATCHES)
@pytest.mark.parametrize("M,K", SHAPES)
def test_gpu_adc_screen_lists_contract_and_capacity(ra, M, K, nq, n_probe, ip, scaled):
    import torch
    from reductive_amd import _lib
    pq, w = make_pq(ra, M, K), world(M, K, nq, n_probe, ip)
    sd = w["sd"] if scaled else None
    got = pq.adc_screen_lists_device(w["cd"], w["td"], w["od"], w["pd"], w["thr"], ip=ip, scales=sd, allow=w["wd"], check=True)
    check_screen(pq, w, ip, scaled, w["thr"], got)                         # check=True: no poisoned row was read
    lims, idx = got
    total = int(lims[-1])
    for cap in (0, total // 2, total):                                     # counts always, a valid prefix when short
        l2, i2, t2, _ = pq._adc_screen_lists(w["cd"], w["td"], w["od"], w["pd"], w["thr"], ip, sd, w["wd"], cap, None, False)
        assert t2 == total and torch.equal(l2, lims) and torch.equal(i2, idx[:cap])
    out = torch.full((total // 2 + 8,), -7, dtype=torch.int64, device="cuda")   # sentinels behind a short capacity stay
    td, ld = torch.from_numpy(w["thr"]).cuda(), torch.empty_like(lims)       # alive across the call
    rc = _lib.lib().pqhip_adc_screen_lists_f32_dev(
        pq._cb(), pq._slot_for(w["cd"]), w["td"].data_ptr(), nq, w["cd"].data_ptr(), 1, N, M + 1, w["wd"].data_ptr(), w["od"].data_ptr(), len(LENS),
        w["pd"].data_ptr(), n_probe, n_probe, int(ip), sd.data_ptr() if scaled else None, td.data_ptr(),
        ld.data_ptr(), out.data_ptr(), total // 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out[: total // 2], idx[: total // 2]) and bool((out[total // 2:] == -7).all())


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, True)])
@pytest.mark.parametrize("M,K", SHAPES)
def test_gpu_adc_screen_lists_one_result_for_every_grid_unit_chunk_and_split(ra, M, K, ip, scaled):
    import torch
    nq, n_probe = BATCHES[2]
    pq, w = make_pq(ra, M, K), world(M, K, nq, n_probe, ip)
    call = lambda s=slice(None): pq.adc_screen_lists_device(w["cd"], w["td"][s], w["od"], w["pd"][s], w["thr"][s], ip=ip,
                                                            scales=w["sd"] if scaled else None, allow=w["wd"])
    want = call()
    try:
        for values in ((1, 64, 1), (3, 128, 32), (1, 128, 0), (0, 64, 0)):  # one workgroup keeps the image from unit to unit
            for name, v in zip(OPTIONS, values):
                ra.set_option(name, v)
            same(call(), want)
    finally:
        for name in OPTIONS:
            ra.set_option(name, 0)
    a, b = call(slice(0, 40)), call(slice(40, nq))
    same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), want)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_gpu_adc_screen_lists_special_tables_scales_bad_lists_and_the_range_flag(ra, ip, scaled):
    import torch
    from test_adc_screen import _tables
    M, K, nq, n_probe = 7, 16, 12, 3
    pq, base = make_pq(ra, M, K), world(M, K, 33, 3, ip)
    w = dict(base)
    t = np.stack([base["t"][0]] + list(_tables(M, K, 9).values()))         # the CPU test's adversarial tables
    sc = base["scales"].copy()
    sc[::5] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38], np.float32), sc[::5].size)
    v0 = asr.values(t[0], base["codes"], ip, sc if scaled else None)
    thr = np.full(nq, np.sort(v0[np.isfinite(v0)])[100], np.float32)
    thr[8:] = [np.nextafter(thr[0], np.float32(np.inf)), np.nextafter(thr[0], np.float32(-np.inf)), np.inf, -np.inf]
    w.update(t=t, td=torch.from_numpy(t).cuda(), scales=sc, sd=torch.from_numpy(sc).cuda(), probes=base["probes"][:nq], pd=base["pd"][:nq])
    kw = dict(ip=ip, scales=w["sd"] if scaled else None, allow=w["wd"])
    check_screen(pq, w, ip, scaled, thr, pq.adc_screen_lists_device(w["cd"], w["td"], w["od"], w["pd"], thr, check=True, **kw))
    # ids out of range, a list named twice, clamped and inverted offsets: skipped resp. clamped, and flagged
    probes = w["probes"].copy()
    probes[0], probes[1], probes[4] = [6, 8, 5], [5, 5, -4], [7, 6, 7]
    off = OFF.copy()
    off[3], off[8] = off[4] + 5, N + 40                                    # list 2 inverted, list 3 shifted, list 7 past the end
    clean = np.ones(N, bool)                                               # no poison here: other rows are probed now
    cd = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")
    cd[:, :M] = torch.from_numpy(base["codes"].astype(np.uint8)).cuda()
    for pr, of in ((probes, OFF), (w["probes"], off)):
        w2 = dict(w, probes=pr, pd=torch.from_numpy(pr).cuda(), cd=cd[:, :M], allow=clean, wd=dev_words(clean))
        od = torch.from_numpy(of).cuda()
        kw2 = dict(kw, allow=w2["wd"])
        check_screen(pq, w2, ip, scaled, thr, pq.adc_screen_lists_device(w2["cd"], w2["td"], od, w2["pd"], thr, **kw2), of, od)
        with pytest.raises(ra.PanicError, match="out of"):
            pq.adc_screen_lists_device(w2["cd"], w2["td"], od, w2["pd"], thr, check=True, **kw2)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, True)])
def test_gpu_adc_screen_lists_pairs_beyond_the_hit_word_budget(ra, ip, scaled):
    """one list of 4,000 of 4,099 rows, probed by every query: 8 budgeted words per query against a pair's 125, so the
    fill pass forms most pairs again -- the result of the rows spread over 63 lists (within the budget), and the model's"""
    import torch
    M, K, nq, n = 15, 256, 33, 4099
    pq, base = make_pq(ra, M, K), world(M, K, 33, 3, ip)
    rng = np.random.default_rng(5)
    codes = np.where(rng.random((n, M)) < 0.5, rng.integers(0, 4, (n, M)), rng.integers(0, K, (n, M))).astype(np.uint8)
    allow = rng.random(n) < 0.7
    sc = (rng.random(n) + 0.5).astype(np.float32)
    long_off = np.concatenate([[0, 4000], 4000 + np.cumsum([2] * 36 + [1] * 27)]).astype(np.int64)
    even_off = np.concatenate([np.arange(0, 4000, 64), [4000, 4099]]).astype(np.int64)       # 62 lists of 64, one of 32, one of 99
    v = np.stack([asr.values(tq, codes.astype(np.int64), ip, sc if scaled else None) for tq in base["t"]])
    thr = np.sort(v[:, :4000][:, allow[:4000]], axis=1)[:, -40 if ip else 40].copy()
    cd, td = torch.from_numpy(codes).cuda(), base["td"]
    kw = dict(ip=ip, scales=torch.from_numpy(sc).cuda() if scaled else None, allow=dev_words(allow))
    got = []
    for off, pr in ((long_off, np.zeros((nq, 1), np.int64)), (even_off, np.tile(np.arange(63), (nq, 1)))):
        got.append(pq.adc_screen_lists_device(cd, td, torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda(), thr, check=True, **kw))
    same(got[0], got[1])
    lims, idx = (a.cpu().numpy() for a in got[0])
    for q in range(nq):
        keep = asr.screen(base["t"][q], codes.astype(np.int64), thr[q], ip, sc if scaled else None)[0]
        assert np.array_equal(idx[lims[q]:lims[q + 1]], np.flatnonzero(keep[:4000] & allow[:4000])), q


@functools.lru_cache(maxsize=None)
def batch_world(ip):
    """20,000 rows in 40 lists of 500 around list centres: a query near a centre has its best rows in few lists"""
    import torch
    rng = np.random.default_rng(31)
    M, K, n, nq = 15, 256, 20000, 70
    t = (rng.random((nq, M, K)) * 4 + 1).astype(np.float32)
    t[:, :, :8] *= np.float32(0.02)                                        # eight good centroids per subquantizer
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    near = rng.random((n, M)) < np.repeat(np.linspace(0.9, 0.1, 40), 500)[:, None]   # the lists differ in how good their rows are
    codes[near] = rng.integers(0, 8, int(near.sum())).astype(np.uint8)
    codes[1000:1010] = codes[1000]                                         # duplicate rows: ties
    if ip:
        t = -t
    scales = (rng.random(n) * 0.2 + 0.9).astype(np.float32)
    allow = rng.random(n) < 0.8
    probes = np.stack([np.concatenate([[q % 3], rng.permutation(np.delete(np.arange(40), q % 3))[:23]]) for q in range(nq)])   # good rows first
    probes[5, 7] = probes[5, 2]                                            # a doubled probe
    return dict(M=M, K=K, t=t, codes=codes, scales=scales, allow=allow, probes=probes, off=np.arange(0, n + 1, 500, dtype=np.int64),
                cd=torch.from_numpy(codes).cuda(), td=torch.from_numpy(t).cuda(), sd=torch.from_numpy(scales).cuda(),
                wd=dev_words(allow), od=torch.arange(0, n + 1, 500, device="cuda"), pd=torch.from_numpy(probes).cuda())


@pytest.mark.parametrize("k,masked,fell", [(1, False, 1), (10, True, 1), (128, False, None), (1024, True, None)])
@pytest.mark.parametrize("ip,scaled", [(False, False), (True, False), (True, True)])
def test_gpu_adc_search_lists_batch_equals_the_plain_list_search(ra, ip, scaled, k, masked, fell):
    from reductive_amd import pq as rules
    w = batch_world(ip)
    pq = make_pq(ra, w["M"], w["K"])
    kw = {"scales": w["sd"] if scaled else None} if ip else {}
    plain = pq.adc_ip_search_lists_device if ip else pq.adc_search_lists_device
    wd = w["wd"] if masked else None
    stats = {}
    got = pq.adc_search_lists_batch_device(w["cd"], w["td"], w["od"], w["pd"], k, ip=ip, allow=wd, stats=stats, check=True, **kw)
    same(got, plain(w["cd"], w["td"], w["od"], w["pd"], k, allow=wd, **kw))
    print("k %d candidates %d fallback %d of 70, sample slots %d" % (k, stats["candidates"], stats["fallback_queries"], stats["sample_slots"]))
    assert fell is None or stats["fallback_queries"] == fell, stats       # the doubled probe alone: the rest went through the screen
    if fell is not None:                                                   # and the numpy model says so too
        _, _, took_plain, share, _ = ref_adc_search_lists_batch(w["t"][:8], w["codes"].astype(np.int64), w["off"], w["probes"][:8], k, rules,
                                                                ip, w["scales"] if scaled else None, w["allow"] if masked else None)
        assert share < rules.flat_lists_batch_fraction() and took_plain.tolist() == [False] * 5 + [True, False, False]


def test_gpu_adc_search_lists_batch_thin_samples_and_short_lists(ra):
    import torch
    w = batch_world(False)
    pq = make_pq(ra, w["M"], w["K"])
    few = np.zeros(20000, bool)
    few[[5, 17, 640, 12001]] = True                                        # thin: fewer than k allowed rows in the sample
    stats = {}
    got = pq.adc_search_lists_batch_device(w["cd"], w["td"], w["od"], w["pd"], 3, allow=dev_words(few), stats=stats)
    same(got, pq.adc_search_lists_device(w["cd"], w["td"], w["od"], w["pd"], 3, allow=dev_words(few)))
    assert stats["fallback_queries"] == 70
    od, pd = torch.arange(0, 1001, 500, device="cuda"), torch.zeros((70, 1), dtype=torch.int64, device="cuda")
    same(pq.adc_search_lists_batch_device(w["cd"][:1000], w["td"], od, pd, 1024),          # k above the probed rows
         pq.adc_search_lists_device(w["cd"][:1000], w["td"], od, pd, 1024))


def test_gpu_screen_route_of_the_partitioned_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    M, K, n = 15, 256, 6000
    pq = make_pq(ra, M, K)
    x = synth.normalish(73, (n, 4 * M))
    rng = np.random.default_rng(9)
    qm = qmatrix.QuantizedMatrix(pq, rng.integers(0, K, (n, M)).astype(np.uint8), norms=(rng.random(n) + 0.5).astype(np.float32))
    pm = qmatrix.PartitionedMatrix(qm.attach_vectors(x), x[:12].copy(), rng.integers(0, 12, n))
    pm.vectors = qm.vectors                                                # as QuantizedMatrix.partition hands them on
    q = torch.from_numpy(x[:40] * np.float32(1.01)).cuda()
    allow = rng.random(n) < 0.7
    for a in (None, allow):
        same(pm.nearest(q, 2, 5, allow=a, screen=True), pm.nearest(q, 2, 5, allow=a))
        for use_norms in (True, False):
            same(pm.most_similar(q, 2, 5, use_norms=use_norms, allow=a, screen=True), pm.most_similar(q, 2, 5, use_norms=use_norms, allow=a))
    same(pm.nearest(q, 3, 5, refine=20, screen=True), pm.nearest(q, 3, 5, refine=20))
    same(pm.most_similar(q, 3, 5, refine=20, screen=True), pm.most_similar(q, 3, 5, refine=20))
    pm16 = qmatrix.PartitionedMatrix(qmatrix.QuantizedMatrix(make_pq(ra, 7, 16), np.zeros((8, 7), np.uint8)), np.zeros((2, 28), np.float32), np.zeros(8, np.int64))
    with pytest.raises(ra.PanicError, match="unpack4"):
        pm16.pack4().nearest(np.zeros(28, np.float32), 1, 1, screen=True)
