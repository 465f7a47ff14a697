"""GPU tests of the 16-bit table screen over resident codes (include/pqhip.h: pqhip_adc_screen16_f32_dev) through
Pq.adc_screen_device(image_bits=16), of the batch search on it (Pq.adc_search_batch_device(image_bits=16)) and of
screen="u16" on QuantizedMatrix.  The screen equals the numpy model of tests/adc_screen16_ref.py id for id, contains what
the device's own range calls return and stays within the stated slack; one result for every grid, split and capacity;
the batch search equals the plain calls bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

import adc_screen16_ref as a16
import synth
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
N = 4099            # 65 hit words, the last of 3 rows; 5 workgroups' worth of 1,024 rows
NQ = 37             # 16 slots: 16 + 16 + 8; 8 slots: 4 x 8 + 8; 4 slots: 9 x 4 + 4
# L = 65,535; 16, 8 and 4 slots per pass; one code dword and the widest row fetch; M L = 65,500
SHAPES = [(1, 256), (15, 256), (20, 256), (48, 256), (7, 16), (100, 16)]
FORMS = [(False, False), (True, False), (True, True)]


@functools.lru_cache(maxsize=None)
def world(M, K, ip, seed=7100):
    """skewed codes in rows M + 1 bytes apart (an unaligned row stride), tables with a few small entries per subquantizer,
    scales and a mask; per form the thresholds at the 20th best value of each query; host copies beside the device tensors"""
    import torch
    rng = np.random.default_rng(seed + M)
    codes = np.where(rng.random((N, M)) < 0.5, rng.integers(0, min(K, 4), (N, M)), rng.integers(0, K, (N, M))).astype(np.uint8)
    t = (rng.random((NQ, M, K)) + 0.5).astype(np.float32)
    t[:, :, : min(K, 4)] *= np.float32(0.1)
    if ip:
        t = -t
    scales = (rng.random(N) + 0.5).astype(np.float32)
    allow = rng.random(N) < 0.7
    c64 = codes.astype(np.int64)
    thr = {sc: np.stack([np.sort(a16.values(tq, c64, ip, scales if sc else None))[-20 if ip else 19] for tq in t]) for sc in (False, True)}
    buf = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")
    buf[:, :M] = torch.from_numpy(codes).cuda()
    return dict(codes=c64, t=t, scales=scales, allow=allow, thr=thr, cd=buf[:, :M], td=torch.from_numpy(t).cuda(),
                sd=torch.from_numpy(scales).cuda(), wd=dev_words(allow))


def model(w, thr, ip, scaled, allow=None, t=None):
    """(lims, idx, parameters per query) of the numpy model"""
    t = w["t"] if t is None else t
    res = [a16.screen16(tq, w["codes"], th, ip, w["scales"] if scaled else None) for tq, th in zip(t, thr)]
    ids = [np.flatnonzero(r[0] if allow is None else r[0] & allow) for r in res]
    return np.concatenate([[0], np.cumsum([i.size for i in ids])]).astype(np.int64), np.concatenate(ids), [r[1] for r in res]


def equals(got, want):
    lims, idx = (a.cpu().numpy() for a in got)
    assert np.array_equal(lims, want[0]) and np.array_equal(idx, want[1])


@pytest.mark.parametrize("ip,scaled", FORMS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_gpu_adc_screen16_equals_the_model_and_contains_the_range_call(ra, M, K, ip, scaled):
    pq, w = make_pq(ra, M, K), world(M, K, ip)
    thr, kw = w["thr"][scaled], dict(ip=ip, scales=w["sd"] if scaled else None, image_bits=16)
    want = model(w, thr, ip, scaled)
    for nq in (NQ, 17, 1):
        got = pq.adc_screen_device(w["cd"], w["td"][:nq], thr[:nq], check=True, **kw)
        equals(got, (want[0][: nq + 1], want[1][: want[0][nq]]))
    lims, idx = (a.cpu().numpy() for a in got)
    rng_call = pq.adc_ip_range_device if ip else pq.adc_range_device
    rl, _, ri = (a.cpu().numpy() for a in rng_call(w["cd"], w["td"], thr, **({"scales": w["sd"]} if scaled else {})))
    assert (np.diff(rl) >= 20).all()
    for q in range(NQ):
        mine, p = want[1][want[0][q]:want[0][q + 1]], want[2][q]
        assert np.isin(ri[rl[q]:rl[q + 1]], mine).all(), q                 # a superset of the device's range call
        ch = a16.chain(w["t"][q], w["codes"][mine]).astype(np.float64)
        if not scaled:
            assert ((thr[q] - ch if ip else ch - thr[q]) <= a16.slack16(p, M) * (1 + 1e-9)).all(), q
        else:
            c = w["scales"].astype(np.float64)[mine]
            assert (float(thr[q]) - ch * c <= a16.slack16(p, M, ch, c) * (1 + 1e-9)).all(), q


def test_gpu_adc_screen16_is_no_less_selective_than_the_u8_screen_at_48_subquantizers(ra):
    """A condition on this data, not a theorem (a coarser image may round a row in either direction).  The seed was picked
    with the two numpy models on the CPU: they return 1,911 (u8) and 894 (16-bit) rows for these 37 queries,
    740 of which meet their thresholds."""
    M, K = 48, 256
    pq, w = make_pq(ra, M, K), world(M, K, False)
    totals = [int(pq.adc_screen_device(w["cd"], w["td"], w["thr"][False], image_bits=b)[0][-1]) for b in (8, 16)]
    print("candidates u8 / u16:", totals)
    assert 20 * NQ <= totals[1] <= totals[0]


def test_gpu_adc_screen16_saturated_rows_sum_to_M_L_and_are_excluded(ra):
    import torch
    M, K = 100, 16
    pq, w = make_pq(ra, M, K), world(M, K, False)
    t = np.full((1, M, K), np.float32(1e6))
    t[:, :, 0] = np.float32(0.25)                    # every non-minimal entry saturates: U is L times their number
    cd = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")[:, :M]
    cd.copy_(w["cd"])
    cd[7], cd[8] = 0, K - 1                          # the all-minimum row; a row of U = M L = 65,500
    codes = cd.cpu().numpy().astype(np.int64)
    thr = np.array([0.25 * M + 1.0], np.float32)
    keep, p, U = a16.screen16(t[0], codes, thr[0])
    assert U[8] == 65500 and p["ulim"] == 654 and keep[7] and not keep[8]
    lims, idx = pq.adc_screen_device(cd, torch.from_numpy(t).cuda(), thr, image_bits=16, check=True)
    assert idx.cpu().numpy().tolist() == np.flatnonzero(keep).tolist() == np.flatnonzero((codes == 0).all(1)).tolist()


@pytest.mark.parametrize("ip,scaled", FORMS)
@pytest.mark.parametrize("M,K", [(100, 16), (48, 256)])
def test_gpu_adc_screen16_one_result_for_every_call_form(ra, M, K, ip, scaled):
    import torch
    from reductive_amd import _lib
    pq, w = make_pq(ra, M, K), world(M, K, ip)
    thr, sd = w["thr"][scaled], w["sd"] if scaled else None
    poisoned = torch.zeros((N, M + 1), dtype=torch.uint8, device="cuda")[:, :M]    # the unaligned row stride again
    poisoned.copy_(w["cd"])
    # codes >= K in every disallowed row; a byte cannot exceed K = 256, there the rows become the best ones instead
    poisoned[torch.from_numpy(~w["allow"]).cuda()] = 255 if K < 256 else 0
    call = lambda s=slice(None), cd=poisoned: pq.adc_screen_device(cd, w["td"][s], thr[s], ip=ip, scales=sd, allow=w["wd"],
                                                                  image_bits=16, check=True)    # check: the range flag is clear
    want = call()
    equals(want, model(w, thr, ip, scaled, w["allow"]))
    try:
        for wgs in (1, 3):
            ra.set_option("adc_screen_wgs", wgs)
            same(call(), want)
    finally:
        ra.set_option("adc_screen_wgs", 0)
    a, b = call(slice(0, 21)), call(slice(21, NQ))                          # the queries split over two calls
    same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), want)
    lims, idx = want
    total = int(lims[-1])
    l0, i0, t0, _ = pq._adc_screen(poisoned, w["td"], thr, ip, sd, w["wd"], 0, None, False, a16.NAME)
    assert t0 == total and torch.equal(l0, lims) and i0.numel() == 0        # capacity 0 counts
    out = torch.full((total // 2 + 8,), -7, dtype=torch.int64, device="cuda")   # sentinels behind a short capacity stay
    td, ld = torch.from_numpy(thr).cuda(), torch.empty_like(lims)
    rc = getattr(_lib.lib(), a16.NAME)(pq._cb(), pq._slot_for(poisoned), w["td"].data_ptr(), NQ, poisoned.data_ptr(), 1, N, poisoned.stride(0),
                                       w["wd"].data_ptr(), int(ip), sd.data_ptr() if scaled else None, td.data_ptr(), ld.data_ptr(),
                                       out.data_ptr(), total // 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(ld, lims) and torch.equal(out[: total // 2], idx[: total // 2]) and bool((out[total // 2:] == -7).all())


@pytest.mark.parametrize("ip,scaled", FORMS)
def test_gpu_adc_screen16_keeps_all_where_the_proof_does_not_reach(ra, ip, scaled):
    import torch
    M, K = 7, 16
    pq, w = make_pq(ra, M, K), dict(world(M, K, ip))
    t = np.repeat(w["t"][:1], 8, axis=0)
    t[1, 2, 3], t[2, 0, 1], t[3, 6, 0] = np.nan, np.inf, -np.inf            # a NaN entry, infinite entries
    thr = np.full(8, w["thr"][scaled][0], np.float32)
    thr[4:7] = [np.nan, np.inf, -np.inf]
    sc = w["scales"].copy()
    sc[::5] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, 1e-30, 3e38], np.float32), sc[::5].size)
    w["scales"] = sc
    got = pq.adc_screen_device(w["cd"], torch.from_numpy(t).cuda(), thr, ip=ip, scales=torch.from_numpy(sc).cuda() if scaled else None,
                               image_bits=16, check=True)
    want = model(w, thr, ip, scaled, t=t)
    equals(got, want)
    counts = np.diff(want[0])
    assert (counts[1:5] == N).all() and counts[0] < N // 4                   # special entries and a NaN threshold keep every row
    if not scaled:
        assert counts[5:7].tolist() == ([0, N] if ip else [N, 0])


@pytest.mark.parametrize("ip,scaled", FORMS)
def test_gpu_adc_search_batch_with_the_16_bit_image_equals_the_plain_search(ra, ip, scaled):
    import torch
    M, K = 48, 256
    pq, w = make_pq(ra, M, K), world(M, K, ip)
    kw = {"scales": w["sd"] if scaled else None} if ip else {}
    plain = pq.adc_ip_search_device if ip else pq.adc_search_device
    ties = (w["cd"] % 3).contiguous()                                         # codes drawn from three values: ties everywhere
    for cd, k, wd in ((w["cd"], 1, None), (w["cd"], 10, w["wd"]), (w["cd"], 300, None), (ties, 10, None), (ties, 300, w["wd"])):
        stats = {}
        got = pq.adc_search_batch_device(cd, w["td"], k, ip=ip, allow=wd, stats=stats, check=True, image_bits=16, **kw)
        same(got, plain(cd, w["td"], k, allow=wd, **kw))
        assert scaled or cd is ties or stats["fallback_queries"] == (0 if k <= 10 else NQ), stats   # as the model on the CPU: 0.5 %, 2.4 % and 8.5 % pass
    wide = make_pq(ra, 100, 256)                                              # four 16-bit images do not fit: the plain call
    cd = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (N, 100)).astype(np.uint8)).cuda()
    td = torch.from_numpy(synth.normalish(71, (9, 100, 256))).cuda()
    with pytest.raises(ra.PqHipError, match="unsupported"):
        wide.adc_screen_device(cd, td, 0.0, ip=ip, image_bits=16)
    stats = {}
    same(wide.adc_search_batch_device(cd, td, 4, ip=ip, image_bits=16, stats=stats, **kw), (wide.adc_ip_search_device if ip else wide.adc_search_device)(cd, td, 4, **kw))
    assert stats["fallback_queries"] == 9


def test_gpu_u16_screen_route_of_the_quantized_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    M, K = 15, 256
    pq, w = make_pq(ra, M, K), world(M, K, False)
    x = synth.normalish(72, (N, 4 * M))
    qm = qmatrix.QuantizedMatrix(pq, w["codes"].astype(np.uint8), norms=w["scales"]).attach_vectors(x)
    q = torch.from_numpy(x[:40] * np.float32(1.01)).cuda()
    seen = []
    real = pq.adc_search_batch_device
    pq.adc_search_batch_device = lambda *a, **k: (seen.append(k["image_bits"]), real(*a, **k))[1]
    try:
        for allow in (None, w["allow"]):
            same(qm.nearest(q, 1, allow=allow, screen="u16"), qm.nearest(q, 1, allow=allow))
            for use_norms in (True, False):
                same(qm.most_similar(q, 2, use_norms=use_norms, allow=allow, screen="u16"), qm.most_similar(q, 2, use_norms=use_norms, allow=allow))
        same(qm.nearest(q, 3, refine=20, screen="u16"), qm.nearest(q, 3, refine=20))
        same(qm.most_similar(q, 3, refine=20, screen="u16"), qm.most_similar(q, 3, refine=20))
        assert seen == [16] * 8
        qm.nearest(q, 1, screen=True)
        assert seen[-1] == 8
    finally:
        del pq.adc_search_batch_device
    with pytest.raises(ra.PanicError, match="unpack4"):
        qmatrix.QuantizedMatrix(make_pq(ra, 7, 16), np.zeros((8, 7), np.uint8)).pack4().nearest(np.zeros(28, np.float32), 1, screen="u16")
