"""ADC search (include/pqhip.h: pqhip_adc_search_f32_dev): the k nearest rows of every query under the first-minimum
order of cluster_assignments (kmeans.rs:133-159, oracle of_less) -- NaN above +Inf, -0 == +0, ties to the smaller row
index -- with the scan's own distances.  Reference: the oracle's tables and scan, then a stable selection in numpy.
CPU: the reference selection against the oracle's first_min.  GPU: HIP search vs reference, indices exactly, distances
bit for bit (NaN as NaN), padding past the last row, nothing written outside the outputs."""
import ctypes

import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc


# ---- reference selection --------------------------------------------------------------------------------
def ref_search(dist, k):
    """dist [n] or [nq, n] f32 -> (d, i) [nq, k]: rows ordered by (key(dist), index); index -1 / +Inf past the end."""
    d2 = np.atleast_2d(np.asarray(dist, np.float32))
    nq, n = d2.shape
    out_d = np.full((nq, k), np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    rows = np.arange(n)
    for q in range(nq):
        v = d2[q].astype(np.float64)
        nan = np.isnan(v)
        val = np.where(nan, 0.0, v) + 0.0             # -0 -> +0; NaN rows ordered by the flag below
        order = np.lexsort((rows, val, nan))           # last key is primary: NaN flag, value, row index
        top = order[:min(k, n)]
        out_i[q, :top.size] = top
        out_d[q, :top.size] = d2[q, top]
    return out_d, out_i


def test_reference_top1_is_first_min():
    rng = np.random.default_rng(9900)
    for trial in range(200):
        n = int(rng.integers(1, 300))
        v = rng.integers(-3, 4, n).astype(np.float32)          # many ties
        for special in (np.nan, np.inf, -np.inf, -0.0):
            sel = rng.random(n) < 0.1
            v[sel] = special
        d, i = ref_search(v, 5)
        assert i[0, 0] == orc.first_min(v)
        # the whole prefix is the repeated first-minimum of what is left
        rest = v.copy()
        live = np.ones(n, bool)
        for j in range(min(5, n)):
            cand = np.where(live)[0]
            best = cand[orc.first_min(rest[cand])]
            assert i[0, j] == best
            live[best] = False
        assert (i[0, min(5, n):] == -1).all() and np.isposinf(d[0, min(5, n):]).all()


def test_reference_nan_above_inf_and_signed_zero():
    v = np.array([np.nan, np.inf, 0.0, -0.0, 1.0, np.nan, -np.inf], np.float32)
    d, i = ref_search(v, 7)
    assert i[0].tolist() == [6, 2, 3, 4, 1, 0, 5]


# ---- GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


SENT_D = np.float32(-1234.5)
SENT_I = -777


def search_raw(ra, pq, codes, tables, k, pad=3):
    """The C entry point with row strides k + pad and sentinels around the outputs; checks the sentinels and returns
    (dist, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n, M = codes.shape
    rs = k + pad
    dbuf = torch.full((nq * rs + 2 * pad,), float(SENT_D), dtype=torch.float32, device=codes.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream
    rc = _lib.lib().pqhip_adc_search_f32_dev(pq._cb(), pq._slot_for(codes), tables.data_ptr(), nq, codes.data_ptr(),
                                            codes.element_size(), n, codes.stride(0) if n > 1 else max(codes.stride(0), M),
                                            k, dbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs,
                                            ctypes.c_void_p(stream))
    assert rc == _lib.OK, rc
    db, ib = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(db.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (db[~body] == SENT_D).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    d = np.stack([db[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    i = np.stack([ib[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    return d, i


def assert_same(got_d, got_i, want_d, want_i):
    assert np.array_equal(got_i, want_i)
    gn, wn = np.isnan(got_d), np.isnan(want_d)
    assert np.array_equal(gn, wn)
    assert got_d[~gn].tobytes() == want_d[~wn].tobytes()


def check_all(ra, pq, cd, t, dist, ks):
    """Every k of ks: the Python entry point and the raw one (sentinels) against the reference."""
    for k in ks:
        want_d, want_i = ref_search(dist, k)
        d, i = pq.adc_search_device(cd, t, k, check=True)
        if t.dim() == 2:
            assert tuple(d.shape) == (k,) and tuple(i.shape) == (k,)
            d, i = d[None], i[None]
        assert d.dtype.is_floating_point and str(i.dtype) == "torch.int64"
        assert_same(d.cpu().numpy(), i.cpu().numpy(), want_d, want_i)
        rd, ri = search_raw(ra, pq, cd, t, k)
        assert_same(rd, ri, want_d, want_i)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", [(15, 256, 20, False), (48, 256, 16, False), (10, 128, 2, False), (3, 7, 5, True)])
@pytest.mark.parametrize("n,nq", [(1, 4), (64, 1), (100, 13), (1024, 8), (5003, 13), (200003, 8)])
def test_gpu_search_matches_reference(ra, M, K, dsub, opq, n, nq):
    import torch
    d = M * dsub
    q = synth.normalish(9910 + d + K, (M, K, dsub))
    P = synth.orthonormal(9911 + d, d) if opq else None
    pq = ra.Pq(P, q)
    ys = synth.normalish(9912 + d + nq, (nq, d))
    want_t = orc.adc_tables(q, ys, projection=P)
    t = pq.adc_tables_device(torch.from_numpy(ys).cuda())
    assert t.cpu().numpy().tobytes() == want_t.tobytes()
    codes = synth.codes_u8(9913 + d + n, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    dist = orc.adc_scan(want_t, codes)
    ks = (1, 7, 64, 100, 1024) if n <= 5003 else (1, 100, 1024)
    check_all(ra, pq, cd, t, dist, ks)
    if nq == 13:
        # a single query ([M, K] tables) gives [k] outputs
        check_all(ra, pq, cd, t[5].contiguous(), dist[5], (1, 64))
    # top-1 is the first minimum of the scan, by definition
    d1, i1 = pq.adc_search_device(cd, t, 1)
    scan = pq.adc_scan_device(cd, t).cpu().numpy()
    assert [orc.first_min(scan[j]) for j in range(nq)] == i1[:, 0].cpu().numpy().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 8])
def test_gpu_search_ties_at_kth_across_workgroups(ra, nq):
    """A handful of distinct rows repeated over the whole matrix: thousands of rows tie on the k-th distance in every
    workgroup; the lowest indices must win."""
    import torch
    M, K, dsub, n = 15, 256, 20, 300001
    q = synth.normalish(9920, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9921, (nq, M * dsub))
    t = pq.adc_tables_device(torch.from_numpy(ys).cuda())
    want_t = t.cpu().numpy()
    for n_distinct in (2, 4):
        base = synth.codes_u8(9922 + n_distinct, (n_distinct, M), K)
        pick = np.random.default_rng(9923).integers(0, n_distinct, n)
        codes = np.ascontiguousarray(base[pick])
        dist = orc.adc_scan(want_t, codes)
        check_all(ra, pq, torch.from_numpy(codes).cuda(), t, dist, (7, 100, 1024))


@pytest.mark.gpu
def test_gpu_search_descending_order(ra):
    """Rows sorted by descending distance of query 0: every row enters every wave's list (correctness only)."""
    import torch
    M, K, dsub, n = 15, 256, 20, 120000
    q = synth.normalish(9930, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9931, (8, M * dsub))
    t = pq.adc_tables_device(torch.from_numpy(ys).cuda())
    want_t = t.cpu().numpy()
    codes = synth.codes_u8(9932, (n, M), K)
    d0 = orc.adc_scan(want_t[0], codes)
    codes = np.ascontiguousarray(codes[np.argsort(-d0, kind="stable")])
    cd = torch.from_numpy(codes).cuda()
    check_all(ra, pq, cd, t, orc.adc_scan(want_t, codes), (10, 100, 1024))
    check_all(ra, pq, cd, t[0].contiguous(), orc.adc_scan(want_t[0], codes), (100, 1024))


@pytest.mark.gpu
def test_gpu_search_non_finite(ra):
    """Queries with a +Inf and a NaN component, and tables with planted +Inf / -Inf / NaN entries: Inf / NaN mixtures
    across rows; NaN ranks above +Inf."""
    import torch
    M, K, dsub, n = 15, 256, 20, 50001
    q = synth.normalish(9940, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9941, (8, M * dsub))
    ys[1, 7] = np.inf
    ys[2, 30] = np.nan
    t = pq.adc_tables_device(torch.from_numpy(ys).cuda())
    tt = t.cpu().numpy().copy()
    rng = np.random.default_rng(9942)
    for qq in (3, 4, 5):
        for m in range(M):
            j = rng.integers(0, K, 12)
            tt[qq, m, j[:4]] = np.inf
            tt[qq, m, j[4:8]] = np.nan
            if qq == 5:
                tt[qq, m, j[8:]] = -np.inf
    t2 = torch.from_numpy(tt).cuda()
    codes = synth.codes_u8(9943, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    dist = orc.adc_scan(tt, codes)
    assert np.isnan(dist).any() and np.isinf(dist).any()
    check_all(ra, pq, cd, t2, dist, (1, 100, 1024))
    # n < k on a NaN-only query: every row, then the padding
    check_all(ra, pq, cd[:300], t2[2].contiguous(), dist[2, :300], (1024,))


@pytest.mark.gpu
def test_gpu_search_layout_and_range(ra):
    """Unaligned first row and an odd row stride; 32-bit codes at K = 1,024 (table in LDS) and K = 4,096 (through L2);
    a code >= K raises the scan's PanicError with check=True."""
    import torch
    M, K, dsub = 15, 256, 20
    q = synth.normalish(9950, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9951, (13, M * dsub))
    t = pq.adc_tables_device(torch.from_numpy(ys).cuda())
    want_t = t.cpu().numpy()
    wide = synth.codes_u8(9952, (40003, M + 6), K)               # row stride 21
    wd = torch.from_numpy(wide).cuda()
    for r0, c0 in ((1, 3), (2, 5), (3, 0)):
        view = wd[r0:, c0:c0 + M]
        dist = orc.adc_scan(want_t, np.ascontiguousarray(wide[r0:, c0:c0 + M]))
        check_all(ra, pq, view, t, dist, (7, 100))
    for K32, n in ((1024, 30011), (4096, 20011)):
        q32 = synth.normalish(9953 + K32, (M, K32, 4))
        p32 = ra.Pq(None, q32)
        y32 = synth.normalish(9954, (5, M * 4))
        t32 = p32.adc_tables_device(torch.from_numpy(y32).cuda())
        c32 = synth.codes_u8(9955, (n, M), 256).astype(np.int32) * (K32 // 256) + (np.arange(n)[:, None] % (K32 // 256))
        c32 = np.ascontiguousarray(c32.astype(np.int32))
        cd32 = torch.from_numpy(c32).cuda()
        dist = orc.adc_scan(t32.cpu().numpy(), c32)
        ra.launch_log(reset=True)
        check_all(ra, p32, cd32, t32, dist, (1, 64, 1024))
        log = ra.launch_log(reset=True)
        assert ("k_adc_search_wide" if K32 == 1024 else "k_adc_search_any") in log, log
        bad = cd32.clone()
        bad[n - 1, M - 1] = K32
        with pytest.raises(ra.PanicError, match="index out of bounds"):
            p32.adc_search_device(bad, t32, 10, check=True)
    bad = torch.from_numpy(np.ascontiguousarray(wide[:, :M])).cuda()
    pq_small = ra.Pq(None, synth.normalish(9956, (M, 100, 4)))
    t_small = pq_small.adc_tables_device(torch.from_numpy(synth.normalish(9957, (8, M * 4))).cuda())
    bad = bad % 100
    bad[12345, 3] = 100
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq_small.adc_search_device(bad, t_small, 10, check=True)
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq_small.adc_scan_device(bad, t_small, check=True)


@pytest.mark.gpu
def test_gpu_search_status_codes(ra):
    import torch
    from reductive_amd import _lib
    M, K = 15, 256
    pq = ra.Pq(None, synth.normalish(9960, (M, K, 4)))
    t = pq.adc_tables_device(torch.from_numpy(synth.normalish(9961, (2, M * 4))).cuda())
    cd = torch.from_numpy(synth.codes_u8(9962, (100, M), K)).cuda()
    for k, want in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(_lib.PqHipError) as e:
            pq.adc_search_device(cd, t, k)
        assert e.value.status == want
    # n == 0: the padding only
    d, i = pq.adc_search_device(cd[:0], t, 5)
    assert (i.cpu().numpy() == -1).all() and np.isposinf(d.cpu().numpy()).all()
    # stride checks
    L = _lib.lib()
    out_d = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rc = L.pqhip_adc_search_f32_dev(pq._cb(), 0, t.data_ptr(), 1, cd.data_ptr(), 1, 100, M, 10, out_d.data_ptr(), 9,
                                    out_i.data_ptr(), 10, ctypes.c_void_p(s))
    assert rc == _lib.ESHAPE
    rc = L.pqhip_adc_search_f32_dev(pq._cb(), 0, t.data_ptr(), 1, cd.data_ptr(), 1, 100, M - 1, 10, out_d.data_ptr(), 10,
                                    out_i.data_ptr(), 10, ctypes.c_void_p(s))
    assert rc == _lib.ESHAPE
    rc = L.pqhip_adc_search_f32_dev(pq._cb(), 0, t.data_ptr(), 1, cd.data_ptr(), 2, 100, M, 10, out_d.data_ptr(), 10,
                                    out_i.data_ptr(), 10, ctypes.c_void_p(s))
    assert rc == _lib.EUNSUPPORTED


@pytest.mark.gpu
def test_gpu_search_indices_past_2_31(ra):
    """M = 1, K = 256, n = 2^31 + 4096 rows of one far code, with near codes planted past row 2^31: the answer is known
    in closed form (no CPU scan)."""
    import torch
    M, K, n = 1, 256, (1 << 31) + 4096
    pq = ra.Pq(None, synth.normalish(9970, (M, K, 2)))
    codes = torch.full((n, 1), 255, dtype=torch.uint8, device="cuda")
    planted = [(1 << 31) + 4095 - 37 * j for j in range(10)]     # row of code j
    for j, r in enumerate(planted):
        codes[r, 0] = j
    codes[(1 << 31) - 1, 0] = 3                                    # one more code 3, at a smaller index than planted[3]
    tab = torch.arange(K, dtype=torch.float32, device="cuda").reshape(1, 1, K).repeat(2, 1, 1).contiguous()
    want_i = [planted[0], planted[1], planted[2], (1 << 31) - 1, planted[3]] + planted[4:] + [0, 1, 2, 3, 4]
    want_d = [0, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9, 255, 255, 255, 255, 255]
    d, i = pq.adc_search_device(codes, tab, 16, check=True)
    assert i.cpu().numpy().tolist() == [want_i, want_i]
    assert d.cpu().numpy().tolist() == [want_d, want_d]
    del codes
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_search_launch_log(ra):
    """The 8-query headline shape runs the fused multi-query kernel plus the merge and no scan kernel; the scan keeps
    its names."""
    import torch
    M, K, dsub, n = 15, 256, 20, 100000
    pq = ra.Pq(None, synth.normalish(9980, (M, K, dsub)))
    t = pq.adc_tables_device(torch.from_numpy(synth.normalish(9981, (8, M * dsub))).cuda())
    cd = torch.from_numpy(synth.codes_u8(9982, (n, M), K)).cuda()
    torch.cuda.synchronize()
    for k in (10, 100):
        ra.launch_log(reset=True)
        pq.adc_search_device(cd, t, k)
        log = ra.launch_log(reset=True)
        assert "k_adc_search_u8_mq<8 queries>" in log and "k_adc_search_merge" in log, log
        assert "k_adc_scan" not in log, log
    ra.launch_log(reset=True)
    pq.adc_search_device(cd, t[:1], 1024)
    log = ra.launch_log(reset=True)
    assert "k_adc_search_u8 " in log + " " and "mq" not in log, log
    pq.adc_scan_device(cd, t)
    log = ra.launch_log(reset=True)
    assert "k_adc_scan_u8_mq<8 queries>" in log and "search" not in log, log
    torch.cuda.synchronize()
