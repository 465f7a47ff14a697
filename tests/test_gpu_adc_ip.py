"""ADC similarity search on the GPU (include/pqhip.h: pqhip_adc_ip_tables_f32_dev, pqhip_adc_ip_search_f32_dev): the
inner-product tables bit for bit against the reference (tests/adc_ip_ref.py, pinned to the oracle by test_adc_ip.py),
the k rows of largest score fl(scan * scale) -- indices exactly, scores bit for bit (zero as +0, NaN as the canonical
NaN), padding -1 / -Inf, nothing written outside the outputs -- and QuantizedMatrix.most_similar / inner_products."""
import ctypes
import io

import numpy as np
import pytest

import synth
from adc_ip_ref import assert_same, ip_tables, ref_ip_search, scores
from oracle import pq_oracle as orc

SHAPES = [(15, 256, 20, False), (48, 256, 16, False), (10, 128, 2, False), (3, 7, 5, True)]


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


SENT_S = np.float32(-1234.5)
SENT_I = -777


def search_raw(pq, codes, tables, k, scales=None, pad=3):
    """The C entry point with row strides k + pad and sentinels around the outputs; checks the sentinels and returns
    (score, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n, M = codes.shape
    rs = k + pad
    sbuf = torch.full((nq * rs + 2 * pad,), float(SENT_S), dtype=torch.float32, device=codes.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream
    rc = _lib.lib().pqhip_adc_ip_search_f32_dev(pq._cb(), pq._slot_for(codes), tables.data_ptr(), nq, codes.data_ptr(),
                                               codes.element_size(), n,
                                               codes.stride(0) if n > 1 else max(codes.stride(0), M),
                                               scales.data_ptr() if scales is not None else None, k,
                                               sbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs,
                                               ctypes.c_void_p(stream))
    assert rc == _lib.OK, rc
    sb, ib = sbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(sb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (sb[~body] == SENT_S).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    s = np.stack([sb[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    i = np.stack([ib[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    return s, i


def check_all(pq, cd, t, score, ks, scales=None):
    """Every k of ks: the Python entry point and the raw one (sentinels) against the reference selection of `score`."""
    for k in ks:
        want_s, want_i = ref_ip_search(score, k)
        s, i = pq.adc_ip_search_device(cd, t, k, scales=scales, check=True)
        if t.dim() == 2:
            assert tuple(s.shape) == (k,) and tuple(i.shape) == (k,)
            s, i = s[None], i[None]
        assert str(s.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
        assert_same(s.cpu().numpy(), i.cpu().numpy(), want_s, want_i)
        rs_, ri = search_raw(pq, cd, t, k, scales=scales)
        assert_same(rs_, ri, want_s, want_i)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", SHAPES + [(15, 1024, 4, False), (8, 1024, 6, True)])
def test_gpu_ip_tables_match_reference(ra, M, K, dsub, opq):
    import torch
    d = M * dsub
    q = synth.normalish(9710 + d + K, (M, K, dsub))
    P = synth.orthonormal(9711 + d, d) if opq else None
    pq = ra.Pq(P, q)
    ys = synth.normalish(9712 + d, (5, d))
    want = ip_tables(q, ys, projection=P)
    ra.launch_log(reset=True)
    t = pq.adc_ip_tables_device(torch.from_numpy(ys).cuda())
    torch.cuda.synchronize()
    log = ra.launch_log(reset=True)
    assert "k_adc_ip_tables" in log and ("k_adc_rotate_queries" in log) == opq, log
    assert tuple(t.shape) == (5, M, K) and t.cpu().numpy().tobytes() == want.tobytes()
    t1 = pq.adc_ip_tables_device(torch.from_numpy(ys[3]).cuda())
    assert tuple(t1.shape) == (M, K) and t1.cpu().numpy().tobytes() == want[3].tobytes()
    # the distance tables are unchanged and are fl(fl(yy + cc) - fl(ip + ip)) of these
    assert pq.adc_tables_device(torch.from_numpy(ys).cuda()).cpu().numpy().tobytes() == \
        orc.adc_tables(q, ys, projection=P).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n,nq,wide", [(1, 4, False), (64, 1, False), (5003, 13, False), (5003, 8, False),
                                       (200003, 8, False), (200003, 1, False), (200003, 4, False),
                                       (1, 4, True), (64, 1, True), (5003, 13, True), (200003, 8, True)])
def test_gpu_ip_search_matches_reference(ra, n, nq, wide):
    import torch
    M, K, dsub = 15, 256, 20
    q = synth.normalish(9720, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9721 + nq, (nq, M * dsub))
    t = pq.adc_ip_tables_device(torch.from_numpy(ys).cuda())
    tt = t.cpu().numpy()
    assert tt.tobytes() == ip_tables(q, ys).tobytes()
    codes = synth.codes_u8(9722 + n, (n, M), K)
    cd = torch.from_numpy(codes.astype(np.int32) if wide else codes).cuda()
    sc = (synth.uniform01(9723 + n, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)   # some negative
    scd = torch.from_numpy(sc).cuda()
    scan = orc.adc_scan(tt, codes)
    ks = (1, 10, 100, 1024)
    check_all(pq, cd, t, scores(scan), ks)
    check_all(pq, cd, t, scores(scan, sc), ks, scales=scd)
    if nq == 13:
        check_all(pq, cd, t[5].contiguous(), scores(scan[5], sc), (1, 100), scales=scd)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", [(48, 256, 16, False), (10, 128, 2, False), (3, 7, 5, True)])
def test_gpu_ip_search_other_shapes(ra, M, K, dsub, opq):
    import torch
    d = M * dsub
    q = synth.normalish(9730 + d + K, (M, K, dsub))
    P = synth.orthonormal(9731 + d, d) if opq else None
    pq = ra.Pq(P, q)
    ys = synth.normalish(9732 + d, (9, d))
    t = pq.adc_ip_tables_device(torch.from_numpy(ys).cuda())
    tt = t.cpu().numpy()
    assert tt.tobytes() == ip_tables(q, ys, projection=P).tobytes()
    codes = synth.codes_u8(9733 + d, (30011, M), K)
    cd = torch.from_numpy(codes).cuda()
    sc = synth.uniform01(9734, (30011,)) + np.float32(0.25)
    scan = orc.adc_scan(tt, codes)
    check_all(pq, cd, t, scores(scan), (1, 64, 1024))
    check_all(pq, cd, t, scores(scan, sc), (10, 256), scales=torch.from_numpy(sc).cuda())


@pytest.mark.gpu
def test_gpu_ip_search_non_finite_and_special_scales(ra):
    """Tables with planted NaN / +Inf / -Inf entries, and scales of 0, -0, negative, NaN and +-Inf: NaN after -Inf,
    zero scores as +0, 0 * Inf = NaN."""
    import torch
    M, K, dsub, n = 15, 256, 20, 50001
    q = synth.normalish(9740, (M, K, dsub))
    pq = ra.Pq(None, q)
    ys = synth.normalish(9741, (8, M * dsub))
    tt = pq.adc_ip_tables_device(torch.from_numpy(ys).cuda()).cpu().numpy().copy()
    rng = np.random.default_rng(9742)
    for qq in (3, 4, 5):
        for m in range(M):
            j = rng.integers(0, K, 12)
            tt[qq, m, j[:4]] = np.inf
            tt[qq, m, j[4:8]] = np.nan
            if qq == 5:
                tt[qq, m, j[8:]] = -np.inf
    tt[6] = np.round(tt[6])                              # many exact ties and exact zeros
    t2 = torch.from_numpy(tt).cuda()
    codes = synth.codes_u8(9743, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    scan = orc.adc_scan(tt, codes)
    assert np.isnan(scan).any() and np.isinf(scan).any()
    sc = (synth.uniform01(9744, (n,)) + np.float32(0.5)).astype(np.float32)
    pick = rng.integers(0, n, 3000)
    sc[pick[:500]] = 0.0
    sc[pick[500:1000]] = -0.0
    sc[pick[1000:1500]] = -sc[pick[1000:1500]]
    sc[pick[1500:1800]] = np.nan
    sc[pick[1800:2100]] = np.inf
    sc[pick[2100:2400]] = -np.inf
    check_all(pq, cd, t2, scores(scan), (1, 100, 1024))
    check_all(pq, cd, t2, scores(scan, sc), (1, 100, 1024), scales=torch.from_numpy(sc).cuda())
    # n < k on a NaN-heavy query: every row, then the padding
    check_all(pq, cd[:300], t2[4].contiguous(), scores(scan[4, :300], sc[:300]), (1024,),
              scales=torch.from_numpy(sc[:300]).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 8])
def test_gpu_ip_search_ties_at_kth_across_workgroups(ra, nq):
    """A handful of distinct rows repeated over the whole matrix: thousands of rows tie on the k-th score in every
    workgroup; the lowest indices must win, with and without (tied) scales."""
    import torch
    M, K, dsub, n = 15, 256, 20, 300001
    pq = ra.Pq(None, synth.normalish(9750, (M, K, dsub)))
    t = pq.adc_ip_tables_device(torch.from_numpy(synth.normalish(9751, (nq, M * dsub))).cuda())
    tt = t.cpu().numpy()
    for n_distinct in (2, 4):
        base = synth.codes_u8(9752 + n_distinct, (n_distinct, M), K)
        pick = np.random.default_rng(9753).integers(0, n_distinct, n)
        codes = np.ascontiguousarray(base[pick])
        cd = torch.from_numpy(codes).cuda()
        scan = orc.adc_scan(tt, codes)
        check_all(pq, cd, t, scores(scan), (7, 100, 1024))
        sc = np.where(pick % 2 == 0, np.float32(2.0), np.float32(0.5)).astype(np.float32)
        check_all(pq, cd, t, scores(scan, sc), (7, 1024), scales=torch.from_numpy(sc).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 4, 8, 13])
def test_gpu_ip_search_is_l2_search_of_negated_tables(ra, nq):
    """Without scales, ip_search(T) selects what adc_search_device(-T) selects, with score == -dist up to the sign of
    zero: sum_m (-T) = -(sum_m T) exactly under round-to-nearest."""
    import torch
    M, K, dsub, n = 15, 256, 20, 120011
    pq = ra.Pq(None, synth.normalish(9760, (M, K, dsub)))
    t = pq.adc_ip_tables_device(torch.from_numpy(synth.normalish(9761 + nq, (nq, M * dsub))).cuda())
    cd = torch.from_numpy(synth.codes_u8(9762, (n, M), K)).cuda()
    for k in (1, 10, 100, 1024):
        s, i = pq.adc_ip_search_device(cd, t, k)
        d, j = pq.adc_search_device(cd, (-t).contiguous(), k)
        assert torch.equal(i, j)
        assert torch.equal(s, -d)            # == compares -0 and +0 equal


@pytest.mark.gpu
def test_gpu_ip_search_status_codes_and_edges(ra):
    import torch
    from reductive_amd import _lib
    M, K = 15, 256
    pq = ra.Pq(None, synth.normalish(9770, (M, K, 4)))
    t = pq.adc_ip_tables_device(torch.from_numpy(synth.normalish(9771, (2, M * 4))).cuda())
    cd = torch.from_numpy(synth.codes_u8(9772, (100, M), K)).cuda()
    for k, want in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        with pytest.raises(_lib.PqHipError) as e:
            pq.adc_ip_search_device(cd, t, k)
        assert e.value.status == want
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_s = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")

    def call(nq=1, cb=1, n=100, c_rs=M, k=10, s_rs=10, i_rs=10, scales=None):
        return L.pqhip_adc_ip_search_f32_dev(pq._cb(), 0, t.data_ptr(), nq, cd.data_ptr(), cb, n, c_rs, scales, k,
                                             out_s.data_ptr(), s_rs, out_i.data_ptr(), i_rs, ctypes.c_void_p(s))
    assert call(cb=2) == _lib.EUNSUPPORTED
    assert call(cb=2, k=0) == _lib.EINVAL                          # EINVAL before EUNSUPPORTED
    assert call(s_rs=9) == _lib.ESHAPE
    assert call(i_rs=9) == _lib.ESHAPE
    assert call(c_rs=M - 1) == _lib.ESHAPE
    assert call(k=1025, s_rs=9) == _lib.EUNSUPPORTED               # EUNSUPPORTED before ESHAPE
    assert L.pqhip_adc_ip_search_f32_dev(pq._cb(), 7, t.data_ptr(), 1, cd.data_ptr(), 1, 100, M, None, 10,
                                         out_s.data_ptr(), 10, out_i.data_ptr(), 10, ctypes.c_void_p(s)) == _lib.ENODEV
    assert L.pqhip_adc_ip_tables_f32_dev(pq._cb(), 0, t.data_ptr(), 1, M * 4 - 1, out_s.data_ptr(),
                                         ctypes.c_void_p(s)) == _lib.ESHAPE
    # n_queries == 0 launches nothing
    torch.cuda.synchronize()
    ra.launch_log(reset=True)
    assert call(nq=0) == _lib.OK
    assert L.pqhip_adc_ip_tables_f32_dev(pq._cb(), 0, t.data_ptr(), 0, M * 4, out_s.data_ptr(),
                                         ctypes.c_void_p(s)) == _lib.OK
    assert ra.launch_log(reset=True) == ""
    # n == 0: the padding only (-1 / -Inf)
    sc, i = pq.adc_ip_search_device(cd[:0], t, 5)
    assert (i.cpu().numpy() == -1).all() and np.isneginf(sc.cpu().numpy()).all()
    # a code >= K raises the range error with check=True, on the u8 and the 32-bit paths
    bad = cd.clone()
    bad[77, 3] = 255
    pq_small = ra.Pq(None, synth.normalish(9773, (M, 200, 4)))
    ts = pq_small.adc_ip_tables_device(torch.from_numpy(synth.normalish(9774, (8, M * 4))).cuda())
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq_small.adc_ip_search_device(bad, ts, 10, check=True)
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq_small.adc_ip_search_device(bad.to(torch.int32), ts[0].contiguous(), 10, check=True)
    pq_small.adc_ip_search_device(bad % 200, ts, 10, check=True)   # flag consumed


@pytest.mark.gpu
def test_gpu_ip_search_generic_kernels(ra):
    """32-bit codes at K = 1,024 (table in LDS) and K = 4,096 (through L2), with scales."""
    import torch
    M = 15
    for K32, n in ((1024, 30011), (4096, 20011)):
        q32 = synth.normalish(9780 + K32, (M, K32, 4))
        p32 = ra.Pq(None, q32)
        t32 = p32.adc_ip_tables_device(torch.from_numpy(synth.normalish(9781, (5, M * 4))).cuda())
        c32 = synth.codes_u8(9782, (n, M), 256).astype(np.int32) * (K32 // 256) + (np.arange(n)[:, None] % (K32 // 256))
        c32 = np.ascontiguousarray(c32.astype(np.int32))
        cd32 = torch.from_numpy(c32).cuda()
        scan = orc.adc_scan(t32.cpu().numpy(), c32)
        sc = synth.uniform01(9783, (n,)) - np.float32(0.3)
        ra.launch_log(reset=True)
        check_all(p32, cd32, t32, scores(scan, sc), (1, 64, 1024), scales=torch.from_numpy(sc).cuda())
        log = ra.launch_log(reset=True)
        assert ("k_adc_ip_search_wide" if K32 == 1024 else "k_adc_ip_search_any") in log, log
        assert "k_adc_search" not in log, log


@pytest.mark.gpu
def test_gpu_ip_search_indices_past_2_31(ra):
    """M = 1, K = 256, n = 2^31 + 4096 rows of one low-scoring code, with high-scoring codes planted past row 2^31: the
    answer is known in closed form (no CPU scan)."""
    import torch
    M, K, n = 1, 256, (1 << 31) + 4096
    pq = ra.Pq(None, synth.normalish(9790, (M, K, 2)))
    codes = torch.full((n, 1), 255, dtype=torch.uint8, device="cuda")
    planted = [(1 << 31) + 4095 - 37 * j for j in range(10)]     # row of code j
    for j, r in enumerate(planted):
        codes[r, 0] = j
    codes[(1 << 31) - 1, 0] = 3                                    # one more code 3, at a smaller index than planted[3]
    tab = -torch.arange(K, dtype=torch.float32, device="cuda").reshape(1, 1, K).repeat(2, 1, 1).contiguous()
    want_i = [planted[0], planted[1], planted[2], (1 << 31) - 1, planted[3]] + planted[4:] + [0, 1, 2, 3, 4]
    want_s = [0, -1, -2, -3, -3, -4, -5, -6, -7, -8, -9, -255, -255, -255, -255, -255]
    s, i = pq.adc_ip_search_device(codes, tab, 16, check=True)
    assert i.cpu().numpy().tolist() == [want_i, want_i]
    assert s.cpu().numpy().tolist() == [want_s, want_s]
    assert not np.signbit(s.cpu().numpy()[:, 0]).any()            # the zero score of code 0 comes back as +0
    del codes
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_ip_search_launch_log(ra):
    """The 8-query headline shape runs the fused multi-query similarity kernel plus its merge, no scan kernel and no
    distance-search kernel; one query at k = 1024 runs the single-query form."""
    import torch
    M, K, dsub, n = 15, 256, 20, 100000
    pq = ra.Pq(None, synth.normalish(9800, (M, K, dsub)))
    t = pq.adc_ip_tables_device(torch.from_numpy(synth.normalish(9801, (8, M * dsub))).cuda())
    cd = torch.from_numpy(synth.codes_u8(9802, (n, M), K)).cuda()
    sc = torch.from_numpy(synth.uniform01(9803, (n,))).cuda()
    torch.cuda.synchronize()
    for k in (10, 100):
        for scales in (None, sc):
            ra.launch_log(reset=True)
            pq.adc_ip_search_device(cd, t, k, scales=scales)
            log = ra.launch_log(reset=True)
            assert "k_adc_ip_search_u8_mq<8 queries>" in log and "k_adc_ip_search_merge" in log, log
            assert "k_adc_scan" not in log and "k_adc_search" not in log, log
    ra.launch_log(reset=True)
    pq.adc_ip_search_device(cd, t[:1], 1024)
    log = ra.launch_log(reset=True)
    assert "k_adc_ip_search_u8 " in log + " " and "mq" not in log, log
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("opq", [False, True])
def test_gpu_qmatrix_most_similar_and_inner_products(ra, opq):
    """A loaded chunk with norms: most_similar ranks rows by the scan over the IP tables times the norms (use_norms)
    or by the scan alone; inner_products is that scan (times the norms); a chunk without norms ranks by the scan."""
    import torch
    from reductive_amd import qmatrix
    M, K, dsub, N = 15, 256, 8, 40009
    d = M * dsub
    q = synth.normalish(9810, (M, K, dsub))
    P = synth.orthonormal(9811, d) if opq else None
    codes = synth.codes_u8(9812, (N, M), K)
    norms = synth.uniform01(9813, (N,)) + np.float32(0.5)
    ys = synth.normalish(9814, (3, d))
    scan = orc.adc_scan(ip_tables(q, ys, projection=P), codes)
    for with_norms in (True, False):
        qm = qmatrix.QuantizedMatrix.load(io.BytesIO(qmatrix.dumps(ra.Pq(P, q), codes, norms if with_norms else None)))
        yd = torch.from_numpy(ys).cuda()
        for use_norms in (True, False):
            scaled = with_norms and use_norms
            want = scores(scan, norms) if scaled else scan
            got = qm.inner_products(yd, use_norms=use_norms).cpu().numpy()
            assert got.tobytes() == want.tobytes()
            assert qm.inner_products(yd[1], use_norms=use_norms).cpu().numpy().tobytes() == want[1].tobytes()
            for k in (1, 10, 500):
                want_s, want_i = ref_ip_search(want, k)
                s, i = qm.most_similar(yd, k, use_norms=use_norms)
                assert_same(s.cpu().numpy(), i.cpu().numpy(), want_s, want_i)
                s1, i1 = qm.most_similar(yd[2], k, use_norms=use_norms)
                assert_same(s1.cpu().numpy()[None], i1.cpu().numpy()[None], want_s[2:3], want_i[2:3])
        # the ranking is by the inner product with what embeddings() returns
        s, i = qm.most_similar(yd[0], 5)
        emb = qm.embeddings(i).cpu().numpy().astype(np.float64)
        assert np.allclose(emb @ ys[0].astype(np.float64), s.cpu().numpy(), rtol=1e-4, atol=1e-4)
