"""GPU tests of the exact re-ranking (include/pqhip.h: pqhip_rerank_f32_dev) against tests/rerank_ref.py: indices exact,
values bit for bit, through Pq.rerank_device and through the raw C entry point with padded row strides and sentinels
around the outputs."""
import ctypes

import numpy as np
import pytest

import rerank_ref as rr
import synth
from test_gpu_adc_search_lists import SENT_I, SENT_V, ra  # noqa: F401

OPTION = "rerank_wgs_per_query"


def rerank_raw(pq, q, x, cand, k, ip, n_rows=None, pad=3):
    """The C entry point on 2-D tensors as they are strided, output row strides k + pad, sentinels around and between
    the output rows; checks the sentinels and returns (value, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq, d = q.shape
    n = x.shape[0] if n_rows is None else n_rows
    n_cand = cand.shape[1]
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=x.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = _lib.lib().pqhip_rerank_f32_dev(
        pq._cb(), pq._slot_for(x), q.data_ptr(), nq, q.stride(0) if nq > 1 else max(q.stride(0), d),
        x.data_ptr() if n > 0 else None, x.element_size(), n, d, x.stride(0) if n > 1 else max(x.stride(0), d),
        cand.data_ptr(), n_cand, cand.stride(0) if nq > 1 else max(cand.stride(0), n_cand), 1 if ip else 0, k,
        vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, ctypes.c_void_p(stream))
    assert rc == _lib.OK, rc
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for i in range(nq):
        body[pad + i * rs: pad + i * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    v = np.stack([vb[pad + i * rs: pad + i * rs + k] for i in range(nq)])
    i_ = np.stack([ib[pad + i * rs: pad + i * rs + k] for i in range(nq)])
    return v, i_


def make_pq(ra, seed=9900):
    """any quantizer: the call only borrows its device slot, scratch and flag"""
    return ra.Pq(None, synth.normalish(seed, (3, 7, 5)))


def make_data(seed, n, d, nq, half=False):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    return q, (x.astype(np.float16) if half else x)


def make_cand(seed, nq, n, n_cand, holes=True):
    """distinct rows per query (while n allows), some -1 padding inside and at the end"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.permutation(n)[:n_cand] if n_cand <= n else rng.integers(0, n, n_cand) for _ in range(nq)])
    c = c.astype(np.int64)
    if holes and n_cand > 2:
        c[rng.random(c.shape) < 0.1] = -1
        c[0, n_cand // 2:] = -1
    return c


def check_all(pq, q, x, cand, ks, single=False):
    """both metrics, every k: Pq.rerank_device and the raw call against the reference"""
    import torch
    qd, xd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(cand).cuda()
    for ip in (False, True):
        for k in ks:
            want_v, want_i, flag = rr.ref_rerank(q, x, cand, k, ip=ip)
            assert not flag
            if single:
                v, i = pq.rerank_device(qd[0], xd, cd[0], k, ip=ip, check=True)
                assert tuple(v.shape) == (k,) and tuple(i.shape) == (k,)
                v, i = v[None], i[None]
            else:
                v, i = pq.rerank_device(qd, xd, cd, k, ip=ip, check=True)
                assert tuple(v.shape) == (q.shape[0], k)
            assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
            rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = rerank_raw(pq, qd, xd, cd, k, ip)
            rr.assert_same(rv, ri, want_v, want_i)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [1, 20, 63, 64, 65, 300, 768, 4096])
def test_gpu_rerank_widths(ra, d, half):
    pq = make_pq(ra)
    n, nq = 3001, 8
    q, x = make_data(9901 + d, n, d, nq, half)
    x[17] = x[5]                                    # a tie for whoever names both: the smaller row id first
    cand = make_cand(9902 + d, nq, n, 64)
    cand[1, :2] = (17, 5)
    check_all(pq, q, x, cand, (1, 10, 100))


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 8, 257])
@pytest.mark.parametrize("n_cand", [1, 7, 64, 1000, 1024])
def test_gpu_rerank_candidates_queries_and_k(ra, n_cand, nq):
    pq = make_pq(ra)
    n, d = 5003, 100
    q, x = make_data(9910 + n_cand, n, d, nq, half=(n_cand % 2 == 1))
    cand = make_cand(9911 + nq, nq, n, n_cand)
    check_all(pq, q, x, cand, (1, 10, 100, 1024), single=(nq == 1))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_rerank_respects_row_strides(ra, half):
    """queries, vectors and candidates as column slices of wider tensors: no copy is made, the strides go to the C call"""
    import torch
    pq = make_pq(ra)
    n, d, nq, n_cand = 1234, 77, 5, 40
    q, x = make_data(9920, n, d + 3, nq, half)
    cand = make_cand(9921, nq, n, n_cand + 9)
    qd, xd, cd = torch.from_numpy(q).cuda()[:, :d], torch.from_numpy(x).cuda()[:, 2:2 + d], torch.from_numpy(cand).cuda()[:, 4:4 + n_cand]
    assert not qd.is_contiguous() and not xd.is_contiguous() and not cd.is_contiguous()
    qs, xs, cs = q[:, :d], x[:, 2:2 + d], cand[:, 4:4 + n_cand]
    for ip in (False, True):
        for k in (3, 64):
            want_v, want_i, _ = rr.ref_rerank(qs, xs, cs, k, ip=ip)
            v, i = pq.rerank_device(qd, xd, cd, k, ip=ip, check=True)
            rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = rerank_raw(pq, qd, xd, cd, k, ip)
            rr.assert_same(rv, ri, want_v, want_i)
    # a unit column stride is made by a copy where it is missing
    v, i = pq.rerank_device(qd, torch.from_numpy(np.ascontiguousarray(xs.T)).cuda().T, cd, 5, check=True)
    want_v, want_i, _ = rr.ref_rerank(qs, xs, cs, 5)
    rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)


@pytest.mark.gpu
def test_gpu_rerank_edges(ra):
    """all-(-1) rows, k beyond the candidates, duplicated ids, NaN / Inf / signed zeros, no rows at all"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 300, 70, 4
    q, x = make_data(9930, n, d, nq)
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1]                                       # distance 0 to query 1
    x[9] = 0                                          # inner product +-0
    x[10] = -0.0
    cand = make_cand(9931, nq, n, 30, holes=False)
    cand[0, :] = -1                                   # nothing to return
    cand[1, :11] = (10, 9, 8, 6, 4, 3, 3, 8, -1, 12, 12)
    cand[2, 5:] = -1                                  # k > |C_q|
    cand[3, :8] = (3, 4, 6, 9, 10, 250, 251, 3)
    check_all(pq, q, x, cand, (1, 7, 31, 1024))
    qd = torch.from_numpy(q).cuda()
    empty = torch.zeros((0, d), dtype=torch.float32, device="cuda")
    allpad = torch.full((nq, 30), -1, dtype=torch.int64, device="cuda")
    for ip in (False, True):
        v, i = pq.rerank_device(qd, empty, allpad, 6, ip=ip, check=True)
        assert (i.cpu().numpy() == -1).all() and (v.cpu().numpy() == (-np.inf if ip else np.inf)).all()
        rv, ri = rerank_raw(pq, qd, empty, allpad, 6, ip)
        assert (ri == -1).all() and (rv == (-np.inf if ip else np.inf)).all()


@pytest.mark.gpu
def test_gpu_rerank_reports_bad_ids_and_changes_nothing_else(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    n, d, nq, n_cand = 500, 130, 3, 20
    q, x = make_data(9940, n, d, nq, half=True)
    good = make_cand(9941, nq, n, n_cand)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for row, col, bad in ((0, 0, n), (1, 7, -2), (2, 19, 1 << 40), (1, 3, -(1 << 62)), (0, 1, (1 << 32) + 5)):
        c = good.copy()
        c[row, col] = bad
        cd = torch.from_numpy(c).cuda()
        for ip in (False, True):
            want_v, want_i, flag = rr.ref_rerank(q, x, c, 10, ip=ip)
            assert flag
            with pytest.raises(ra.PanicError, match="index out of bounds"):
                pq.rerank_device(qd, xd, cd, 10, ip=ip, check=True)
            v, i = pq.rerank_device(qd, xd, cd, 10, ip=ip)
            rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            assert _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
            rv, ri = rerank_raw(pq, qd, xd, cd, 10, ip)                  # sentinels intact
            rr.assert_same(rv, ri, want_v, want_i)
            assert _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
    pq.rerank_device(qd, xd, torch.from_numpy(good).cuda(), 10, check=True)   # flag consumed, good input passes
    # with no rows every id but -1 is out of range
    c = torch.tensor([[-1, 0, -1]] * nq, dtype=torch.int64, device="cuda")
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.rerank_device(qd, xd[:0], c, 2, check=True)


@pytest.mark.gpu
def test_gpu_rerank_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    n, d, nq, n_cand = 100, 40, 2, 12
    q, x = make_data(9950, n, d, nq)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    cd = torch.from_numpy(make_cand(9951, nq, n, n_cand)).cuda()
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")

    def call(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, cp=cd.data_ptr(), nc=n_cand,
             c_rs=n_cand, metric=0, k=10, vp=out_v.data_ptr(), v_rs=10, ip_=out_i.data_ptr(), i_rs=10, cb=True):
        return L.pqhip_rerank_f32_dev(pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, cp, nc, c_rs, metric, k,
                                      vp, v_rs, ip_, i_rs, ctypes.c_void_p(s))
    assert call() == _lib.OK and call(metric=1) == _lib.OK
    for bad in (dict(k=0), dict(nc=0), dict(dd=0), dict(metric=2), dict(metric=-1), dict(nq=-1), dict(nn=-1), dict(cb=False),
                dict(qp=None), dict(xp=None), dict(cp=None), dict(vp=None), dict(ip_=None)):
        assert call(**bad) == _lib.EINVAL, bad
    for bad in (dict(k=1025), dict(nc=1025), dict(vb=1), dict(vb=8), dict(nn=(1 << 32) - 1), dict(dd=16385)):
        assert call(**bad) == _lib.EUNSUPPORTED, bad
    for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1), dict(c_rs=n_cand - 1), dict(v_rs=9), dict(i_rs=9)):
        assert call(**bad) == _lib.ESHAPE, bad
    assert call(slot=7) == _lib.ENODEV
    # precedence: EINVAL, ENODEV, EUNSUPPORTED, the null pointers, ESHAPE
    assert call(slot=7, k=0) == _lib.EINVAL
    assert call(slot=7, vb=3) == _lib.ENODEV
    assert call(slot=7, qp=None) == _lib.ENODEV
    assert call(k=1025, qp=None) == _lib.EUNSUPPORTED
    assert call(k=1025, v_rs=9) == _lib.EUNSUPPORTED
    assert call(qp=None, v_rs=9) == _lib.EINVAL
    assert call(nn=0, xp=None) == _lib.OK                                 # no rows: the vectors are not read
    assert call(nn=0, xp=None, x_rs=0) == _lib.OK
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE   # every id but -1 is out of range then
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK            # and the flag is consumed
    assert call(nn=(1 << 32) - 2, k=1025) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    ra.launch_log(reset=True)
    assert call(nq=0) == _lib.OK                                          # n_queries == 0 launches nothing
    assert call(nq=0, qp=None, xp=None, cp=None, vp=None, ip_=None) == _lib.OK
    assert ra.launch_log(reset=True) == ""
    assert call() == _lib.OK
    assert ra.launch_log(reset=True) == "k_rerank_dist + k_rerank_select"
    # the largest width served
    qw, xw = make_data(9952, 9, 16384, 1)
    v, i = pq.rerank_device(torch.from_numpy(qw).cuda(), torch.from_numpy(xw).cuda(), torch.arange(9, device="cuda")[None], 9, check=True)
    want_v, want_i, _ = rr.ref_rerank(qw, xw, np.arange(9)[None], 9)
    rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_rerank_does_not_depend_on_the_grid(ra):
    import torch
    pq = make_pq(ra)
    cases = [(4001, 300, 9, 1000, False), (2000, 65, 1, 1024, True), (600, 20, 33, 7, False)]
    try:
        for n, d, nq, n_cand, half in cases:
            q, x = make_data(9960 + d, n, d, nq, half)
            cand = make_cand(9961 + d, nq, n, n_cand)
            qd, xd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(cand).cuda()
            for ip in (False, True):
                want_v, want_i, _ = rr.ref_rerank(q, x, cand, 100, ip=ip)
                for g in (0, 1, 2, 3, 7, 64, 1024, 5000):
                    ra.set_option(OPTION, g)
                    v, i = pq.rerank_device(qd, xd, cd, 100, ip=ip, check=True)
                    rr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
                    rv, ri = rerank_raw(pq, qd, xd, cd, 100, ip)
                    rr.assert_same(rv, ri, want_v, want_i)
    finally:
        ra.set_option(OPTION, 0)
