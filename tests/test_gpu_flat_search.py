"""GPU tests of the exact search over resident vectors (include/pqhip.h: pqhip_flat_search_f32_dev) against
tests/flat_search_ref.py (rerank_ref.ref_rerank over the allowed rows): indices exact, values bit for bit, both metrics and
both dtypes, through Pq.flat_search_device and through the raw C entry point with padded row strides and sentinels
around the outputs."""
import ctypes

import numpy as np
import pytest

import flat_search_ref as fr
from test_gpu_adc_search_lists import SENT_I, SENT_V, ra  # noqa: F401
from test_gpu_rerank import make_data, make_pq

OPTION = "flat_search_wgs"


def flat_raw(pq, q, x, k, ip, words=None, n_rows=None, pad=3):
    """The C entry point on 2-D tensors as they are strided, output row strides k + pad, sentinels around and between
    the output rows; checks the sentinels and returns (value, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq, d = q.shape
    n = x.shape[0] if n_rows is None else n_rows
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=q.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=q.device)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    rc = _lib.lib().pqhip_flat_search_f32_dev(
        pq._cb(), pq._slot_for(q), q.data_ptr(), nq, q.stride(0) if nq > 1 else max(q.stride(0), d),
        x.data_ptr() if n > 0 else None, x.element_size(), n, d, x.stride(0) if n > 1 else max(x.stride(0), d),
        None if words is None else words.data_ptr(), 1 if ip else 0, k,
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


def check_all(pq, q, x, ks, allow=None, words=None, single=False, metrics=(False, True)):
    """both metrics, every k: Pq.flat_search_device and the raw call against the reference.  allow: bool [n] or None;
    words: the mask words to pass (default: packed from allow)"""
    import torch
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    wd = None
    if allow is not None:
        wd = torch.from_numpy(fr.mask_words(allow) if words is None else words).cuda()
    for ip in metrics:
        for k in ks:
            want_v, want_i = fr.ref_flat_search(q, x, k, ip=ip, allow=allow)
            if single:
                v, i = pq.flat_search_device(qd[0], xd, k, ip=ip, allow=wd, check=True)
                assert tuple(v.shape) == (k,) and tuple(i.shape) == (k,)
                v, i = v[None], i[None]
            else:
                v, i = pq.flat_search_device(qd, xd, k, ip=ip, allow=wd, check=True)
                assert tuple(v.shape) == (q.shape[0], k)
            assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
            fr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = flat_raw(pq, qd, xd, k, ip, words=wd)
            fr.assert_same(rv, ri, want_v, want_i)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300, 768])
def test_gpu_flat_search_widths(ra, d, half):
    """two workgroups (1,100 rows), a pass of four queries and one of a single query"""
    pq = make_pq(ra)
    n, nq = 1100, 5
    q, x = make_data(7100 + d, n, d, nq, half)
    x[17] = x[5]                                    # ties: the smaller row first
    x[1090] = x[1029]
    check_all(pq, q, x, (1, 10, 100))


@pytest.mark.gpu
@pytest.mark.parametrize("d,nq", [(4096, 5), (9216, 4), (9217, 4), (16384, 2)])
def test_gpu_flat_search_wide_rows(ra, d, nq):
    """70 rows; d = 9,216 is the widest row that four queries share a pass on, 16,384 the widest served"""
    pq = make_pq(ra)
    q, x = make_data(7200 + d, 70, d, nq, half=(d == 4096))
    check_all(pq, q, x, (10, 100))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_gpu_flat_search_row_counts(ra, n):
    pq = make_pq(ra)
    q, x = make_data(7300 + n, n, 65, 3, half=(n % 2 == 1))
    check_all(pq, q, x, (1, 64, 65, 1024))


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 8, 9, 17])
def test_gpu_flat_search_queries_and_k(ra, nq):
    """k = 128 / 129 is the boundary between four queries and one per pass, 64 / 65 the boundary between two list lengths"""
    pq = make_pq(ra)
    q, x = make_data(7400 + nq, 1500, 100, nq, half=(nq % 2 == 0))
    check_all(pq, q, x, (1, 10, 64, 65, 100, 128, 129, 1024), single=(nq == 1))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_search_respects_strides_and_unaligned_bases(ra, half):
    """vectors and queries as column slices of wider tensors whose first element is one element into the allocation:
    no copy is made, rows start at odd multiples of the element size"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 1234, 77, 5
    q, x = make_data(7500, n, d + 4, nq, half)
    xbuf = torch.zeros(n * (d + 4) + 1, dtype=torch.float16 if half else torch.float32, device="cuda")
    xbuf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xd = xbuf[1:].view(n, d + 4)[:, 2:2 + d]
    qbuf = torch.zeros(nq * (d + 4) + 1, dtype=torch.float32, device="cuda")
    qbuf[1:] = torch.from_numpy(q).cuda().reshape(-1)
    qd = qbuf[1:].view(nq, d + 4)[:, :d]
    assert not xd.is_contiguous() and not qd.is_contiguous()
    assert xd.data_ptr() % (2 * xd.element_size()) != 0 and xd.stride(0) == d + 4
    qs, xs = q[:, :d], x[:, 2:2 + d]
    allow = np.random.default_rng(7501).random(n) < 0.5
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    for ip in (False, True):
        for k in (3, 64):
            want_v, want_i = fr.ref_flat_search(qs, xs, k, ip=ip)
            v, i = pq.flat_search_device(qd, xd, k, ip=ip, check=True)
            fr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = flat_raw(pq, qd, xd, k, ip)
            fr.assert_same(rv, ri, want_v, want_i)
            want_v, want_i = fr.ref_flat_search(qs, xs, k, ip=ip, allow=allow)
            rv, ri = flat_raw(pq, qd, xd, k, ip, words=wd)
            fr.assert_same(rv, ri, want_v, want_i)
    # a unit column stride is made by a copy where it is missing
    v, i = pq.flat_search_device(qd, torch.from_numpy(np.ascontiguousarray(xs.T)).cuda().T, 5, check=True)
    want_v, want_i = fr.ref_flat_search(qs, xs, 5)
    fr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)


@pytest.mark.gpu
def test_gpu_flat_search_does_not_depend_on_the_workgroups(ra):
    import torch
    pq = make_pq(ra)
    q, x = make_data(7600, 5000, 70, 9)
    x[4999] = x[0]
    allow = np.random.default_rng(7601).random(5000) < 0.4
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    try:
        for ip in (False, True):
            for k in (10, 1000):
                want = fr.ref_flat_search(q, x, k, ip=ip)
                want_m = fr.ref_flat_search(q, x, k, ip=ip, allow=allow)
                first = None
                for g in (0, 1, 2, 3, 5):
                    ra.set_option(OPTION, g)
                    rv, ri = flat_raw(pq, qd, xd, k, ip)
                    fr.assert_same(rv, ri, *want)
                    if first is None:
                        first = (rv.tobytes(), ri.tobytes())
                    assert (rv.tobytes(), ri.tobytes()) == first
                    rv, ri = flat_raw(pq, qd, xd, k, ip, words=wd)
                    fr.assert_same(rv, ri, *want_m)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
def test_gpu_flat_search_edges(ra):
    """duplicate rows, NaN / Inf / signed zeros, k beyond the rows"""
    pq = make_pq(ra)
    n, d, nq = 300, 70, 4
    q, x = make_data(7700, n, d, nq)
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1]                                       # distance 0 to query 1
    x[9] = 0                                          # inner product +-0
    x[10] = -0.0
    x[200] = x[20]
    x[299] = x[20]
    check_all(pq, q, x, (1, 7, 31, 300, 1024))
    allow = np.ones(n, bool)
    allow[[3, 20, 9]] = False
    check_all(pq, q, x, (7, 300), allow=allow)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_search_masks(ra, half):
    """random, all ones, all zero, junk bits beyond n; NaN written over the disallowed rows changes nothing"""
    pq = make_pq(ra)
    n, d, nq = 2085, 130, 5
    q, x = make_data(7800, n, d, nq, half)
    rng = np.random.default_rng(7801)
    for allow in (rng.random(n) < 0.5, rng.random(n) < 0.02, np.ones(n, bool), np.zeros(n, bool)):
        check_all(pq, q, x, (10, 200), allow=allow)
        junk = fr.mask_words(allow).copy()
        junk.view(np.uint32)[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
        check_all(pq, q, x, (10,), allow=allow, words=junk)
    allow = rng.random(n) < 0.3
    allow[16:48] = False                              # whole tiles without an allowed row
    allow[1024:1100] = False
    want = [fr.ref_flat_search(q, x, 50, ip=ip, allow=allow) for ip in (False, True)]
    poisoned = x.copy()
    poisoned[~allow] = np.nan
    import torch
    qd, pd = torch.from_numpy(q).cuda(), torch.from_numpy(poisoned).cuda()
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    for ip in (False, True):
        rv, ri = flat_raw(pq, qd, pd, 50, ip, words=wd)
        fr.assert_same(rv, ri, *want[ip])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 1000, 1024])
def test_gpu_flat_search_equals_the_rerank_of_all_rows(ra, n):
    import torch
    pq = make_pq(ra)
    q, x = make_data(7900 + n, n, 300, 6, half=(n == 65))
    x[n // 2] = x[0]
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    cand = torch.arange(n, device="cuda").expand(6, n).contiguous()
    allow = np.random.default_rng(7901).random(n) < 0.5
    allow[0] = True
    rows = torch.from_numpy(np.flatnonzero(allow)).cuda()
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    for ip in (False, True):
        for k in (1, 100):
            v, i = pq.flat_search_device(qd, xd, k, ip=ip, check=True)
            wv, wi = pq.rerank_device(qd, xd, cand, k, ip=ip, check=True)
            assert torch.equal(i, wi) and v.cpu().numpy().tobytes() == wv.cpu().numpy().tobytes()
            v, i = pq.flat_search_device(qd, xd, k, ip=ip, allow=wd, check=True)
            wv, wi = pq.rerank_device(qd, xd, rows.expand(6, rows.shape[0]).contiguous(), k, ip=ip, check=True)
            assert torch.equal(i, wi) and v.cpu().numpy().tobytes() == wv.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_gpu_flat_search_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    n, d = 100, 40
    q, x = make_data(7950, n, d, 2)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    wd = torch.from_numpy(fr.mask_words(np.ones(n, bool))).cuda()
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")

    def call(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, ap=None, metric=0, k=10,
             vp=out_v.data_ptr(), v_rs=10, ip_=out_i.data_ptr(), i_rs=10, cb=True):
        return L.pqhip_flat_search_f32_dev(pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, ap, metric, k,
                                           vp, v_rs, ip_, i_rs, ctypes.c_void_p(s))
    assert call() == _lib.OK and call(metric=1) == _lib.OK and call(ap=wd.data_ptr()) == _lib.OK
    for bad in (dict(k=0), dict(k=-1), dict(dd=0), dict(metric=2), dict(metric=-1), dict(nq=-1), dict(nn=-1), dict(cb=False),
                dict(qp=None), dict(xp=None), dict(vp=None), dict(ip_=None)):
        assert call(**bad) == _lib.EINVAL, bad
    for bad in (dict(k=1025), dict(vb=1), dict(vb=8), dict(dd=16385, q_rs=16385, x_rs=16385)):
        assert call(**bad) == _lib.EUNSUPPORTED, bad
    for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1), dict(v_rs=9), dict(i_rs=9)):
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
    torch.cuda.synchronize()
    assert (out_i[:10].cpu().numpy() == -1).all() and (out_v[:10].cpu().numpy() == np.inf).all()
    ra.launch_log(reset=True)
    assert call(nq=0) == _lib.OK                                          # n_queries == 0 launches nothing
    assert call(nq=0, qp=None, xp=None, vp=None, ip_=None) == _lib.OK
    assert ra.launch_log(reset=True) == ""
    assert call() == _lib.OK
    assert ra.launch_log(reset=True) == "k_flat_search x2 + k_adc_search_merge x2"
    q8 = torch.from_numpy(make_data(7951, 1, d, 9)[0]).cuda()
    v, i = pq.flat_search_device(q8, xd, 10, ip=True)
    assert ra.launch_log(reset=True) == "k_flat_ip_search<4 queries> x2 + k_adc_ip_search_merge x3 + k_flat_ip_search"
    pq.flat_search_device(q8, xd, 129)
    assert ra.launch_log(reset=True) == "k_flat_search x9 + k_adc_search_merge x9"
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK
    torch.cuda.synchronize()
