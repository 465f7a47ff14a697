"""GPU tests of the exact range search over resident vectors (include/pqhip.h: pqhip_flat_range_f32_dev) against
tests/flat_range_ref.py: lims, indices and the bits of every value, both metrics and both dtypes, through
Pq.flat_range_device and through the raw C entry point with sentinels before and after d_val / d_idx."""
import ctypes

import numpy as np
import pytest

import flat_range_ref as frr
import flat_search_ref as fr
from test_gpu_adc_search_lists import SENT_I, SENT_V, ra  # noqa: F401
from test_gpu_rerank import make_data, make_pq

PAD = 5


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def assert_csr(got, want, prefix=None):
    """lims equal; idx and the bits of val equal (prefix: only the first `prefix` entries were written)"""
    lims, val, idx = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got)
    assert lims.tolist() == want[0].tolist()
    m = want[1].size if prefix is None else min(prefix, want[1].size)
    assert idx[:m].tolist() == want[2][:m].tolist()
    assert bits(val[:m]) == bits(want[1][:m])
    if prefix is None:
        assert val.size == want[1].size and idx.size == want[2].size


def thresholds(values, ip, nq, first=0):
    """One query class per threshold, from the reference's own values so that each is non-trivial by construction: NaN
    (nothing), +-Inf (every non-NaN row), beyond the best value (nothing), exactly a row's value (the equality case), a
    median, query i taking class (first + i) mod 5."""
    out = np.zeros(nq, np.float32)
    for i in range(nq):
        v = values[i][np.isfinite(values[i])]
        if v.size == 0:
            out[i] = 0
            continue
        s = np.sort(v)
        kind = (first + i) % 5
        if kind == 0:
            out[i] = np.nan
        elif kind == 1:
            out[i] = -np.inf if ip else np.inf
        elif kind == 2:
            out[i] = np.nextafter(s[-1], np.float32(np.inf)) if ip else np.nextafter(s[0], np.float32(-np.inf))
        elif kind == 3:
            out[i] = s[-1 - s.size // 7] if ip else s[s.size // 7]          # a row's own value: it qualifies itself
        else:
            out[i] = s[s.size // 2]
    return out


def range_raw(pq, q, x, thr, ip, capacity, words=None, lists=None, null_out=False, expect=None):
    """The C entry point on 2-D tensors as they are strided; d_val / d_idx are `capacity` entries inside buffers with PAD
    sentinels on either side.  Checks that nothing outside the first min(total, capacity) entries was written and returns
    (lims, val, idx) as numpy, val / idx cut to what was written.  lists: (list_off, probes [nq, n_probe])."""
    import torch
    from reductive_amd import _lib
    nq, d = q.shape
    n = x.shape[0]
    vbuf = torch.full((capacity + 2 * PAD,), float(SENT_V), dtype=torch.float32, device=q.device)
    ibuf = torch.full((capacity + 2 * PAD,), SENT_I, dtype=torch.int64, device=q.device)
    lims = torch.full((nq + 3,), SENT_I, dtype=torch.int64, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    head = (pq._cb(), pq._slot_for(q), q.data_ptr(), nq, q.stride(0) if nq > 1 else max(q.stride(0), d),
            x.data_ptr() if n > 0 else None, x.element_size(), n, d, x.stride(0) if n > 1 else max(x.stride(0), d),
            None if words is None else words.data_ptr())
    tail = (1 if ip else 0, thr.data_ptr(), lims.data_ptr() + 8, None if null_out else vbuf.data_ptr() + 4 * PAD,
            None if null_out else ibuf.data_ptr() + 8 * PAD, capacity, stream)
    if lists is None:
        rc = _lib.lib().pqhip_flat_range_f32_dev(*head, *tail)
    else:
        list_off, pr = lists
        rc = _lib.lib().pqhip_flat_range_lists_f32_dev(*head, list_off.data_ptr(), list_off.shape[0] - 1, pr.data_ptr(),
                                                       pr.shape[1], pr.stride(0) if nq > 1 else max(pr.stride(0), pr.shape[1]),
                                                       *tail)
    assert rc == _lib.OK if expect is None else rc == expect, rc
    torch.cuda.synchronize()
    lb, vb, ib = lims.cpu().numpy(), vbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert lb[0] == SENT_I and lb[-1] == SENT_I, "write outside lims"
    total = int(lb[nq + 1])
    m = min(total, capacity)
    assert (vb[:PAD] == SENT_V).all() and (vb[PAD + m:] == SENT_V).all(), "write outside the values"
    assert (ib[:PAD] == SENT_I).all() and (ib[PAD + m:] == SENT_I).all(), "write outside the indices"
    return lb[1:nq + 2], vb[PAD:PAD + m], ib[PAD:PAD + m]


def check_all(pq, q, x, allow=None, words=None, single=False, metrics=(False, True), poisoned=None):
    """both metrics: Pq.flat_range_device and the raw call against the reference, with the thresholds of thresholds().
    allow: bool [n] or None; words: the mask words to pass (default: packed from allow); poisoned: the matrix to hand to
    the device in the place of x (same allowed rows)."""
    import torch
    qd = torch.from_numpy(q).cuda()
    xd = torch.from_numpy(x if poisoned is None else poisoned).cuda()
    wd = None
    if allow is not None:
        wd = torch.from_numpy(fr.mask_words(allow) if words is None else words).cuda()
    for ip in metrics:
        values = frr.all_values(q, x, ip)
        thr = thresholds(values if allow is None else np.where(allow[None], values, np.nan), ip, q.shape[0], 4 if single else 0)
        want = frr.ref_flat_range(q, x, thr, ip=ip, allow=allow, values=values)
        td = torch.from_numpy(thr).cuda()
        if single:
            got = pq.flat_range_device(qd[0], xd, float(thr[0]), ip=ip, allow=wd, check=True)
            assert tuple(got[0].shape) == (2,)
        else:
            got = pq.flat_range_device(qd, xd, td, ip=ip, allow=wd, check=True)
        assert str(got[0].dtype) == "torch.int64" and str(got[1].dtype) == "torch.float32" and str(got[2].dtype) == "torch.int64"
        assert_csr(got, want)
        assert_csr(range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 7, words=wd), want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300])
def test_gpu_flat_range_widths(ra, d, half):
    """two workgroups (1,100 rows), a pass of four queries and one of a single query"""
    pq = make_pq(ra)
    q, x = make_data(8100 + d, 1100, d, 5, half)
    x[17] = x[5]
    x[1090] = x[1029]
    check_all(pq, q, x)


@pytest.mark.gpu
def test_gpu_flat_range_one_query_per_pass_beyond_9216(ra):
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    q, x = make_data(8200, 70, 9217, 2)
    import torch
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    for ip in (False, True):
        values = frr.all_values(q, x, ip)
        thr = np.array([np.sort(values[0])[35], np.sort(values[1])[20]], np.float32)
        want = frr.ref_flat_range(q, x, thr, ip=ip, values=values)
        assert 0 < want[0][1] < 70
        ra.launch_log(reset=True)
        assert_csr(pq.flat_range_device(qd, xd, thr, ip=ip), want)
        name = "k_flat_ip_range" if ip else "k_flat_range"
        assert ra.launch_log(reset=True) == "%s x4 + k_adc_range_scan x2" % name
        assert_csr(range_raw(pq, qd, xd, torch.from_numpy(thr).cuda(), ip, 200), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2100])
def test_gpu_flat_range_row_counts(ra, n):
    pq = make_pq(ra)
    q, x = make_data(8300 + n, n, 65, 5, half=(n % 2 == 1))
    want = check_all(pq, q, x)
    if n == 0:
        assert want[0].tolist() == [0] * 6
    check_all(pq, q[:1], x, single=True)


@pytest.mark.gpu
def test_gpu_flat_range_nan_and_inf_rows(ra):
    pq = make_pq(ra)
    n, d = 300, 70
    q, x = make_data(8400, n, d, 5)
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[3]                                       # distance 0 to query 3: the equality class holds a zero
    x[9] = 0
    x[10] = -0.0
    x[200] = x[20]
    x[299] = x[20]
    want = check_all(pq, q, x)
    assert want[0][2] - want[0][1] < n                # the NaN rows are in no result
    allow = np.ones(n, bool)
    allow[[3, 20, 9]] = False
    check_all(pq, q, x, allow=allow)


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True])
def test_gpu_flat_range_capacity(ra, ip):
    import torch
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    q, x = make_data(8500, 1500, 40, 5, half=ip)
    values = frr.all_values(q, x, ip)
    thr = thresholds(values, ip, 5)
    want = frr.ref_flat_range(q, x, thr, ip=ip, values=values)
    total = int(want[0][-1])
    assert total > 1500
    qd, xd, td = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(thr).cuda()
    ra.launch_log(reset=True)
    lims, val, idx = range_raw(pq, qd, xd, td, ip, 0, null_out=True)         # a count call: null outputs, no fill
    assert lims.tolist() == want[0].tolist() and val.size == 0
    name = "k_flat_ip_range" if ip else "k_flat_range"
    assert ra.launch_log(reset=True) == "%s<4 queries> + k_adc_range_scan x2 + %s" % (name, name)
    for cap in (total - 1, 13, total, total + 100):
        got = range_raw(pq, qd, xd, td, ip, cap)
        assert got[1].size == min(cap, total)
        assert_csr(got, want, prefix=cap)
    # the wrapper: a first call that is too small is repeated once with the exact size
    for cap in (None, 0, 13, total, 1 << 12):
        ra.launch_log(reset=True)
        assert_csr(pq.flat_range_device(qd, xd, td, ip=ip, capacity=cap), want)
        calls = 2 if cap in (0, 13) else 1
        assert ra.launch_log(reset=True).count("k_adc_range_scan x%d" % (2 * calls)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_masks(ra, half):
    """random, all ones, all zero, junk bits beyond n, whole tiles and whole 1,024-row ranges clear; NaN written over the
    disallowed rows changes nothing"""
    pq = make_pq(ra)
    n, d, nq = 2085, 50, 5
    q, x = make_data(8600, n, d, nq, half)
    rng = np.random.default_rng(8601)
    for allow in (rng.random(n) < 0.5, rng.random(n) < 0.02, np.ones(n, bool), np.zeros(n, bool)):
        want = check_all(pq, q, x, allow=allow)
        assert want[0][2] - want[0][1] == int(allow.sum())
        junk = fr.mask_words(allow).copy()
        junk.view(np.uint32)[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
        check_all(pq, q, x, allow=allow, words=junk, metrics=(False,))
    allow = rng.random(n) < 0.3
    allow[16:48] = False                              # whole tiles without an allowed row
    allow[1024:2048] = False                          # a whole workgroup range
    poisoned = x.copy()
    poisoned[~allow] = np.nan
    check_all(pq, q, x, allow=allow, poisoned=poisoned)


@pytest.mark.gpu
def test_gpu_flat_range_does_not_depend_on_the_grid(ra):
    import torch
    pq = make_pq(ra)
    n = 5000
    q, x = make_data(8700, n, 70, 5)
    x[4999] = x[0]
    allow = np.random.default_rng(8701).random(n) < 0.4
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    try:
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            thr = thresholds(values, ip, 5)
            td = torch.from_numpy(thr).cuda()
            want = frr.ref_flat_range(q, x, thr, ip=ip, values=values)
            want_m = frr.ref_flat_range(q, x, thr, ip=ip, allow=allow, values=values)
            first = None
            for g in (0, 1, 2, 3, 7, frr.grid_cap()):
                ra.set_option(frr.OPTION, g)
                got = range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 3)
                assert_csr(got, want)
                blob = tuple(a.tobytes() for a in got)
                first = first or blob
                assert blob == first
                assert_csr(range_raw(pq, qd, xd, td, ip, int(want_m[0][-1]), words=wd), want_m)
            ra.set_option(frr.OPTION, 0)
            # the 5-query call against five single-query calls
            at = 0
            for i in range(5):
                l, v, r = range_raw(pq, qd[i:i + 1], xd, td[i:i + 1], ip, n)
                cnt = int(want[0][i + 1] - want[0][i])
                assert l.tolist() == [0, cnt]
                assert v.tobytes() == got[1][at:at + cnt].tobytes() and r.tobytes() == got[2][at:at + cnt].tobytes()
                at += cnt
    finally:
        ra.set_option(frr.OPTION, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_respects_strides_and_unaligned_bases(ra, half):
    """vectors and queries as column slices of wider tensors whose first element is one element into the allocation"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 1234, 77, 5
    q, x = make_data(8800, n, d + 4, nq, half)
    xbuf = torch.zeros(n * (d + 4) + 1, dtype=torch.float16 if half else torch.float32, device="cuda")
    xbuf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xd = xbuf[1:].view(n, d + 4)[:, 2:2 + d]
    qbuf = torch.zeros(nq * (d + 4) + 1, dtype=torch.float32, device="cuda")
    qbuf[1:] = torch.from_numpy(q).cuda().reshape(-1)
    qd = qbuf[1:].view(nq, d + 4)[:, :d]
    assert not xd.is_contiguous() and not qd.is_contiguous()
    assert xd.data_ptr() % (2 * xd.element_size()) != 0 and xd.stride(0) == d + 4
    qs, xs = np.ascontiguousarray(q[:, :d]), np.ascontiguousarray(x[:, 2:2 + d])
    allow = np.random.default_rng(8801).random(n) < 0.5
    wd = torch.from_numpy(fr.mask_words(allow)).cuda()
    for ip in (False, True):
        values = frr.all_values(qs, xs, ip)
        thr = thresholds(values, ip, nq)
        td = torch.from_numpy(thr).cuda()
        want = frr.ref_flat_range(qs, xs, thr, ip=ip, values=values)
        assert_csr(pq.flat_range_device(qd, xd, td, ip=ip, check=True), want)
        assert_csr(range_raw(pq, qd, xd, td, ip, int(want[0][-1])), want)
        want = frr.ref_flat_range(qs, xs, thr, ip=ip, allow=allow, values=values)
        assert_csr(range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 1, words=wd), want)
    # a unit column stride is made by a copy where it is missing
    values = frr.all_values(qs, xs)
    thr = thresholds(values, False, nq)
    got = pq.flat_range_device(qd, torch.from_numpy(np.ascontiguousarray(xs.T)).cuda().T, thr, check=True)
    assert_csr(got, frr.ref_flat_range(qs, xs, thr, values=values))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 1000, 1024])
def test_gpu_flat_range_values_are_the_flat_search_values(ra, n):
    """the cross-check: the rows of flat_search_device with k = 1,024 that pass the predicate, with their values"""
    import torch
    pq = make_pq(ra)
    q, x = make_data(8900 + n, n, 300, 6, half=(n == 65))
    x[n // 2] = x[0]
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    for ip in (False, True):
        top_v, top_i = (t.cpu().numpy() for t in pq.flat_search_device(qd, xd, 1024, ip=ip))
        thr = np.array([np.sort(top_v[i][top_i[i] >= 0])[(n - 1) // 2] for i in range(6)], np.float32)
        lims, val, idx = (t.cpu().numpy() for t in pq.flat_range_device(qd, xd, thr, ip=ip))
        for i in range(6):
            ok = (top_i[i] >= 0) & ((top_v[i] >= thr[i]) if ip else (top_v[i] <= thr[i]))
            order = np.argsort(top_i[i][ok])
            assert ok.sum() >= 1
            assert idx[lims[i]:lims[i + 1]].tolist() == top_i[i][ok][order].tolist()
            assert bits(val[lims[i]:lims[i + 1]]) == bits(top_v[i][ok][order])


@pytest.mark.gpu
def test_gpu_flat_range_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    n, d = 100, 40
    q, x = make_data(8950, n, d, 2)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    wd = torch.from_numpy(fr.mask_words(np.ones(n, bool))).cuda()
    td = torch.full((2,), float("inf"), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(200, dtype=torch.float32, device="cuda")
    out_i = torch.empty(200, dtype=torch.int64, device="cuda")
    lims = torch.full((3,), -5, dtype=torch.int64, device="cuda")

    def call(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, ap=None, metric=0,
             tp=td.data_ptr(), lp=lims.data_ptr(), vp=out_v.data_ptr(), ip_=out_i.data_ptr(), cap=200, cb=True):
        return L.pqhip_flat_range_f32_dev(pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, ap, metric, tp, lp,
                                          vp, ip_, cap, ctypes.c_void_p(s))
    assert call() == _lib.OK and call(metric=1) == _lib.OK and call(ap=wd.data_ptr()) == _lib.OK
    for bad in (dict(dd=0), dict(metric=2), dict(metric=-1), dict(nq=-1), dict(nn=-1), dict(cap=-1), dict(cb=False), dict(qp=None),
                dict(xp=None), dict(vp=None), dict(ip_=None), dict(tp=None), dict(lp=None)):
        assert call(**bad) == _lib.EINVAL, bad
    for bad in (dict(vb=1), dict(vb=8), dict(dd=16385, q_rs=16385, x_rs=16385)):
        assert call(**bad) == _lib.EUNSUPPORTED, bad
    for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1)):
        assert call(**bad) == _lib.ESHAPE, bad
    assert call(slot=7) == _lib.ENODEV
    # precedence: EINVAL, ENODEV, EUNSUPPORTED, the null pointers, ESHAPE
    assert call(slot=7, cap=-1) == _lib.EINVAL
    assert call(slot=7, vb=3) == _lib.ENODEV
    assert call(slot=7, qp=None) == _lib.ENODEV
    assert call(vb=3, lp=None) == _lib.EUNSUPPORTED
    assert call(vb=3, q_rs=d - 1) == _lib.EUNSUPPORTED
    assert call(lp=None, q_rs=d - 1) == _lib.EINVAL
    assert call(cap=0, vp=None, ip_=None) == _lib.OK                      # a count call takes null outputs
    assert call(nn=0, xp=None) == _lib.OK                                 # no rows: the vectors are not read
    assert call(nn=0, xp=None, x_rs=0) == _lib.OK
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0, 0, 0]
    ra.launch_log(reset=True)
    lims.fill_(-5)
    assert call(nq=0) == _lib.OK                                          # n_queries == 0 launches and writes nothing
    assert call(nq=0, qp=None, xp=None, vp=None, ip_=None, tp=None, lp=None) == _lib.OK
    torch.cuda.synchronize()
    assert ra.launch_log(reset=True) == "" and lims.cpu().tolist() == [-5, -5, -5]
    assert call() == _lib.OK
    assert ra.launch_log(reset=True) == "k_flat_range x4 + k_adc_range_scan x2"
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0, 100, 200]
    q9 = torch.from_numpy(make_data(8951, 1, d, 9)[0]).cuda()
    pq.flat_range_device(q9, xd, 0.0, ip=True)
    assert ra.launch_log(reset=True) == "k_flat_ip_range<4 queries> x4 + k_adc_range_scan x3 + k_flat_ip_range x2"
    for bad_q in (q9[:, :d - 1], q9.double()):
        with pytest.raises(ra.PanicError):
            pq.flat_range_device(bad_q, xd, 0.0)
    with pytest.raises(ra.PanicError):
        pq.flat_range_device(q9, xd, [0.0, 1.0])                          # one threshold, or one per query
    with pytest.raises(ra.PanicError):
        pq.flat_range_device(q9, xd, 0.0, capacity=-1)
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK
    torch.cuda.synchronize()
