"""GPU tests of the exact search in probed lists (include/pqhip.h: pqhip_flat_search_lists_f32_dev) against
tests/flat_lists_ref.py (flat_search_ref.ref_flat_search under the mask of the probed, allowed rows): indices exact, values
bit for bit, both metrics and both dtypes, through Pq.flat_search_lists_device and through the raw C entry point with
padded row strides and sentinels around the outputs; and, device to device, against Pq.flat_search_device with the mask
of the same rows.

Seven lists of lengths 17, 0, 1, the rest (> 1,024 rows), 15, 33 and 16: a 16-place tile straddles a boundary of every
kind (into, out of and across an empty list, several short lists in one tile) and the long list spans workgroup slices."""
import ctypes

import numpy as np
import pytest

import flat_lists_ref as flr
from test_gpu_adc_search_lists import SENT_I, SENT_V, ra  # noqa: F401
from test_gpu_rerank import make_data, make_pq

OPTION = "flat_lists_wgs_per_query"
SHORT = (17, 0, 1, None, 15, 33, 16)          # None: the rest of the rows
EMPTY, ONE, REST = 1, 2, 3                    # the lists of length 0, 1 and the rest


def make_lists(n):
    return flr.offsets([n - sum(l for l in SHORT if l is not None) if l is None else l for l in SHORT])


def make_probes(seed, nq, n_probe, n_lists=len(SHORT)):
    """distinct list ids per row, -1 padding inside some rows; row 0 names the one-row list alone (k > T_q)"""
    rng = np.random.default_rng(seed)
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    if n_probe > 1:
        pr[rng.random(pr.shape) < 0.2] = -1
        if nq > 1:
            pr[1, 0] = REST if REST not in pr[1] else pr[1, 0]       # the long list in a row with padding behind it
            pr[1, 1] = -1
    pr[0] = -1
    pr[0, n_probe // 2] = ONE
    return pr


def lists_raw(pq, q, x, off, pr, k, ip, words=None, n_rows=None, n_lists=None, pad=3, rc_want=None):
    """The C entry point on 2-D tensors as they are strided, the probe rows inside a wider tensor whose other columns
    name the long list, output row strides k + pad, sentinels around and between the output rows; checks the sentinels
    and returns (value, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq, d = q.shape
    n = x.shape[0] if n_rows is None else n_rows
    n_probe = pr.shape[1]
    wide = torch.full((nq, n_probe + 2), REST, dtype=torch.int64, device=q.device)
    wide[:, :n_probe] = pr
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=q.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=q.device)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    rc = _lib.lib().pqhip_flat_search_lists_f32_dev(
        pq._cb(), pq._slot_for(q), q.data_ptr(), nq, q.stride(0) if nq > 1 else max(q.stride(0), d),
        x.data_ptr() if n > 0 else None, x.element_size(), n, d, x.stride(0) if n > 1 else max(x.stride(0), d),
        off.data_ptr(), off.shape[0] - 1 if n_lists is None else n_lists, wide.data_ptr(), n_probe, n_probe + 2,
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


def flag_is_down(pq):
    import torch
    from reductive_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK


def check_all(pq, q, x, off, pr, ks, allow=None, single=False, metrics=(False, True)):
    """both metrics, every k: Pq.flat_search_lists_device and the raw call against the reference"""
    import torch
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    od, pd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda()
    wd = None if allow is None else torch.from_numpy(flr.mask_words(allow)).cuda()
    for ip in metrics:
        for k in ks:
            want_v, want_i, flag = flr.ref_flat_search_lists(q, x, off, pr, k, ip=ip, allow=allow)
            assert not flag
            if single:
                v, i = pq.flat_search_lists_device(qd[0], xd, od, pd[0], k, ip=ip, allow=wd, check=True)
                assert tuple(v.shape) == (k,) and tuple(i.shape) == (k,)
                v, i = v[None], i[None]
            else:
                v, i = pq.flat_search_lists_device(qd, xd, od, pd, k, ip=ip, allow=wd, check=True)
                assert tuple(v.shape) == (q.shape[0], k)
            assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
            flr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = lists_raw(pq, qd, xd, od, pd, k, ip, words=wd)
            flr.assert_same(rv, ri, want_v, want_i)
    assert flag_is_down(pq)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300])
def test_gpu_flat_lists_widths(ra, d, half):
    pq = make_pq(ra)
    n, nq = 1300, 5
    q, x = make_data(8100 + d, n, d, nq, half)
    x[1299] = x[20]                                 # ties across lists: the smaller position first
    x[5] = x[40]
    check_all(pq, q, x, make_lists(n), make_probes(8100 + d, nq, 3), (1, 10, 129))


@pytest.mark.gpu
@pytest.mark.parametrize("n_probe", [1, 3, 7])
@pytest.mark.parametrize("nq", [1, 3, 5])
def test_gpu_flat_lists_queries_probes_and_k(ra, nq, n_probe):
    """64 / 65 and 128 / 129 are boundaries between list lengths; row 0 probes one row, so k > T_q there"""
    pq = make_pq(ra)
    n = 1100 + 100 * nq + n_probe
    q, x = make_data(8200 + 10 * nq + n_probe, n, 65, nq, half=(nq == 3))
    pr = make_probes(8200 + 10 * nq + n_probe, nq, n_probe)
    if nq == 5 and n_probe == 7:
        pr[4] = np.random.default_rng(8299).permutation(7)      # every list, shuffled, no padding
    check_all(pq, q, x, make_lists(n), pr, (1, 10, 64, 65, 128, 129, 1024), single=(nq == 1))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_lists_equal_the_exhaustive_search_under_the_mask(ra, half):
    """device to device: every list probed in a shuffled order is the unmasked exhaustive call; any probe set is the
    exhaustive call with that set's mask, query by query; with allow= it is the call with the intersection"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 5000, 70, 5
    q, x = make_data(8300, n, d, nq, half)
    x[4999] = x[0]
    off = make_lists(n)
    qd, xd, od = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    rng = np.random.default_rng(8301)
    every = np.stack([rng.permutation(7) for _ in range(nq)]).astype(np.int64)
    some = make_probes(8302, nq, 4)
    allow = rng.random(n) < 0.4
    wd = torch.from_numpy(flr.mask_words(allow)).cuda()
    for ip in (False, True):
        for k in (10, 200):
            v, i = pq.flat_search_lists_device(qd, xd, od, torch.from_numpy(every).cuda(), k, ip=ip, check=True)
            wv, wi = pq.flat_search_device(qd, xd, k, ip=ip)
            assert torch.equal(i, wi) and v.cpu().numpy().tobytes() == wv.cpu().numpy().tobytes()
            for words, flags in ((None, None), (wd, allow)):
                v, i = pq.flat_search_lists_device(qd, xd, od, torch.from_numpy(some).cuda(), k, ip=ip, allow=words, check=True)
                for qi in range(nq):
                    mask = flr.probed_mask(off, some[qi], n)[0]
                    if flags is not None:
                        mask &= flags
                    md = torch.from_numpy(flr.mask_words(mask)).cuda()
                    wv, wi = pq.flat_search_device(qd[qi], xd, k, ip=ip, allow=md)
                    assert torch.equal(i[qi], wi) and v[qi].cpu().numpy().tobytes() == wv.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_gpu_flat_lists_do_not_depend_on_the_workgroups_per_query(ra):
    import torch
    pq = make_pq(ra)
    n, nq = 5000, 3
    q, x = make_data(8400, n, 70, nq)
    x[4999] = x[0]
    off = make_lists(n)
    pr = make_probes(8401, nq, 7)
    pr[2] = np.random.default_rng(8402).permutation(7)
    allow = np.random.default_rng(8403).random(n) < 0.4
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    od, pd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda()
    wd = torch.from_numpy(flr.mask_words(allow)).cuda()
    try:
        for ip in (False, True):
            for k in (10, 1000):
                want = flr.ref_flat_search_lists(q, x, off, pr, k, ip=ip)[:2]
                want_m = flr.ref_flat_search_lists(q, x, off, pr, k, ip=ip, allow=allow)[:2]
                first = None
                for g in (0, 1, 2, 3, 16):
                    ra.set_option(OPTION, g)
                    rv, ri = lists_raw(pq, qd, xd, od, pd, k, ip)
                    flr.assert_same(rv, ri, *want)
                    if first is None:
                        first = (rv.tobytes(), ri.tobytes())
                    assert (rv.tobytes(), ri.tobytes()) == first
                    rv, ri = lists_raw(pq, qd, xd, od, pd, k, ip, words=wd)
                    flr.assert_same(rv, ri, *want_m)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_lists_respect_strides_and_unaligned_bases(ra, half):
    """vectors and queries as column slices of wider tensors whose first element is one element into the allocation:
    no copy is made, rows start at odd multiples of the element size; the probe row stride exceeds n_probe (lists_raw)"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 1234, 77, 5
    q, x = make_data(8500, n, d + 4, nq, half)
    xbuf = torch.zeros(n * (d + 4) + 1, dtype=torch.float16 if half else torch.float32, device="cuda")
    xbuf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xd = xbuf[1:].view(n, d + 4)[:, 2:2 + d]
    qbuf = torch.zeros(nq * (d + 4) + 1, dtype=torch.float32, device="cuda")
    qbuf[1:] = torch.from_numpy(q).cuda().reshape(-1)
    qd = qbuf[1:].view(nq, d + 4)[:, :d]
    assert not xd.is_contiguous() and not qd.is_contiguous()
    assert xd.data_ptr() % (2 * xd.element_size()) != 0 and xd.stride(0) == d + 4
    qs, xs = q[:, :d], x[:, 2:2 + d]
    off = make_lists(n)
    pr = make_probes(8501, nq, 3)
    od = torch.from_numpy(off).cuda()
    pwide = torch.full((nq, 6), REST, dtype=torch.int64, device="cuda")
    pwide[:, 1:4] = torch.from_numpy(pr).cuda()
    pd = pwide[:, 1:4]                                # a column slice: row stride 6
    allow = np.random.default_rng(8502).random(n) < 0.5
    wd = torch.from_numpy(flr.mask_words(allow)).cuda()
    for ip in (False, True):
        for k in (3, 64):
            want_v, want_i, _ = flr.ref_flat_search_lists(qs, xs, off, pr, k, ip=ip)
            v, i = pq.flat_search_lists_device(qd, xd, od, pd, k, ip=ip, check=True)
            flr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            rv, ri = lists_raw(pq, qd, xd, od, pd, k, ip)
            flr.assert_same(rv, ri, want_v, want_i)
            want_v, want_i, _ = flr.ref_flat_search_lists(qs, xs, off, pr, k, ip=ip, allow=allow)
            rv, ri = lists_raw(pq, qd, xd, od, pd, k, ip, words=wd)
            flr.assert_same(rv, ri, want_v, want_i)


@pytest.mark.gpu
def test_gpu_flat_lists_bad_probes_and_offsets_raise_the_flag(ra):
    """an id outside [0, n_lists) is skipped, an offset beyond n_rows is clamped: the result is the reference's,
    check=True raises the range error and the flag is down afterwards"""
    import torch
    from reductive_amd.pq import PanicError
    pq = make_pq(ra)
    n, nq = 1300, 3
    q, x = make_data(8600, n, 65, nq)
    off = make_lists(n)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    pr = make_probes(8601, nq, 3)
    bad_id = pr.copy()
    bad_id[2, 1] = 7                                  # n_lists
    bad_neg = pr.copy()
    bad_neg[1, 2] = -2
    bad_off = off.copy()
    bad_off[7] = n + 500                              # the last list (16 rows) runs past the matrix
    last = pr.copy()
    last[2, 0] = 6
    inverted = off.copy()
    inverted[1] = 40                                  # list 0 = [0, 40) overlaps; list 1 = [40, 17) is inverted
    inv_pr = pr.copy()
    inv_pr[2] = (EMPTY, 4, -1)
    for o, p in ((off, bad_id), (off, bad_neg), (bad_off, last), (inverted, inv_pr)):
        od, pd = torch.from_numpy(o).cuda(), torch.from_numpy(p).cuda()
        for ip in (False, True):
            want_v, want_i, flag = flr.ref_flat_search_lists(q, x, o, p, 20, ip=ip)
            assert flag
            v, i = pq.flat_search_lists_device(qd, xd, od, pd, 20, ip=ip)
            flr.assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            with pytest.raises(PanicError, match="index out of bounds"):
                pq.flat_search_lists_device(qd, xd, od, pd, 20, ip=ip, check=True)
            assert flag_is_down(pq)
    v, i = pq.flat_search_lists_device(qd, xd, torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda(), 20, check=True)
    assert flag_is_down(pq)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_lists_nan_rows_outside_the_searched_set_change_nothing(ra, half):
    """NaN written over the unprobed lists and over the rows whose mask bit is clear: no byte of them is loaded"""
    import torch
    pq = make_pq(ra)
    n, nq = 1300, 3
    q, x = make_data(8700, n, 130, nq, half)
    off = make_lists(n)
    pr = np.array([[REST, 0, -1], [4, 5, 6], [5, -1, REST]], np.int64)
    allow = np.random.default_rng(8701).random(n) < 0.5
    allow[off[REST] + 16:off[REST] + 80] = False      # whole tiles without an allowed row
    searched = np.stack([flr.probed_mask(off, pr[qi], n)[0] for qi in range(nq)]).any(0)
    od, pd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda()
    qd = torch.from_numpy(q).cuda()
    for flags in (None, allow):
        poisoned = x.copy()
        poisoned[~searched if flags is None else ~(searched & flags)] = np.nan
        wd = None if flags is None else torch.from_numpy(flr.mask_words(flags)).cuda()
        for ip in (False, True):
            want_v, want_i, _ = flr.ref_flat_search_lists(q, x, off, pr, 50, ip=ip, allow=flags)
            assert not np.isnan(want_v).any()
            rv, ri = lists_raw(pq, qd, torch.from_numpy(poisoned).cuda(), od, pd, 50, ip, words=wd)
            flr.assert_same(rv, ri, want_v, want_i)


@pytest.mark.gpu
def test_gpu_flat_lists_edges(ra):
    """NaN / Inf / signed zeros in probed rows, duplicate rows in different lists"""
    pq = make_pq(ra)
    n, nq = 1300, 4
    q, x = make_data(8800, n, 70, nq)
    off = make_lists(n)
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1]
    x[9] = 0
    x[10] = -0.0
    x[1290] = x[20]
    x[200] = x[20]
    pr = np.tile(np.array([0, REST, 6, 5], np.int64), (nq, 1))
    pr[3] = (6, 5, 0, -1)
    check_all(pq, q, x, off, pr, (1, 7, 31, 1024))
    allow = np.ones(n, bool)
    allow[[3, 20, 9]] = False
    check_all(pq, q, x, off, pr, (7, 300), allow=allow)


@pytest.mark.gpu
def test_gpu_flat_lists_status_codes_and_degenerate_sizes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    n, d = 100, 40
    q, x = make_data(8900, n, d, 2)
    qd, xd = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
    od = torch.tensor([0, 30, 30, 100], dtype=torch.int64, device="cuda")
    pd = torch.tensor([[0, 2], [1, -1]], dtype=torch.int64, device="cuda")
    wd = torch.from_numpy(flr.mask_words(np.ones(n, bool))).cuda()
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")

    def call(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, op=od.data_ptr(), nl=3,
             pp=pd.data_ptr(), npr=2, p_rs=2, ap=None, metric=0, k=10, vp=out_v.data_ptr(), v_rs=10, ip_=out_i.data_ptr(),
             i_rs=10, cb=True):
        return L.pqhip_flat_search_lists_f32_dev(pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, op, nl, pp,
                                                 npr, p_rs, ap, metric, k, vp, v_rs, ip_, i_rs, ctypes.c_void_p(s))
    assert call() == _lib.OK and call(metric=1) == _lib.OK and call(ap=wd.data_ptr()) == _lib.OK
    for bad in (dict(k=0), dict(k=-1), dict(dd=0), dict(metric=2), dict(metric=-1), dict(nq=-1), dict(nn=-1), dict(cb=False),
                dict(nl=-1), dict(npr=0), dict(npr=-3), dict(qp=None), dict(xp=None), dict(vp=None), dict(ip_=None),
                dict(op=None), dict(pp=None)):
        assert call(**bad) == _lib.EINVAL, bad
    for bad in (dict(k=1025), dict(vb=1), dict(vb=8), dict(dd=16385, q_rs=16385, x_rs=16385), dict(nn=(1 << 32) - 1),
                dict(npr=1 << 24, p_rs=1 << 24)):
        assert call(**bad) == _lib.EUNSUPPORTED, bad
    for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1), dict(v_rs=9), dict(i_rs=9), dict(p_rs=1)):
        assert call(**bad) == _lib.ESHAPE, bad
    assert call(slot=7) == _lib.ENODEV
    # precedence: EINVAL, ENODEV, EUNSUPPORTED, the null pointers, ESHAPE
    assert call(slot=7, npr=0) == _lib.EINVAL
    assert call(slot=7, vb=3) == _lib.ENODEV
    assert call(slot=7, pp=None) == _lib.ENODEV
    assert call(k=1025, pp=None) == _lib.EUNSUPPORTED
    assert call(k=1025, p_rs=1) == _lib.EUNSUPPORTED
    assert call(pp=None, p_rs=1) == _lib.EINVAL
    for empty in (dict(nn=0, xp=None), dict(nn=0, xp=None, x_rs=0), dict(nl=0)):      # no rows / no lists: padding only
        out_i.zero_()
        assert call(**empty) == _lib.OK
        torch.cuda.synchronize()
        assert (out_i.cpu().numpy() == -1).all() and (out_v.cpu().numpy() == np.inf).all()
    ra.launch_log(reset=True)
    assert call(nq=0) == _lib.OK                                          # n_queries == 0 launches nothing
    assert call(nq=0, qp=None, xp=None, vp=None, ip_=None, op=None, pp=None) == _lib.OK
    assert ra.launch_log(reset=True) == ""
    assert call() == _lib.OK
    assert ra.launch_log(reset=True) == "k_adc_lists_plan + k_flat_search_lists + k_adc_search_merge"
    assert call(metric=1) == _lib.OK
    assert ra.launch_log(reset=True) == "k_adc_lists_plan + k_flat_ip_search_lists + k_adc_ip_search_merge"
    torch.cuda.synchronize()
    assert out_i.cpu().numpy()[10:].tolist() == [-1] * 10                 # query 1 probes the empty list
    assert flag_is_down(pq)
