"""GPU tests of the exact range search in probed lists (include/pqhip.h: pqhip_flat_range_lists_f32_dev) against
tests/flat_range_ref.py: lims, positions and the bits of every value in the order of the concatenation of the probed
lists, through Pq.flat_range_lists_device and the raw C entry point with sentinels around d_val / d_idx; and, device to
device, against Pq.flat_range_device.

900 rows in nine lists of lengths 17, 0, 1, 300, 15, 33, 16, 250 and 268: a 16-place tile straddles a boundary of every
kind (into, out of and across an empty list, several short lists in one tile)."""
import ctypes

import numpy as np
import pytest

import flat_lists_ref as flr
import flat_range_ref as frr
from test_gpu_adc_search_lists import ra  # noqa: F401
from test_gpu_flat_range import assert_csr, bits, range_raw, thresholds
from test_gpu_rerank import make_data, make_pq

N = 900
LENGTHS = (17, 0, 1, 300, 15, 33, 16, 250, 268)
EMPTY, ONE = 1, 2
N_PROBE = 3


def make_probes(seed, nq):
    """distinct list ids per row; row 0 names the one-row and the empty list, row 1 has padding inside, row 2 names a
    list twice, row 3 probes across the short lists (tiles that straddle them)"""
    rng = np.random.default_rng(seed)
    pr = np.stack([rng.permutation(len(LENGTHS))[:N_PROBE] for _ in range(nq)]).astype(np.int64)
    pr[0] = (EMPTY, ONE, -1)
    if nq > 1:
        pr[1] = (3, -1, 0)
    if nq > 2:
        pr[2] = (7, 4, 7)
    if nq > 3:
        pr[3] = (4, 5, 6)
    return pr


def device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def flag_is_down(pq):
    import torch
    from reductive_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK


def probed_values(values, off, pr, allow=None):
    """values [nq, n] with NaN where a row is not probed (or not allowed): what thresholds() draws from"""
    out = np.full(values.shape, np.nan, np.float32)
    for i in range(values.shape[0]):
        m, _ = flr.probed_mask(off, pr[i], values.shape[1])
        if allow is not None:
            m = m & allow
        out[i, m] = values[i, m]
    return out


def check_all(pq, q, x, off, pr, allow=None, metrics=(False, True), flagged=False):
    import torch
    qd, xd, od, pd = device(q, x, off, pr)
    wd = None if allow is None else device(flr.mask_words(allow))[0]
    for ip in metrics:
        values = frr.all_values(q, x, ip)
        thr = thresholds(probed_values(values, off, pr, allow), ip, q.shape[0], first=1)
        want = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, allow=allow, values=values)
        td = torch.from_numpy(thr).cuda()
        if flagged:
            with pytest.raises(ra_module().PanicError):
                pq.flat_range_lists_device(qd, xd, od, pd, td, ip=ip, allow=wd, check=True)
            got = pq.flat_range_lists_device(qd, xd, od, pd, td, ip=ip, allow=wd)
            assert not flag_is_down(pq)
        else:
            got = pq.flat_range_lists_device(qd, xd, od, pd, td, ip=ip, allow=wd, check=True)
        assert_csr(got, want)
        assert_csr(range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 7, words=wd, lists=(od, pd)), want)
        if flagged:
            assert not flag_is_down(pq)
    assert flag_is_down(pq)
    return want


def ra_module():
    import reductive_amd
    return reductive_amd


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [20, 65])
def test_gpu_flat_range_lists_widths(ra, d, half):
    pq = make_pq(ra)
    q, x = make_data(9300 + d, N, d, 6, half)
    x[899] = x[20]
    x[5] = x[40]
    off, pr = flr.offsets(LENGTHS), make_probes(9300 + d, 6)
    want = check_all(pq, q, x, off, pr)
    # query 0 (every non-NaN row of its lists): the one row of list ONE; query 2 names list 7 twice: its rows twice
    assert want[0][1] == 1 and want[2][0] == off[ONE]
    seg = want[2][want[0][2]:want[0][3]]
    assert seg.size > 0 and (np.sort(seg[(seg >= off[7]) & (seg < off[8])]).reshape(-1, 2).T[0]
                             == np.unique(seg[(seg >= off[7]) & (seg < off[8])])).all()
    # one query, 1-D probes
    qd, xd, od, pd = device(q, x, off, pr)
    values = frr.all_values(q[3:4], x)
    thr = float(np.sort(values[0][off[4]:off[7]])[30])
    one = pq.flat_range_lists_device(qd[3], xd, od, pd[3], thr, check=True)
    assert tuple(one[0].shape) == (2,)
    assert_csr(one, frr.ref_flat_range_lists(q[3:4], x, off, pr[3:4], thr, values=values))


@pytest.mark.gpu
def test_gpu_flat_range_lists_bad_ids_and_corrupted_offsets(ra):
    """an id out of range is skipped, an offset beyond n is clamped and an inverted range is empty: each raises the
    stream's flag, and no row outside the matrix is read (the matrix ends where its allocation ends)"""
    pq = make_pq(ra)
    q, x = make_data(9400, N, 20, 5)
    off = flr.offsets(LENGTHS)
    pr = make_probes(9400, 5)
    pr[4] = (3, 99, 5)
    check_all(pq, q, x, off, pr, flagged=True)
    pr = make_probes(9401, 5)
    pr[4] = (8, 3, 5)
    clamped = off.copy()
    clamped[9] = N + 5000                                   # list 8 runs past the end: clamped to n
    check_all(pq, q, x, clamped, pr, flagged=True)
    inverted = off.copy()
    inverted[4] = off[3] - 10                               # list 3 is inverted: empty
    check_all(pq, q, x, inverted, pr, flagged=True, metrics=(False,))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_lists_mask_in_position_order(ra, half):
    pq = make_pq(ra)
    q, x = make_data(9500, N, 65, 6, half)
    off, pr = flr.offsets(LENGTHS), make_probes(9500, 6)
    rng = np.random.default_rng(9501)
    for allow in (rng.random(N) < 0.5, np.zeros(N, bool)):
        check_all(pq, q, x, off, pr, allow=allow)
    allow = rng.random(N) < 0.4
    allow[32:64] = False                                    # whole tiles without an allowed row
    poisoned = x.copy()
    poisoned[~allow] = np.nan                               # a disallowed row is not loaded
    import torch
    qd, pd_, od, prd, wd = device(q, poisoned, off, pr, flr.mask_words(allow))
    for ip in (False, True):
        values = frr.all_values(q, x, ip)
        thr = thresholds(probed_values(values, off, pr, allow), ip, 6, first=1)
        want = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, allow=allow, values=values)
        assert_csr(range_raw(pq, qd, pd_, torch.from_numpy(thr).cuda(), ip, int(want[0][-1]), words=wd, lists=(od, prd)), want)


@pytest.mark.gpu
def test_gpu_flat_range_lists_do_not_depend_on_the_workgroups_per_query(ra):
    import torch
    pq = make_pq(ra)
    q, x = make_data(9600, N, 65, 6)
    off, pr = flr.offsets(LENGTHS), make_probes(9600, 6)
    pr[5] = (3, 7, 8)
    allow = np.random.default_rng(9601).random(N) < 0.5
    qd, xd, od, pd, wd = device(q, x, off, pr, flr.mask_words(allow))
    try:
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            thr = thresholds(probed_values(values, off, pr), ip, 6, first=1)
            td = torch.from_numpy(thr).cuda()
            want = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, values=values)
            want_m = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, allow=allow, values=values)
            first = None
            for g in (0, 1, 2, 5, frr.lists_grid_cap()):
                ra.set_option(frr.OPTION_LISTS, g)
                got = range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 2, lists=(od, pd))
                assert_csr(got, want)
                blob = tuple(a.tobytes() for a in got)
                first = first or blob
                assert blob == first
                assert_csr(range_raw(pq, qd, xd, td, ip, int(want_m[0][-1]), words=wd, lists=(od, pd)), want_m)
    finally:
        ra.set_option(frr.OPTION_LISTS, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_lists_equal_the_exhaustive_call(ra, half):
    """every list probed in ascending order is the exhaustive call, byte for byte; any probe row is the exhaustive call
    under the mask of its rows, query by query, as a set and in values"""
    import torch
    pq = make_pq(ra)
    q, x = make_data(9700, N, 65, 5, half)
    x[3, 7] = np.nan
    off = flr.offsets(LENGTHS)
    qd, xd, od = device(q, x, off)
    every = torch.arange(len(LENGTHS), dtype=torch.int64, device="cuda").expand(5, len(LENGTHS)).contiguous()
    pr = make_probes(9700, 5)
    pr[2] = (7, 4, 0)                                       # no list twice: a row is in the masked result once
    prd = torch.from_numpy(pr).cuda()
    for ip in (False, True):
        thr = thresholds(frr.all_values(q, x, ip), ip, 5, first=1)
        td = torch.from_numpy(thr).cuda()
        a = pq.flat_range_lists_device(qd, xd, od, every, td, ip=ip, check=True)
        b = pq.flat_range_device(qd, xd, td, ip=ip)
        assert all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
                   for s, t in zip(a, b))
        assert int(a[0][-1]) > 0
        lims, val, pos = (t.cpu().numpy() for t in pq.flat_range_lists_device(qd, xd, od, prd, td, ip=ip, check=True))
        for i in range(5):
            m, flag = flr.probed_mask(off, pr[i], N)
            assert not flag
            wd = device(flr.mask_words(m))[0]
            l1, v1, r1 = (t.cpu().numpy() for t in pq.flat_range_device(qd[i], xd, float(thr[i]), ip=ip, allow=wd))
            order = np.argsort(pos[lims[i]:lims[i + 1]], kind="stable")
            assert pos[lims[i]:lims[i + 1]][order].tolist() == r1.tolist()
            assert bits(val[lims[i]:lims[i + 1]][order]) == bits(v1)


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True])
def test_gpu_flat_range_lists_capacity(ra, ip):
    import torch
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    q, x = make_data(9800, N, 20, 6, half=ip)
    off, pr = flr.offsets(LENGTHS), make_probes(9800, 6)
    values = frr.all_values(q, x, ip)
    thr = thresholds(probed_values(values, off, pr), ip, 6, first=1)
    want = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, values=values)
    total = int(want[0][-1])
    assert total > 300
    qd, xd, od, pd, td = device(q, x, off, pr, thr)
    ra.launch_log(reset=True)
    lims, val, idx = range_raw(pq, qd, xd, td, ip, 0, lists=(od, pd), null_out=True)     # a count call launches no fill
    assert lims.tolist() == want[0].tolist()
    name = "k_flat_ip_range_lists" if ip else "k_flat_range_lists"
    assert ra.launch_log(reset=True) == "k_adc_lists_plan + %s + k_adc_range_scan" % name
    for cap in (total - 1, 13, total, total + 100):
        got = range_raw(pq, qd, xd, td, ip, cap, lists=(od, pd))
        assert got[1].size == min(cap, total)
        assert_csr(got, want, prefix=cap)
    for cap in (None, 0, 13, total):
        assert_csr(pq.flat_range_lists_device(qd, xd, od, pd, td, ip=ip, capacity=cap), want)


@pytest.mark.gpu
def test_gpu_flat_range_lists_query_chunks_past_the_first(ra):
    """the grid option at its cap leaves 16 queries to a chunk (one scan sums 2^20 counts): 37 queries are two full
    chunks and a shorter third, with thresholds, probe rows and results that differ per query"""
    import torch
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    cap = frr.lists_grid_cap()
    nq = 2 * frr.lists_chunk(1 << 40, N, cap, N_PROBE) + 5
    assert frr.lists_chunk(nq, N, cap, N_PROBE) == 16 and nq == 37
    q, x = make_data(9900, N, 20, nq)
    off = flr.offsets(LENGTHS)
    rng = np.random.default_rng(9901)
    pr = np.stack([rng.permutation(len(LENGTHS))[:N_PROBE] for _ in range(nq)]).astype(np.int64)
    pr[:, 0] = np.where(np.arange(nq) % 2 == 0, 3, pr[:, 0])          # no query without rows
    pr[np.arange(nq) % 2 == 0, 1:] = np.where(pr[np.arange(nq) % 2 == 0, 1:] == 3, 7, pr[np.arange(nq) % 2 == 0, 1:])
    allow = rng.random(N) < 0.8
    qd, xd, od, wd = device(q, x, off, flr.mask_words(allow))
    wide = torch.full((nq, N_PROBE + 2), 3, dtype=torch.int64, device="cuda")      # probe rows inside a wider tensor
    wide[:, :N_PROBE] = torch.from_numpy(pr).cuda()
    pd = wide[:, :N_PROBE]
    try:
        ra.set_option(frr.OPTION_LISTS, cap)
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            pv = probed_values(values, off, pr, allow)
            thr = np.array([np.sort(pv[i][np.isfinite(pv[i])])[::-1 if ip else 1][3 + i] for i in range(nq)], np.float32)
            want = frr.ref_flat_range_lists(q, x, off, pr, thr, ip=ip, allow=allow, values=values)
            counts = np.diff(want[0])
            assert counts.min() >= 4 and len(set(counts.tolist())) > 10 and len(set(thr.tolist())) == nq
            td = torch.from_numpy(thr).cuda()
            ra.launch_log(reset=True)
            got = range_raw(pq, qd, xd, td, ip, int(want[0][-1]) + 3, words=wd, lists=(od, pd))
            name = "k_flat_ip_range_lists" if ip else "k_flat_range_lists"
            assert ra.launch_log(reset=True) == "k_adc_lists_plan x3 + %s x6 + k_adc_range_scan x3" % name
            assert_csr(got, want)
            assert_csr(pq.flat_range_lists_device(qd, xd, od, pd, td, ip=ip, allow=wd, capacity=50), want)
    finally:
        ra.set_option(frr.OPTION_LISTS, 0)


@pytest.mark.gpu
def test_gpu_flat_range_lists_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    d = 20
    q, x = make_data(9950, N, d, 2)
    off, pr = flr.offsets(LENGTHS), make_probes(9950, 2)
    qd, xd, od, pd = device(q, x, off, pr)
    td = torch.full((2,), float("inf"), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(2000, dtype=torch.float32, device="cuda")
    out_i = torch.empty(2000, dtype=torch.int64, device="cuda")
    lims = torch.full((3,), -5, dtype=torch.int64, device="cuda")

    def call(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=N, dd=d, x_rs=d, ap=None, op=od.data_ptr(),
             nl=len(LENGTHS), pp=pd.data_ptr(), n_probe=N_PROBE, p_rs=N_PROBE, metric=0, tp=td.data_ptr(), lp=lims.data_ptr(),
             vp=out_v.data_ptr(), ip_=out_i.data_ptr(), cap=2000, cb=True):
        return L.pqhip_flat_range_lists_f32_dev(pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, ap, op, nl, pp,
                                                n_probe, p_rs, metric, tp, lp, vp, ip_, cap, ctypes.c_void_p(s))
    assert call() == _lib.OK and call(metric=1) == _lib.OK
    for bad in (dict(dd=0), dict(metric=2), dict(nq=-1), dict(nn=-1), dict(cap=-1), dict(nl=-1), dict(n_probe=0), dict(cb=False),
                dict(qp=None), dict(xp=None), dict(vp=None), dict(ip_=None), dict(tp=None), dict(lp=None), dict(op=None), dict(pp=None)):
        assert call(**bad) == _lib.EINVAL, bad
    for bad in (dict(vb=1), dict(dd=16385, q_rs=16385, x_rs=16385), dict(nn=(1 << 32) - 1), dict(n_probe=1 << 24, p_rs=1 << 24)):
        assert call(**bad) == _lib.EUNSUPPORTED, bad
    for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1), dict(p_rs=N_PROBE - 1)):
        assert call(**bad) == _lib.ESHAPE, bad
    assert call(slot=7) == _lib.ENODEV
    assert call(slot=7, n_probe=0) == _lib.EINVAL
    assert call(slot=7, vb=3) == _lib.ENODEV
    assert call(vb=3, pp=None) == _lib.EUNSUPPORTED
    assert call(pp=None, p_rs=1) == _lib.EINVAL
    assert call(cap=0, vp=None, ip_=None) == _lib.OK
    assert call(nn=0, xp=None) == _lib.OK and call(nl=0) == _lib.OK       # all-zero lims
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0, 0, 0]
    ra.launch_log(reset=True)
    lims.fill_(-5)
    assert call(nq=0) == _lib.OK and call(nq=0, qp=None, lp=None, tp=None, op=None, pp=None) == _lib.OK
    torch.cuda.synchronize()
    assert ra.launch_log(reset=True) == "" and lims.cpu().tolist() == [-5, -5, -5]
    assert call() == _lib.OK
    assert ra.launch_log(reset=True) == "k_adc_lists_plan + k_flat_range_lists x2 + k_adc_range_scan"
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK
    torch.cuda.synchronize()
