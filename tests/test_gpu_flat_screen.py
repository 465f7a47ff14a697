"""GPU tests of the matrix-core range screen (include/pqhip.h: pqhip_flat_screen_f32_dev) through Pq.flat_screen_device
and the raw C entry point.  The screen has no single right answer, so every test checks the contract against
tests/flat_range_ref.py and tests/flat_screen_ref.py: R_q <= O_q <= A (sound), a regular row only within the slack
(tight), ascending ids, the capacity protocol, and that the result depends on neither the grid nor the pass grouping."""
import ctypes
import functools

import numpy as np
import pytest

import flat_range_ref as frr
import flat_screen_ref as fsr
import flat_search_ref as fr
from test_gpu_adc_search_lists import SENT_I, ra  # noqa: F401
from test_gpu_rerank import make_data, make_pq

pytestmark = pytest.mark.gpu
PAD = 5
ABS = 2.0 ** -99        # twice kFlatScreenAbs: what the header adds to the slack


@functools.lru_cache(maxsize=None)
def case(seed, n, d, nq, half, scale=1.0, special=False):
    """(q, x, {ip: values}) computed once and shared; the arrays are not to be written"""
    q, x = make_data(seed, n, d, nq, half)
    if scale != 1.0:
        x = (x.astype(np.float32) * np.float32(scale)).astype(x.dtype)
        q = q * np.float32(scale)
    if special:
        assert n > 140 and d > 69 and nq > 1
        x[17] = x[5]
        x[140] = x[5]
        x[3, 5] = np.nan
        x[4, 6] = np.inf
        x[6, 69] = -np.inf
        x[8] = q[1].astype(x.dtype)
        x[9] = 0
        x[11, 3] = 1e30 if not half else 65504.0
    values = {ip: frr.all_values(q, x, ip) for ip in (False, True)}
    for a in (q, x) + tuple(values.values()):
        a.setflags(write=False)
    return q, x, values


def mixed_thresholds(values, ip, allow=None):
    """query i: a row's own value (the boundary), a selective value, +Inf, -Inf, NaN, the median, in turn"""
    nq = values.shape[0]
    out = np.zeros(nq, np.float32)
    for i in range(nq):
        v = values[i] if allow is None else values[i][allow]
        v = np.sort(v[np.isfinite(v)])
        if v.size == 0:
            continue
        kind = i % 6
        s = v[::-1] if ip else v
        out[i] = (s[min(3, s.size - 1)], s[s.size // 20], np.inf, -np.inf, np.nan, s[s.size // 2])[kind]
    return out


def check_contract(lims, idx, q, x, values, thr, ip, x_exp, allow=None, tight=True):
    """R_q <= O_q <= A, ascending ids and -- on regular rows under finite thresholds -- the tightness cap"""
    nq, n = values.shape
    lims, idx = np.asarray(lims), np.asarray(idx)
    assert lims.shape == (nq + 1,) and lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == idx.size
    want = frr.ref_flat_range(q, x, thr, ip=ip, allow=allow, values=values)
    reg = fsr.regular_rows(x, x_exp)
    sl = fsr.slack(x, q, x_exp) + ABS
    v64 = values.astype(np.float64)
    for i in range(nq):
        o = idx[lims[i]:lims[i + 1]]
        assert (np.diff(o) > 0).all(), "ids ascend"
        assert o.size == 0 or (o[0] >= 0 and o[-1] < n)
        if allow is not None:
            assert allow[o].all(), "a disallowed row was returned"
        r = want[2][want[0][i]:want[0][i + 1]]
        assert np.isin(r, o).all(), ("a row of the exact result is missing", i, np.setdiff1d(r, o)[:5])
        if tight and np.isfinite(thr[i]) and np.isfinite(q[i]).all():
            rows = o[reg[o]]
            t = float(thr[i])
            ok = (v64[i][rows] >= t - sl[i][rows] / 2) if ip else (v64[i][rows] <= t + sl[i][rows])
            assert ok.all(), ("a regular row beyond the slack", i, rows[~ok][:5])


def run(pq, q, x, thr, ip, x_exp, words=None, stride=None, **kw):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if stride is not None:                              # rows vec_row_stride = stride elements apart
        big = torch.zeros((x.shape[0], stride), dtype=xd.dtype, device="cuda")
        big[:, :x.shape[1]] = xd
        xd = big[:, :x.shape[1]]
    wd = None if words is None else torch.from_numpy(words).cuda()
    lims, idx = pq.flat_screen_device(qd, xd, torch.from_numpy(np.asarray(thr, np.float32)).cuda(), ip=ip, allow=wd,
                                      x_exp=x_exp, check=True, **kw)
    assert str(lims.dtype) == "torch.int64" and str(idx.dtype) == "torch.int64"
    return lims.cpu().numpy(), idx.cpu().numpy()


SHAPES = [(1, 1, 1), (31, 7, 31), (33, 16, 32), (1023, 17, 33), (1025, 300, 70), (4100, 16, 70), (4100, 300, 33),
          (1025, 1030, 33), (33, 1030, 70), (4100, 7, 1)]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,d,nq", SHAPES)
def test_gpu_flat_screen_is_sound_and_tight(ra, n, d, nq, half):
    pq = make_pq(ra)
    q, x, values = case(8800 + n + d, n, d, nq, half)
    x_exp = 10
    for ip in (False, True):
        thr = mixed_thresholds(values[ip], ip)
        lims, idx = run(pq, q, x, thr, ip, x_exp)
        check_contract(lims, idx, q, x, values[ip], thr, ip, x_exp)
        for i in range(nq):                             # +Inf / -Inf: every row resp. (for regular rows) none
            o = idx[lims[i]:lims[i + 1]]
            if thr[i] == (-np.inf if ip else np.inf):
                assert o.size == n
            if thr[i] == (np.inf if ip else -np.inf):
                assert o.size == 0


@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_screen_unaligned_rows(ra, half):
    """vec_row_stride = d + 1: rows start at odd element offsets, no 16-byte loads"""
    pq = make_pq(ra)
    for n, d, nq in ((1025, 300, 33), (4100, 17, 32), (33, 1030, 31)):
        q, x, values = case(8800 + n + d, n, d, nq, half)
        for ip in (False, True):
            thr = mixed_thresholds(values[ip], ip)
            got = run(pq, q, x, thr, ip, 10, stride=d + 1)
            check_contract(*got, q, x, values[ip], thr, ip, 10)
            same = run(pq, q, x, thr, ip, 10)
            assert got[0].tolist() == same[0].tolist() and got[1].tolist() == same[1].tolist()


@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_screen_special_rows_are_never_lost(ra, half):
    """ties, NaN, +-Inf, -0, a zero distance and an element beyond f16: whatever the exact call returns is returned, and
    the rows the proof does not cover come back for every query"""
    pq = make_pq(ra)
    q, x, values = case(8901, 1025, 300, 33, half, special=True)
    for ip in (False, True):
        for x_exp in (0, 4):
            thr = mixed_thresholds(values[ip], ip)
            lims, idx = run(pq, q, x, thr, ip, x_exp)
            check_contract(lims, idx, q, x, values[ip], thr, ip, x_exp)
            for i in range(q.shape[0]):
                o = idx[lims[i]:lims[i + 1]]
                assert np.isin([3, 4, 6], o).all(), (i, x_exp)              # NaN, +Inf, -Inf
                if not half or x_exp > 0:
                    assert 11 in o, (i, x_exp)                              # 1e30 resp. 65504 * 2^4: beyond f16
    # a query with a non-finite element returns every row
    qb = q.copy()
    qb[2, 7] = np.inf
    qb[5, 0] = np.nan
    vb = frr.all_values(qb, x, False)
    thr = np.full(qb.shape[0], 1.0, np.float32)
    lims, idx = run(pq, qb, x, thr, False, 0)
    assert lims[3] - lims[2] == x.shape[0] and lims[6] - lims[5] == x.shape[0]
    check_contract(lims, idx, qb, x, vb, thr, False, 0)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("scale_exp", [-6, 0, 6])
def test_gpu_flat_screen_tightness_at_three_scales(ra, scale_exp, half):
    from reductive_amd import pq as rules
    pq = make_pq(ra)
    q, x, values = case(8950 + scale_exp, 4100, 300, 33, half, scale=2.0 ** scale_exp)
    x_exp = rules.flat_screen_x_exp(float(np.abs(x.astype(np.float32)).max()))
    assert fsr.regular_rows(x, x_exp).all()
    for ip in (False, True):
        thr = np.array([np.sort(v)[::-1 if ip else 1][20] for v in values[ip]], np.float32)   # 21 rows per query
        lims, idx = run(pq, q, x, thr, ip, x_exp)
        check_contract(lims, idx, q, x, values[ip], thr, ip, x_exp)
        counts = np.diff(lims)
        assert (counts >= 21).all() and counts.max() < 4100 // 4, counts.max()     # a screen that returns everything fails


def test_gpu_flat_screen_masks(ra):
    """empty words, partial words, bits beyond n; a disallowed row is not loaded (NaN in it changes nothing)"""
    pq = make_pq(ra)
    q, x, values = case(8990, 1025, 17, 33, False)
    rng = np.random.default_rng(5)
    allow = rng.random(1025) < 0.5
    allow[64:160] = False                               # three empty words
    allow[160:192] = True
    allow[1024] = True
    words = fr.mask_words(allow).copy()
    words[-1] |= np.int32(-2)                           # bits beyond n
    poisoned = x.copy()
    poisoned[~allow] = np.nan
    for ip in (False, True):
        thr = mixed_thresholds(values[ip], ip, allow)
        got = run(pq, q, x, thr, ip, 10, words=words)
        check_contract(*got, q, x, values[ip], thr, ip, 10, allow=allow)
        again = run(pq, q, poisoned, thr, ip, 10, words=words)
        assert got[0].tolist() == again[0].tolist() and got[1].tolist() == again[1].tolist()
    none = np.zeros(1025, bool)
    lims, idx = run(pq, q, x, np.full(33, np.inf, np.float32), False, 10, words=fr.mask_words(none))
    assert lims.tolist() == [0] * 34 and idx.size == 0


def screen_raw(pq, qd, xd, td, ip, x_exp, capacity, null_out=False):
    import torch
    from reductive_amd import _lib
    nq, d = qd.shape
    n = xd.shape[0]
    ibuf = torch.full((capacity + 2 * PAD,), SENT_I, dtype=torch.int64, device="cuda")
    lims = torch.full((nq + 3,), SENT_I, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().pqhip_flat_screen_f32_dev(pq._cb(), pq._slot_for(qd), qd.data_ptr(), nq, qd.stride(0), xd.data_ptr(),
                                              xd.element_size(), n, d, xd.stride(0), None, 1 if ip else 0, x_exp, td.data_ptr(),
                                              lims.data_ptr() + 8, None if null_out else ibuf.data_ptr() + 8 * PAD, capacity,
                                              stream)
    torch.cuda.synchronize()
    return rc, lims.cpu().numpy(), ibuf.cpu().numpy()


def test_gpu_flat_screen_capacity_protocol_and_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    q, x, values = case(8800 + 4100 + 300, 4100, 300, 33, False)
    thr = mixed_thresholds(values[False], False)
    full = run(pq, q, x, thr, False, 10)
    total = int(full[0][-1])
    qd, xd, td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, x, thr))
    for capacity, null_out in ((total + 7, False), (total // 3, False), (1, False), (0, True)):
        rc, lb, ib = screen_raw(pq, qd, xd, td, False, 10, capacity, null_out)
        assert rc == _lib.OK
        assert lb[0] == SENT_I and lb[-1] == SENT_I and lb[1:-1].tolist() == full[0].tolist()     # the true counts, always
        m = min(total, capacity)
        assert (ib[:PAD] == SENT_I).all() and (ib[PAD + m:] == SENT_I).all(), "write outside the first `capacity` ids"
        assert ib[PAD:PAD + m].tolist() == full[1][:m].tolist()                                   # a valid prefix
    # the wrapper's count-first protocol and a short first allocation give the same result
    for cap in (0, 5):
        got = run(pq, q, x, thr, False, 10, capacity=cap)
        assert got[0].tolist() == full[0].tolist() and got[1].tolist() == full[1].tolist()
    wide_q, wide_x = torch.zeros(2, 2049, device="cuda"), torch.zeros(3, 2049, device="cuda")
    rc, _, _ = screen_raw(pq, wide_q, wide_x, td, False, 0, 4)
    assert rc == _lib.EUNSUPPORTED
    rc, lb, ib = screen_raw(pq, wide_q[:, :2048].contiguous(), wide_x[:, :2048].contiguous(), td, False, 0, 8)
    assert rc == _lib.OK and lb[1:4].tolist() == [0, 3, 6] and ib[PAD:PAD + 6].tolist() == [0, 1, 2, 0, 1, 2]


def test_gpu_flat_screen_is_a_function_of_the_inputs_alone(ra):
    """the forced grids 1 and 3 and the default give identical output; so does any grouping of the queries into calls
    (passes of 64 and 32 queries, a last pass of 6)"""
    pq = make_pq(ra)
    q, x, values = case(8800 + 4100 + 16, 4100, 16, 70, False)
    for ip in (False, True):
        thr = mixed_thresholds(values[ip], ip)
        base = run(pq, q, x, thr, ip, 10)
        try:
            for g in (1, 3):
                ra.set_option(fsr.OPTION, g)
                got = run(pq, q, x, thr, ip, 10)
                assert got[0].tolist() == base[0].tolist() and got[1].tolist() == base[1].tolist(), g
        finally:
            ra.set_option(fsr.OPTION, 0)
        parts = [run(pq, q[a:b], x, thr[a:b], ip, 10) for a, b in ((0, 31), (31, 32), (32, 70))]
        assert np.concatenate([p[1] for p in parts]).tolist() == base[1].tolist()
        assert np.concatenate([np.diff(p[0]) for p in parts]).tolist() == np.diff(base[0]).tolist()
