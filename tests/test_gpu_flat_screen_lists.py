"""GPU tests of the matrix-core range screen in probed lists (pqhip_flat_screen_lists_f32_dev) and its compositions: per
query R_q <= O_q <= S_q, the order (probe slot, position), the slack, the capacity protocol, independence of the options."""
import ctypes

import numpy as np
import pytest

import flat_lists_ref as flr
import flat_range_ref as frr
import flat_screen_ref as fsr
from test_gpu_adc_search_lists import SENT_I, ra  # noqa: F401
from test_gpu_flat_screen import ABS, PAD, case, mixed_thresholds
from test_gpu_rerank import make_pq

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 31, 32, 33, 700, 228)      # tiles start at positions that are no multiples of 32
N = sum(LENGTHS)
OFF = flr.offsets(LENGTHS)
LIST_OF = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
OPTIONS = ("flat_screen_lists_wgs", "flat_screen_lists_unit_rows", "flat_screen_lists_chunk_queries")
X_EXP = 10


def probe_rows(nq, n_probe, seed=3):
    rng = np.random.default_rng(seed)
    pr = np.stack([rng.permutation(len(LENGTHS))[:n_probe] for _ in range(nq)]).astype(np.int64)
    if n_probe > 1:
        pr[::3, -1] = -1
    return pr


def probed_values(values, pr, allow=None):
    out = np.full_like(values, np.nan)
    for i in range(values.shape[0]):
        m = flr.probed_mask(OFF, pr[i], N)[0] & (True if allow is None else allow)
        out[i, m] = values[i, m]
    return out


def run(pq, q, x, pr, thr, ip, off=OFF, words=None, stride=None, check=True, **kw):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if stride is not None:
        big = torch.zeros((x.shape[0], stride), dtype=xd.dtype, device="cuda")
        big[:, :x.shape[1]] = xd
        xd = big[:, :x.shape[1]]
    wd = None if words is None else torch.from_numpy(words).cuda()
    lims, idx = pq.flat_screen_lists_device(qd, xd, torch.from_numpy(np.asarray(off)).cuda(), torch.from_numpy(np.asarray(pr)).cuda(),
                                            torch.from_numpy(np.asarray(thr, np.float32)).cuda(), ip=ip, allow=wd, x_exp=X_EXP,
                                            check=check, **kw)
    return lims.cpu().numpy().tolist(), idx.cpu().numpy()


def check_contract(got, q, x, values, pr, thr, ip, allow=None):
    lims, idx = np.asarray(got[0]), got[1]
    nq = values.shape[0]
    assert lims.shape == (nq + 1,) and lims[0] == 0 and lims[-1] == idx.size
    want = frr.ref_flat_range_lists(q, x, OFF, pr, thr, ip=ip, allow=allow, values=values)
    reg = fsr.regular_rows(x, X_EXP)
    sl = fsr.slack(x, q, X_EXP) + ABS
    v64 = values.astype(np.float64)
    for i in range(nq):
        o = idx[lims[i]:lims[i + 1]]
        slot_of_list = np.full(len(LENGTHS), -1)
        slot_of_list[pr[i][pr[i] >= 0]] = np.flatnonzero(pr[i] >= 0)
        slots = slot_of_list[LIST_OF[o]]
        assert (slots >= 0).all(), "a row of an unprobed list"
        assert (np.diff(slots * N + o) > 0).all(), "probe slot first, then ascending position"
        if allow is not None:
            assert allow[o].all(), "a disallowed row was returned"
        r = want[2][want[0][i]:want[0][i + 1]]
        assert np.isin(r, o).all(), ("a row of the exact result is missing", i, np.setdiff1d(r, o)[:5])
        if np.isfinite(thr[i]) and np.isfinite(q[i]).all():
            rows = o[reg[o]]
            t = float(thr[i])
            ok = (v64[i][rows] >= t - sl[i][rows] / 2) if ip else (v64[i][rows] <= t + sl[i][rows])
            assert ok.all(), ("a regular row beyond the slack", i, rows[~ok][:5])


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("nq,n_probe", [(1, 1), (33, 3), (70, 7)])
@pytest.mark.parametrize("d", [17, 300, 1030])
def test_gpu_flat_screen_lists_is_sound_ordered_and_tight(ra, d, nq, n_probe, half):
    pq = make_pq(ra)
    q, x, values = case(9100 + d, N, d, 70, half)
    q, pr = q[:nq], probe_rows(nq, n_probe)
    for ip in (False, True):
        v = values[ip][:nq]
        thr = mixed_thresholds(probed_values(v, pr), ip)
        check_contract(run(pq, q, x, pr, thr, ip), q, x, v, pr, thr, ip)


@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_screen_lists_tightness(ra, half):
    pq = make_pq(ra)
    q, x, values = case(9100 + 300, N, 300, 70, half)
    pr = probe_rows(70, 3)
    for ip in (False, True):
        pv = probed_values(values[ip], pr)
        probed = np.isfinite(pv).sum(1)
        some = probed >= 100
        thr = np.array([np.sort(v[np.isfinite(v)])[::-1 if ip else 1][20] if s else (np.inf if ip else -np.inf)
                        for v, s in zip(pv, some)], np.float32)
        wl, _ = fsr.widest_screen(q, x, thr, X_EXP, ip, values=np.where(np.isfinite(pv), pv, np.inf if not ip else -np.inf))
        assert (np.diff(wl)[some] < probed[some] / 4).all(), "the seed's widest sound screen already exceeds the cap"
        got = run(pq, q, x, pr, thr, ip)
        check_contract(got, q, x, values[ip], pr, thr, ip)
        assert (np.diff(got[0])[some] >= 21).all() and (np.diff(got[0])[some] < probed[some] / 4).all(), np.diff(got[0]).max()


@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_screen_lists_special_rows_masks_and_strides(ra, half):
    pq = make_pq(ra)
    q, x, values = case(9201, N, 300, 33, half, special=True)      # NaN, +-Inf, an element beyond f16, ties
    pr = probe_rows(33, 7)
    rng = np.random.default_rng(5)
    allow = rng.random(N) < 0.5
    allow[64:160] = False                                           # empty words, also inside the 700-row list
    allow[160:192] = True
    allow[[3, 4, 6, 11, N - 1]] = True
    words = flr.mask_words(allow).copy()
    words[-1] |= np.int32(-2)                                       # bits beyond n
    poisoned = x.copy()
    poisoned[~allow] = np.nan
    for ip in (False, True):
        thr = mixed_thresholds(probed_values(values[ip], pr), ip)
        got = run(pq, q, x, pr, thr, ip)
        check_contract(got, q, x, values[ip], pr, thr, ip)
        for i in range(33):                                         # every list is probed unless the pad took its slot
            o = got[1][got[0][i]:got[0][i + 1]]
            rows = [r for r in ([3, 4, 6] if half else [3, 4, 6, 11]) if LIST_OF[r] in pr[i]]
            assert np.isin(rows, o).all(), i
        odd = run(pq, q, x, pr, thr, ip, stride=301)                # rows at odd element offsets: no wide loads
        assert odd[0] == got[0] and odd[1].tolist() == got[1].tolist()
        thr_m = mixed_thresholds(probed_values(values[ip], pr, allow), ip)
        masked = run(pq, q, x, pr, thr_m, ip, words=words)
        check_contract(masked, q, x, values[ip], pr, thr_m, ip, allow=allow)
        again = run(pq, q, poisoned, pr, thr_m, ip, words=words)    # a disallowed row is not loaded
        assert again[0] == masked[0] and again[1].tolist() == masked[1].tolist()


def test_gpu_flat_screen_lists_bad_ids_repeats_and_offsets(ra):
    """seven times the 700-row list: beyond the budget of stored hit words, the fill pass forms them again"""
    from reductive_amd import PanicError
    pq = make_pq(ra)
    q, x, values = case(9100 + 17, N, 17, 70, False)
    q, v = q[:6], values[False][:6]
    every = np.full(6, np.inf, np.float32)
    pr = np.array([[5, 5, 6], [7, 2, -1], [-2, 4, 4], [5, 1, 0], [6, 6, 6], [3, -1, 99]], np.int64)
    want = frr.ref_flat_range_lists(q, x, OFF, np.where((pr < 0) | (pr > 6), -1, pr), every, values=v)
    got = run(pq, q, x, pr, every, False, check=False)
    assert got[0] == want[0].tolist() and got[1].tolist() == want[2].tolist()
    with pytest.raises(PanicError):                                 # reads the flag the call above raised, and clears it
        run(pq, q, x, pr, every, False)
    seven = np.full((6, 7), 5, np.int64)
    thr = mixed_thresholds(v, False)
    one = run(pq, q, x, seven[:, :1], thr, False)
    got = run(pq, q, x, seven, thr, False)
    assert np.diff(got[0]).tolist() == (7 * np.diff(one[0])).tolist()
    for i in range(6):
        assert got[1][got[0][i]:got[0][i + 1]].tolist() == one[1][one[0][i]:one[0][i + 1]].tolist() * 7
    bad_off = OFF.copy()
    bad_off[7] = N + 500                                            # overlong: clamped to n
    bad_off[2] = 40                                                 # list 1 = [0, 40) overlaps, list 2 = [40, 32) inverted
    pr = probe_rows(6, 7)
    want = frr.ref_flat_range_lists(q, x, bad_off, pr, every, values=v)
    got = run(pq, q, x, pr, every, False, off=bad_off, check=False)
    assert got[0] == want[0].tolist() and got[1].tolist() == want[2].tolist()


def screen_raw(pq, qd, xd, od, pd, td, capacity, null_out=False):
    import torch
    from reductive_amd import _lib
    nq, d = qd.shape
    ibuf = torch.full((capacity + 2 * PAD,), SENT_I, dtype=torch.int64, device="cuda")
    lims = torch.full((nq + 3,), SENT_I, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().pqhip_flat_screen_lists_f32_dev(
        pq._cb(), pq._slot_for(qd), qd.data_ptr(), nq, qd.stride(0), xd.data_ptr(), xd.element_size(), xd.shape[0], d, xd.stride(0),
        None, od.data_ptr(), od.shape[0] - 1, pd.data_ptr(), pd.shape[1], pd.stride(0), 0, X_EXP, td.data_ptr(), lims.data_ptr() + 8,
        None if null_out else ibuf.data_ptr() + 8 * PAD, capacity, stream)
    torch.cuda.synchronize()
    return rc, lims.cpu().numpy(), ibuf.cpu().numpy()


def test_gpu_flat_screen_lists_capacity_protocol_and_status_codes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    q, x, values = case(9100 + 300, N, 300, 70, False)
    q, pr = q[:33], probe_rows(33, 3)
    thr = mixed_thresholds(probed_values(values[False][:33], pr), False)
    full = run(pq, q, x, pr, thr, False)
    total = full[0][-1]
    qd, xd, od, pd, td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, x, OFF, pr, thr))
    for capacity, null_out in ((total + 7, False), (total // 3, False), (1, False), (0, True)):
        rc, lb, ib = screen_raw(pq, qd, xd, od, pd, td, capacity, null_out)
        assert rc == _lib.OK
        assert lb[0] == SENT_I and lb[-1] == SENT_I and lb[1:-1].tolist() == full[0]              # the true counts, always
        m = min(total, capacity)
        assert (ib[:PAD] == SENT_I).all() and (ib[PAD + m:] == SENT_I).all(), "write outside the first `capacity` ids"
        assert ib[PAD:PAD + m].tolist() == full[1][:m].tolist()
    got = run(pq, q, x, pr, thr, False, capacity=5)                 # the wrapper's exact-size retry
    assert got[0] == full[0] and got[1].tolist() == full[1].tolist()
    wide_q, wide_x = torch.zeros(33, 2049, device="cuda"), torch.zeros(N, 2049, device="cuda")
    assert screen_raw(pq, wide_q, wide_x, od, pd, td, 4)[0] == _lib.EUNSUPPORTED


def test_gpu_flat_screen_lists_is_a_function_of_the_inputs_alone(ra):
    pq = make_pq(ra)
    q, x, values = case(9100 + 300, N, 300, 70, True)
    pr = probe_rows(70, 7)
    for ip in (False, True):
        thr = mixed_thresholds(probed_values(values[ip], pr), ip)
        base = run(pq, q, x, pr, thr, ip)
        try:
            for setting in ((0, 64, 0), (1, 0, 0), (3, 64, 0), (0, 0, 32), (3, 32, 1)):   # the 700-row list in 11 units; 3 chunks
                for name, value in zip(OPTIONS, setting):
                    ra.set_option(name, value)
                got = run(pq, q, x, pr, thr, ip)
                assert got[0] == base[0] and got[1].tolist() == base[1].tolist(), setting
        finally:
            for name in OPTIONS:
                ra.set_option(name, 0)
        parts = [run(pq, q[a:b], x, pr[a:b], thr[a:b], ip) for a, b in ((0, 31), (31, 32), (32, 70))]
        assert np.concatenate([p[1] for p in parts]).tolist() == base[1].tolist()
        assert np.concatenate([np.diff(p[0]) for p in parts]).tolist() == np.diff(base[0]).tolist()


def on_gpu(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]

@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d,nq,n_probe", [(17, 33, 3), (300, 70, 7), (1030, 33, 3)])
def test_gpu_flat_lists_batch_compositions_are_bit_for_bit(ra, d, nq, n_probe, half):
    pq = make_pq(ra)
    q, x, values = case(9100 + d, N, d, 70, half)
    q, pr = q[:nq], probe_rows(nq, n_probe)
    allow = np.random.default_rng(9).random(N) < 0.7
    for ip in (False, True):
        for mask in (None, allow):
            qd, xd, od, pd, wd = on_gpu(q, x, OFF, pr, None if mask is None else flr.mask_words(mask))
            thr = mixed_thresholds(probed_values(values[ip][:nq], pr, mask), ip)
            want = frr.ref_flat_range_lists(q, x, OFF, pr, thr, ip=ip, allow=mask, values=values[ip][:nq])
            lims, val, idx = pq.flat_range_lists_batch_device(qd, xd, od, pd, on_gpu(thr)[0], ip=ip, allow=wd, x_exp=X_EXP, check=True)
            assert lims.cpu().numpy().tolist() == want[0].tolist() and idx.cpu().numpy().tolist() == want[2].tolist()
            assert val.cpu().numpy().view(np.int32).tolist() == want[1].view(np.int32).tolist()
            for k in (1, 10, 1024):                                 # 1,024: beyond what any query probes -- the plain call
                stats, (wv, wi, _) = {}, flr.ref_flat_search_lists(q, x, OFF, pr, k, ip=ip, allow=mask)
                gv, gi = pq.flat_search_lists_batch_device(qd, xd, od, pd, k, ip=ip, allow=wd, x_exp=X_EXP, check=True, stats=stats)
                flr.assert_same(gv.cpu().numpy(), gi.cpu().numpy(), wv, wi)
                assert (stats["fallback_queries"] == nq) if k == 1024 else (stats["fallback_queries"] < nq or n_probe < 7), stats


def test_gpu_partitioned_flat_matrix_screen_route_equals_the_plain_one(ra):
    import torch
    from reductive_amd.qmatrix import PartitionedFlatMatrix
    q, x, values = case(9100 + 300, N, 300, 70, False)
    rng = np.random.default_rng(2)
    cent = x[rng.choice(N, 7, replace=False)].astype(np.float32)
    assign = ((x[:, None, :].astype(np.float32) - cent[None]) ** 2).sum(2).argmin(1)
    m = PartitionedFlatMatrix(x, cent, assign)
    allow = rng.random(N) < 0.6
    for ip, topk, rng_call in ((False, m.nearest, m.within), (True, m.most_similar, m.similar_above)):
        t = float(np.quantile(values[ip], 0.9 if ip else 0.1))
        for a in (None, allow):
            plain, fast = (topk(q, 10, 3, allow=a, screen=s) for s in (False, True))
            assert all(torch.equal(u, v) for u, v in zip(plain, fast))
            plain, fast = (rng_call(q, t, 3, allow=a, screen=s) for s in (False, True))
            assert all(torch.equal(u, v) for u, v in zip(plain, fast)) and int(plain[0][-1]) > 0
