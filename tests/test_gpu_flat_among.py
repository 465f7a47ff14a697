"""GPU tests of the exact searches among given rows (include/pqhip.h: pqhip_flat_among_f32_dev,
pqhip_flat_range_among_f32_dev), bit for bit throughout, both metrics, f32 and f16: against tests/flat_among_ref.py, and
device to device against the entry points that define them -- Pq.flat_search_device with the mask of C_q query by query,
Pq.rerank_device where it takes the candidates, Pq.flat_range_device without and with a mask -- through
Pq.flat_among_device / flat_range_among_device and through the raw C entry points with sentinels around the outputs.

Shapes are the smallest at which tiles (16 places), trips (256 places per workgroup), list registers (k 64 / 65, 128 / 129,
1,024) and slices (forced workgroups per query) can go wrong."""
import ctypes

import numpy as np
import pytest

import flat_among_ref as far
import flat_range_ref as frr
import flat_search_ref as fr
from test_gpu_adc_search_lists import SENT_I, SENT_V, ra  # noqa: F401
from test_gpu_flat_range import assert_csr, thresholds
from test_gpu_rerank import make_data, make_pq

PAD = 5
RAGGED = (0, 1, 15, 16, 17, 255, 256, 257, 1024, 1025, 5000, 1, 16, 300, 0, 2000, 17)      # ids per query, 17 queries
KS = (1, 10, 64, 65, 128, 129, 1024)


def dev(*arrays):
    import torch
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    return out[0] if len(out) == 1 else out


def nbits(a):
    """the bits of the values with every NaN as one pattern (the top-k returns the canonical NaN)"""
    a = np.asarray(a.cpu() if hasattr(a, "cpu") else a, np.float32)
    return np.where(np.isnan(a), np.float32(7.0), a).view(np.uint32).tolist()


def same_tensors(a, b):
    import torch
    return all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s,
                           t.view(torch.int32) if t.dtype == torch.float32 else t) for s, t in zip(a, b))


def flag_is_down(pq):
    """reads and lowers the stream's range flag"""
    import torch
    from reductive_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK


def draw_lists(seed, n, lengths, distinct=True):
    """(lims, ids): per query a random list of the given length, distinct rows where asked (and possible)"""
    rng = np.random.default_rng(seed)
    parts = [(rng.permutation(n)[:m] if distinct and m <= n else rng.integers(0, n, m)).astype(np.int64) for m in lengths]
    lims = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return lims, (np.concatenate(parts) if parts else np.zeros(0, np.int64))


def head_args(pq, q, x, ids, lims, n_rows=None, n_ids=None):
    nq, d = q.shape
    n = x.shape[0] if n_rows is None else n_rows
    m = ids.shape[0] if n_ids is None else n_ids
    return (pq._cb(), pq._slot_for(q), q.data_ptr(), nq, q.stride(0) if nq > 1 else max(q.stride(0), d),
            x.data_ptr() if n > 0 else None, x.element_size(), n, d, x.stride(0) if x.shape[0] > 1 else max(x.stride(0), d),
            None if lims is None else lims.data_ptr(), ids.data_ptr() if m > 0 else None, m)


def among_raw(pq, q, x, ids, k, ip, lims=None, n_rows=None, n_ids=None, pad=3):
    """The top-k C entry point on 2-D tensors as they are strided, output row strides k + pad, sentinels around and
    between the output rows; checks the sentinels and returns (value, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq = q.shape[0]
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=q.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=q.device)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    rc = _lib.lib().pqhip_flat_among_f32_dev(*head_args(pq, q, x, ids, lims, n_rows, n_ids), 1 if ip else 0, k,
                                             vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, ctypes.c_void_p(stream))
    assert rc == _lib.OK, rc
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for i in range(nq):
        body[pad + i * rs: pad + i * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    return (np.stack([vb[pad + i * rs: pad + i * rs + k] for i in range(nq)]),
            np.stack([ib[pad + i * rs: pad + i * rs + k] for i in range(nq)]))


def range_among_raw(pq, q, x, ids, thr, ip, capacity, lims=None, null_out=False, n_rows=None, n_ids=None):
    """The range C entry point; d_val / d_idx are `capacity` entries inside buffers with PAD sentinels on either side.
    Checks that nothing outside the first min(total, capacity) entries was written -> (lims, val, idx) as numpy."""
    import torch
    from reductive_amd import _lib
    nq = q.shape[0]
    vbuf = torch.full((capacity + 2 * PAD,), float(SENT_V), dtype=torch.float32, device=q.device)
    ibuf = torch.full((capacity + 2 * PAD,), SENT_I, dtype=torch.int64, device=q.device)
    out_l = torch.full((nq + 3,), SENT_I, dtype=torch.int64, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    rc = _lib.lib().pqhip_flat_range_among_f32_dev(*head_args(pq, q, x, ids, lims, n_rows, n_ids), 1 if ip else 0, thr.data_ptr(),
                                                   out_l.data_ptr() + 8, None if null_out else vbuf.data_ptr() + 4 * PAD,
                                                   None if null_out else ibuf.data_ptr() + 8 * PAD, capacity, stream)
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    lb, vb, ib = out_l.cpu().numpy(), vbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert lb[0] == SENT_I and lb[-1] == SENT_I, "write outside lims"
    m = min(int(lb[nq + 1]), capacity)
    assert (vb[:PAD] == SENT_V).all() and (vb[PAD + m:] == SENT_V).all(), "write outside the values"
    assert (ib[:PAD] == SENT_I).all() and (ib[PAD + m:] == SENT_I).all(), "write outside the indices"
    return lb[1:nq + 2], vb[PAD:PAD + m], ib[PAD:PAD + m]


def query_ids(ids, lims, j):
    return ids if lims is None else ids[lims[j]:lims[j + 1]]


def check_topk(pq, q, x, ids, lims, ks, masked_ks=None, rerank_k=None, metrics=(False, True), xdev=None):
    """every k, both metrics: wrapper and raw call against the reference; for masked_ks, query by query, against
    flat_search_device with the mask of C_q (distinct ids); for rerank_k against rerank_device where a query has at most
    1,024 ids.  xdev: the matrix handed to the device in the place of x."""
    import torch
    qd, xd, idd, ld = dev(q, x if xdev is None else xdev, ids, lims)
    n, nq = x.shape[0], q.shape[0]
    for ip in metrics:
        values = frr.all_values(q, x, ip)
        for k in ks:
            wv, wi, flagged = far.ref_flat_among(q, x, ids, k, lims=lims, ip=ip, values=values)
            assert not flagged
            v, i = pq.flat_among_device(qd, xd, idd, k, lims=ld, ip=ip, check=True)
            assert tuple(v.shape) == (nq, k) and str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
            assert i.cpu().numpy().tolist() == wi.tolist() and nbits(v) == nbits(wv)
            rv, ri = among_raw(pq, qd, xd, idd, k, ip, lims=ld)
            assert ri.tolist() == wi.tolist() and nbits(rv) == nbits(wv)
            for j in range(nq):
                mine = query_ids(ids, lims, j)
                if masked_ks and k in masked_ks and xdev is None:
                    allow = np.zeros(n, bool)
                    allow[mine[mine >= 0]] = True
                    mv, mi = pq.flat_search_device(qd[j], xd, k, ip=ip, allow=dev(fr.mask_words(allow)))
                    assert torch.equal(mi, i[j]) and torch.equal(mv.view(torch.int32), v[j].view(torch.int32)), (ip, k, j)
                if rerank_k == k and 0 < mine.size <= 1024:
                    cv, ci = pq.rerank_device(qd[j], xd, dev(mine), k, ip=ip)
                    assert torch.equal(ci, i[j]) and torch.equal(cv.view(torch.int32), v[j].view(torch.int32)), (ip, k, j)
    assert flag_is_down(pq)


def check_range(pq, q, x, ids, lims, metrics=(False, True), first=0, xdev=None):
    """both metrics, the threshold classes of thresholds() over the NAMED values: wrapper and raw call against the
    reference -> the reference results"""
    qd, xd, idd, ld = dev(q, x if xdev is None else xdev, ids, lims)
    n, nq = x.shape[0], q.shape[0]
    out = []
    for ip in metrics:
        values = frr.all_values(q, x, ip)
        named = np.full(values.shape, np.nan, np.float32)
        for j in range(nq):
            mine = query_ids(ids, lims, j)
            mine = mine[(mine >= 0) & (mine < n)]
            named[j, mine] = values[j, mine]
        thr = thresholds(named, ip, nq, first)
        want = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=values)
        assert not want[3]
        got = pq.flat_range_among_device(qd, xd, idd, dev(thr), lims=ld, ip=ip, check=True)
        assert str(got[0].dtype) == "torch.int64" and str(got[1].dtype) == "torch.float32" and str(got[2].dtype) == "torch.int64"
        assert_csr(got, want[:3])
        assert_csr(range_among_raw(pq, qd, xd, idd, dev(thr), ip, int(want[0][-1]) + 7, lims=ld), want[:3])
        out.append((thr, want))
    assert flag_is_down(pq)
    return out


# ---- widths, row counts, ids per query, queries, k ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300, 4096, 16384])
def test_gpu_flat_among_widths(ra, d, half):
    pq = make_pq(ra)
    n = 1025 if d <= 300 else 300 if d == 4096 else 40
    q, x = make_data(7100 + d, n, d, 3, half)
    x[17] = x[5]                                      # ties
    x[n - 1] = x[n - 9]
    lims, ids = draw_lists(7101 + d, n, (min(n, 257), 0, n))
    ids[lims[2]:lims[3]][::9] = -1
    check_topk(pq, q, x, ids, lims, (1, 10, 129), masked_ks=(10,), rerank_k=129)
    check_range(pq, q, x, ids, lims, first=2)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_among_ragged_lists_every_k(ra, half):
    """17 queries whose lists mix every length at which a tile, a trip or the re-ranking's limit ends"""
    pq = make_pq(ra)
    n = 5000
    q, x = make_data(7200, n, 65, len(RAGGED), half)
    x[4000] = x[3]
    x[77, 5] = np.nan
    x[78, 6] = np.inf
    lims, ids = draw_lists(7201, n, RAGGED)
    check_topk(pq, q, x, ids, lims, KS, masked_ks=(10, 1024), rerank_k=64)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_among_ragged_lists(ra, half):
    """the same lists, ascending: per query the masked exhaustive range call with the mask of C_q"""
    pq = make_pq(ra)
    n = 5000
    q, x = make_data(7300, n, 65, len(RAGGED), half)
    x[77, 5] = np.nan
    lims, ids = draw_lists(7301, n, RAGGED)
    for j in range(len(RAGGED)):
        ids[lims[j]:lims[j + 1]].sort()
    qd, xd, idd, ld = dev(q, x, ids, lims)
    for ip, (thr, want) in zip((False, True), check_range(pq, q, x, ids, lims)):
        got = pq.flat_range_among_device(qd, xd, idd, dev(thr), lims=ld, ip=ip)
        for j in range(len(RAGGED)):
            allow = np.zeros(n, bool)
            allow[ids[lims[j]:lims[j + 1]]] = True
            m = pq.flat_range_device(qd[j], xd, float(thr[j]), ip=ip, allow=dev(fr.mask_words(allow)))
            a, b = int(got[0][j]), int(got[0][j + 1])
            assert int(m[0][1]) == b - a and same_tensors((got[1][a:b], got[2][a:b]), m[1:]), (ip, j)
        assert int(got[0][-1]) > 500                    # the cases are not trivial


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17])
def test_gpu_flat_among_small_matrices(ra, n):
    """fewer rows than a tile: every list beyond n rows names rows twice"""
    pq = make_pq(ra)
    q, x = make_data(7400 + n, n, 20, 3, half=(n == 17))
    lims, ids = draw_lists(7401 + n, n, (0, 1, 300), distinct=False)
    ids[lims[2]:lims[3]][::5] = -1
    check_topk(pq, q, x, ids, lims, (1, 10, 65))
    check_range(pq, q, x, ids, lims, first=1)


@pytest.mark.gpu
def test_gpu_flat_among_one_query_and_the_shared_list(ra):
    """a 1-D query gives 1-D outputs; a shared list (lims None) is the CSR that repeats it, in any order of the ids"""
    pq = make_pq(ra)
    n, d = 1025, 65
    q, x = make_data(7500, n, d, 3)
    rng = np.random.default_rng(7501)
    ids = rng.permutation(n)[:1000].astype(np.int64)
    ids[::13] = -1
    check_topk(pq, q, x, ids, None, (10, 1024), masked_ks=(10, 1024), rerank_k=1024)
    check_range(pq, q, x, ids, None, first=2)
    qd, xd, idd = dev(q, x, ids)
    rep_l, rep = dev(np.arange(4, dtype=np.int64) * ids.size, np.tile(ids, 3))
    shuffled = dev(rng.permutation(ids))
    for ip in (False, True):
        a = pq.flat_among_device(qd, xd, idd, 64, ip=ip)
        assert same_tensors(a, pq.flat_among_device(qd, xd, rep, 64, lims=rep_l, ip=ip))
        assert same_tensors(a, pq.flat_among_device(qd, xd, shuffled, 64, ip=ip))          # the order of the ids
        one = pq.flat_among_device(qd[1], xd, idd, 64, ip=ip, check=True)
        assert tuple(one[0].shape) == (64,) and same_tensors(one, (a[0][1], a[1][1]))
        t = float(np.median(frr.all_values(q[1:2], x, ip)))
        r = pq.flat_range_among_device(qd, xd, idd, t, ip=ip)
        assert same_tensors(r, pq.flat_range_among_device(qd, xd, rep, t, lims=rep_l, ip=ip)) and int(r[0][-1]) > 100
        r1 = pq.flat_range_among_device(qd[1], xd, idd, t, ip=ip, check=True)
        assert tuple(r1[0].shape) == (2,)
        a0, b0 = int(r[0][1]), int(r[0][2])
        assert int(r1[0][1]) == b0 - a0 and same_tensors(r1[1:], (r[1][a0:b0], r[2][a0:b0]))


@pytest.mark.gpu
def test_gpu_flat_among_does_not_depend_on_the_workgroups_per_query(ra):
    pq = make_pq(ra)
    n = 5000
    q, x = make_data(7600, n, 65, 3)
    lims, ids = draw_lists(7601, n, (5000, 257, 1025))
    qd, xd, idd, ld = dev(q, x, ids, lims)
    try:
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            thr = np.array([np.median(values[j][query_ids(ids, lims, j)]) for j in range(3)], np.float32)
            want_r = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=values)
            first = {}
            for g in (0, 1, 2, 3, 5):
                ra.set_option(far.OPTION, g)
                ra.set_option(far.OPTION_RANGE, g)
                for k in (10, 129):
                    wv, wi, _ = far.ref_flat_among(q, x, ids, k, lims=lims, ip=ip, values=values)
                    rv, ri = among_raw(pq, qd, xd, idd, k, ip, lims=ld)
                    assert ri.tolist() == wi.tolist() and nbits(rv) == nbits(wv)
                    assert first.setdefault(k, (rv.tobytes(), ri.tobytes())) == (rv.tobytes(), ri.tobytes())
                got = range_among_raw(pq, qd, xd, idd, dev(thr), ip, int(want_r[0][-1]) + 2, lims=ld)
                assert_csr(got, want_r[:3])
                blob = tuple(a.tobytes() for a in got)
                assert first.setdefault("range", blob) == blob
    finally:
        ra.set_option(far.OPTION, 0)
        ra.set_option(far.OPTION_RANGE, 0)


# ---- the range call against the calls that define it ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_range_among_all_rows_is_the_unmasked_range(ra, half):
    """ids = 0 .. n - 1 shared: pqhip_flat_range_f32_dev without a mask, byte for byte; and the (lims, idx) of that call at
    a wider threshold fed back at the narrow one is that call at the narrow one"""
    import torch
    pq = make_pq(ra)
    n = 1025
    q, x = make_data(7700, n, 65, 5, half)
    x[3, 7] = np.nan
    qd, xd = dev(q, x)
    every = torch.arange(n, dtype=torch.int64, device="cuda")
    for ip in (False, True):
        values = frr.all_values(q, x, ip)
        thr = thresholds(values, ip, 5)               # NaN, +-Inf, nothing, a row's own value, a median
        td = dev(thr)
        want = pq.flat_range_device(qd, xd, td, ip=ip)
        assert same_tensors(pq.flat_range_among_device(qd, xd, every, td, ip=ip, check=True), want)
        assert int(want[0][-1]) > n
        finite = np.isfinite(thr)
        wide_thr = np.where(finite, thr - 30 if ip else 2 * thr, thr).astype(np.float32)      # L2: the result at 2 r
        wide = pq.flat_range_device(qd, xd, dev(wide_thr), ip=ip)
        assert int(wide[0][-1]) > int(want[0][-1])
        assert same_tensors(pq.flat_range_among_device(qd, xd, wide[2], td, lims=wide[0], ip=ip, check=True), want)


@pytest.mark.gpu
def test_gpu_flat_range_among_permuted_and_duplicated_ids_come_back_as_named(ra):
    pq = make_pq(ra)
    n = 1025
    q, x = make_data(7800, n, 65, 5)
    x[3, 7] = np.nan
    rng = np.random.default_rng(7801)
    lims, ids = draw_lists(7801, n, (1025, 17, 600, 0, 256))
    ids[lims[2]:lims[3]] = rng.integers(0, 40, 600)                 # every row many times
    ids[lims[0]:lims[1]][::4] = -1
    wants = check_range(pq, q, x, ids, lims, first=4)          # query 0 a median, query 2 +-Inf
    for ip, (thr, want) in zip((False, True), wants):
        seg = want[2][want[0][2]:want[0][3]]
        assert seg.size > np.unique(seg).size > 1                   # duplicates were returned
        assert (np.diff(want[2][want[0][0]:want[0][1]]) < 0).any()   # not ascending: the order named


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True])
def test_gpu_flat_range_among_capacity(ra, ip):
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    n = 1025
    q, x = make_data(7900, n, 20, 6, half=ip)
    lims, ids = draw_lists(7901, n, (300, 0, 1025, 17, 256, 40))
    values = frr.all_values(q, x, ip)
    thr = np.array([np.median(values[j]) for j in range(6)], np.float32)
    want = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=values)
    total = int(want[0][-1])
    assert total > 300
    qd, xd, idd, ld, td = dev(q, x, ids, lims, thr)
    ra.launch_log(reset=True)
    out_l, val, idx = range_among_raw(pq, qd, xd, idd, td, ip, 0, lims=ld, null_out=True)     # a count call launches no fill
    assert out_l.tolist() == want[0].tolist()
    name = "k_flat_ip_range_among" if ip else "k_flat_range_among"
    assert ra.launch_log(reset=True) == "%s + k_adc_range_scan" % name
    for cap in (total - 1, 13, total, total + 100):
        got = range_among_raw(pq, qd, xd, idd, td, ip, cap, lims=ld)
        assert got[1].size == min(cap, total)
        assert_csr(got, want[:3], prefix=cap)
    ra.launch_log(reset=True)
    assert_csr(pq.flat_range_among_device(qd, xd, idd, td, lims=ld, ip=ip), want[:3])
    assert ra.launch_log(reset=True) == "%s x3 + k_adc_range_scan x2" % name                   # count call, then the sized call


# ---- safety ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_among_rows_that_are_not_named_are_not_read(ra, half):
    pq = make_pq(ra)
    n = 1025
    q, x = make_data(8000, n, 65, 3, half)
    rng = np.random.default_rng(8001)
    ids = rng.permutation(n)[:300].astype(np.int64)
    poisoned = x.copy()
    unnamed = np.ones(n, bool)
    unnamed[ids] = False
    poisoned[unnamed] = np.nan
    lims = np.array([0, 100, 100, 300], np.int64)
    check_topk(pq, q, x, ids, None, (10, 129), xdev=poisoned)
    check_range(pq, q, x, ids, None, first=1, xdev=poisoned)
    # per-query lists: what another query names is not read either -- the values of query 0 do not see rows 100 ..
    p0 = x.copy()
    p0[ids[100:]] = np.nan
    qd, xd, pd0, idd, ld = dev(q, x, p0, ids, lims)
    for ip in (False, True):
        a = pq.flat_among_device(qd[:1], xd, idd, 129, lims=ld[:2], ip=ip)
        assert same_tensors(a, pq.flat_among_device(qd[:1], pd0, idd, 129, lims=ld[:2], ip=ip))
        inf = float("-inf") if ip else float("inf")
        r = pq.flat_range_among_device(qd[:1], pd0, idd, inf, lims=ld[:2], ip=ip)
        assert int(r[0][1]) == 100 and r[2].cpu().tolist() == ids[:100].tolist()


@pytest.mark.gpu
def test_gpu_flat_among_bad_ids_and_lims_raise_the_flag_and_are_skipped(ra):
    pq = make_pq(ra)
    n = 1025
    q, x = make_data(8100, n, 20, 3)
    PanicError = ra.PanicError
    lims, ids = draw_lists(8101, n, (300, 17, 256))
    qd, xd = dev(q, x)

    def both(ids_, lims_, flagged):
        idd, ld = dev(ids_, lims_)
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            wv, wi, f = far.ref_flat_among(q, x, ids_, 65, lims=lims_, ip=ip, values=values)
            inf = np.float32(-np.inf if ip else np.inf)
            wr = far.ref_flat_range_among(q, x, ids_, inf, lims=lims_, ip=ip, values=values)
            assert f == flagged and wr[3] == flagged
            for call, check in ((lambda **kw: pq.flat_among_device(qd, xd, idd, 65, lims=ld, ip=ip, **kw),
                                 lambda got: got[1].cpu().numpy().tolist() == wi.tolist() and nbits(got[0]) == nbits(wv)),
                                (lambda **kw: pq.flat_range_among_device(qd, xd, idd, float(inf), lims=ld, ip=ip, **kw),
                                 lambda got: assert_csr(got, wr[:3]) is None)):
                if flagged:
                    with pytest.raises(PanicError):
                        call(check=True)
                    assert check(call())
                    assert not flag_is_down(pq)
                else:
                    assert check(call(check=True))
        assert flag_is_down(pq)

    padded = ids.copy()
    padded[[0, 5, 299, 300, 316, 400]] = -1
    both(padded, lims, False)                                         # -1 raises nothing
    for bad in (-2, n, 1 << 62, -(1 << 63)):
        b = ids.copy()
        b[310] = bad                                                  # in the 17-id list of query 1
        both(b, lims, True)
    for bad_lims in ([-3, 300, 317, 573], [0, 300, 317, 9000], [0, 317, 300, 573], [600, 700, 800, 900], [0, 300, 1 << 62, 573]):
        both(ids, np.array(bad_lims, np.int64), True)
    both(ids, np.array([0, 300, 300, 573], np.int64), False)          # an empty range is legal


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gpu_flat_among_respects_strides_and_unaligned_bases(ra, half):
    """vectors and queries as column slices of wider tensors whose first element is one element into the allocation: no
    copy is made, rows start at odd multiples of the element size; the ids start one element into theirs; the outputs of
    the raw call are wider than k"""
    import torch
    pq = make_pq(ra)
    n, d, nq = 1234, 77, 3
    q, x = make_data(8200, n, d + 4, nq, half)
    xbuf = torch.zeros(n * (d + 4) + 1, dtype=torch.float16 if half else torch.float32, device="cuda")
    xbuf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xd = xbuf[1:].view(n, d + 4)[:, 2:2 + d]
    qbuf = torch.zeros(nq * (d + 4) + 1, dtype=torch.float32, device="cuda")
    qbuf[1:] = torch.from_numpy(q).cuda().reshape(-1)
    qd = qbuf[1:].view(nq, d + 4)[:, :d]
    assert not xd.is_contiguous() and not qd.is_contiguous()
    assert xd.data_ptr() % (2 * xd.element_size()) != 0 and xd.stride(0) == d + 4
    qs, xs = np.ascontiguousarray(q[:, :d]), np.ascontiguousarray(x[:, 2:2 + d])
    lims, ids = draw_lists(8201, n, (257, 1234, 16))
    ibuf = torch.full((ids.size + 2,), 1 << 40, dtype=torch.int64, device="cuda")             # guards: ids out of range
    ibuf[1:-1] = torch.from_numpy(ids).cuda()
    idd, ld = ibuf[1:-1], dev(lims)
    for ip in (False, True):
        values = frr.all_values(qs, xs, ip)
        for k in (3, 64):
            wv, wi, _ = far.ref_flat_among(qs, xs, ids, k, lims=lims, ip=ip, values=values)
            v, i = pq.flat_among_device(qd, xd, idd, k, lims=ld, ip=ip, check=True)
            assert i.cpu().numpy().tolist() == wi.tolist() and nbits(v) == nbits(wv)
            rv, ri = among_raw(pq, qd, xd, idd, k, ip, lims=ld, pad=7)
            assert ri.tolist() == wi.tolist() and nbits(rv) == nbits(wv)
        thr = np.array([np.median(values[j]) for j in range(nq)], np.float32)
        want = far.ref_flat_range_among(qs, xs, ids, thr, lims=lims, ip=ip, values=values)
        assert_csr(pq.flat_range_among_device(qd, xd, idd, dev(thr), lims=ld, ip=ip, check=True), want[:3])
        assert_csr(range_among_raw(pq, qd, xd, idd, dev(thr), ip, int(want[0][-1]), lims=ld), want[:3])
    assert flag_is_down(pq)


# ---- status codes, degenerate sizes, the launch log ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_flat_among_status_codes_and_degenerate_sizes(ra):
    import torch
    from reductive_amd import _lib
    pq = make_pq(ra)
    d, n, k = 20, 300, 4
    q, x = make_data(8300, n, d, 2)
    lims, ids = draw_lists(8301, n, (40, 17))
    qd, xd, idd, ld = dev(q, x, ids, lims)
    td = torch.full((2,), float("inf"), dtype=torch.float32, device="cuda")
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.full((2000,), 5.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((2000,), 5, dtype=torch.int64, device="cuda")
    out_l = torch.full((3,), -5, dtype=torch.int64, device="cuda")

    def head(slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, lp, ip_, n_ids, metric, cb):
        return (pq._cb() if cb else None, slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, lp, ip_, n_ids, metric)

    def topk(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, lp=ld.data_ptr(),
             ip_=idd.data_ptr(), n_ids=57, metric=0, kk=k, vp=out_v.data_ptr(), v_rs=k, op=out_i.data_ptr(), i_rs=k, cb=True):
        return L.pqhip_flat_among_f32_dev(*head(slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, lp, ip_, n_ids, metric, cb), kk, vp, v_rs,
                                          op, i_rs, ctypes.c_void_p(s))

    def rng(slot=0, qp=qd.data_ptr(), nq=2, q_rs=d, xp=xd.data_ptr(), vb=4, nn=n, dd=d, x_rs=d, lp=ld.data_ptr(),
            ip_=idd.data_ptr(), n_ids=57, metric=0, tp=td.data_ptr(), olp=out_l.data_ptr(), vp=out_v.data_ptr(),
            op=out_i.data_ptr(), cap=2000, cb=True):
        return L.pqhip_flat_range_among_f32_dev(*head(slot, qp, nq, q_rs, xp, vb, nn, dd, x_rs, lp, ip_, n_ids, metric, cb), tp, olp,
                                                vp, op, cap, ctypes.c_void_p(s))

    for call in (topk, rng):
        assert call() == _lib.OK and call(metric=1) == _lib.OK and call(lp=None) == _lib.OK and call(vb=2, x_rs=2 * d) == _lib.OK
        for bad in (dict(dd=0), dict(metric=2), dict(nq=-1), dict(nn=-1), dict(n_ids=-1), dict(cb=False), dict(qp=None),
                    dict(xp=None), dict(ip_=None), dict(vp=None), dict(op=None)):
            assert call(**bad) == _lib.EINVAL, bad
        for bad in (dict(vb=1), dict(vb=8), dict(dd=16385, q_rs=16385, x_rs=16385), dict(nn=(1 << 32) - 1)):
            assert call(**bad) == _lib.EUNSUPPORTED, bad
        for bad in (dict(q_rs=d - 1), dict(x_rs=d - 1)):
            assert call(**bad) == _lib.ESHAPE, bad
        # the precedence: EINVAL, ENODEV, EUNSUPPORTED, null pointers, ESHAPE
        assert call(slot=7) == _lib.ENODEV and call(slot=-1) == _lib.ENODEV
        assert call(slot=7, dd=0) == _lib.EINVAL
        assert call(slot=7, vb=3) == _lib.ENODEV
        assert call(vb=3, qp=None) == _lib.EUNSUPPORTED
        assert call(qp=None, q_rs=1) == _lib.EINVAL
        assert call(nn=0, xp=None, x_rs=0) == _lib.OK                # no rows: the padding resp. all-zero lims, and the flag
        assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
        assert call(n_ids=0, ip_=None) == _lib.OK
        assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK
    for bad in (dict(kk=0), dict(kk=-1)):
        assert topk(**bad) == _lib.EINVAL, bad
    assert topk(kk=1025, v_rs=1025, i_rs=1025) == _lib.EUNSUPPORTED and topk(kk=1025, slot=7) == _lib.ENODEV
    assert topk(v_rs=k - 1) == _lib.ESHAPE and topk(i_rs=k - 1) == _lib.ESHAPE and topk(v_rs=k - 1, vp=None) == _lib.EINVAL
    assert rng(cap=-1) == _lib.EINVAL and rng(tp=None) == _lib.EINVAL and rng(olp=None) == _lib.EINVAL
    assert rng(cap=0, vp=None, op=None) == _lib.OK
    # degenerate sizes: only padding ids on an empty matrix raise nothing
    minus = torch.full((57,), -1, dtype=torch.int64, device="cuda")
    assert topk(nn=0, xp=None, ip_=minus.data_ptr()) == _lib.OK and rng(nn=0, xp=None, ip_=minus.data_ptr()) == _lib.OK
    assert L.pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.OK
    assert out_l.cpu().tolist() == [0, 0, 0]
    assert out_i[:2 * k].cpu().tolist() == [-1] * (2 * k) and torch.isinf(out_v[:2 * k]).all()
    assert topk(n_ids=0, ip_=None, metric=1) == _lib.OK and rng(n_ids=0, ip_=None) == _lib.OK
    torch.cuda.synchronize()
    assert out_l.cpu().tolist() == [0, 0, 0] and (out_v[:2 * k] == float("-inf")).all()
    # no query: nothing is launched or written
    ra.launch_log(reset=True)
    out_l.fill_(-5)
    out_i.fill_(5)
    for call in (topk, rng):
        assert call(nq=0) == _lib.OK and call(nq=0, qp=None, xp=None, ip_=None, vp=None, op=None, lp=None) == _lib.OK
    assert rng(nq=0, tp=None, olp=None) == _lib.OK
    torch.cuda.synchronize()
    assert ra.launch_log(reset=True) == "" and out_l.cpu().tolist() == [-5, -5, -5] and (out_i == 5).all()


@pytest.mark.gpu
def test_gpu_flat_among_launch_log_names_the_new_kernels_and_nothing_else_new(ra):
    import torch
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    q, x = make_data(8400, 300, 20, 2)
    lims, ids = draw_lists(8401, 300, (40, 17))
    qd, xd, idd, ld = dev(q, x, ids, lims)
    for half in (False, True):
        xv = xd.half() if half else xd
        for ip, infix in ((False, ""), (True, "ip_")):
            ra.launch_log(reset=True)
            pq.flat_among_device(qd, xv, idd, 10, lims=ld, ip=ip)
            assert ra.launch_log(reset=True) == "k_flat_%samong + k_adc_%ssearch_merge" % (infix, infix)
            pq.flat_among_device(qd, xv, idd[:0], 10, ip=ip)
            assert ra.launch_log(reset=True) == "k_adc_%ssearch_merge" % infix                 # the padding only
            pq.flat_range_among_device(qd, xv, idd, float("-inf") if ip else float("inf"), lims=ld, ip=ip)
            assert ra.launch_log(reset=True) == "k_flat_%srange_among x3 + k_adc_range_scan x2" % infix
            pq.flat_range_among_device(qd, xv, idd, float("nan"), lims=ld, ip=ip)              # nothing qualifies: no fill
            assert ra.launch_log(reset=True) == "k_flat_%srange_among + k_adc_range_scan" % infix
            pq.flat_range_among_device(qd, xv, idd[:0], 1.0, ip=ip)
            assert ra.launch_log(reset=True) == ""
    torch.cuda.synchronize()


# ---- query chunks past the first ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_flat_among_query_chunks_past_the_first(ra):
    """the grid option at its cap and k = 1,024 leave 10 queries to a chunk (512 MB of partial lists): 25 queries are two
    full chunks and a shorter third, with lists and results that differ per query"""
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    cap = far.grid_caps()[0]
    nq, k, n = 25, 1024, 300
    assert far.topk_chunk(nq, cap, k) == 10 and -(-nq // far.topk_chunk(nq, cap, k)) == 3
    q, x = make_data(8500, n, 20, nq)
    lims, ids = draw_lists(8501, n, [5 + 7 * j for j in range(nq)])
    qd, xd, idd, ld = dev(q, x, ids, lims)
    try:
        ra.set_option(far.OPTION, cap)
        for ip in (False, True):
            wv, wi, _ = far.ref_flat_among(q, x, ids, k, lims=lims, ip=ip)
            ra.launch_log(reset=True)
            rv, ri = among_raw(pq, qd, xd, idd, k, ip, lims=ld)
            infix = "ip_" if ip else ""
            assert ra.launch_log(reset=True) == "k_flat_%samong x3 + k_adc_%ssearch_merge x3" % (infix, infix)
            assert ri.tolist() == wi.tolist() and nbits(rv) == nbits(wv)
            assert len({tuple(r) for r in ri.tolist()}) == nq
    finally:
        ra.set_option(far.OPTION, 0)


@pytest.mark.gpu
def test_gpu_flat_range_among_query_chunks_past_the_first(ra):
    """the grid option at its cap leaves 16 queries to a chunk (one scan sums 2^20 counts): 37 queries are two full chunks
    and a shorter third, with thresholds, lists and results that differ per query"""
    pq = make_pq(ra)
    pq._cb()                                          # the codebook's own launches stay out of the log
    cap = far.grid_caps()[1]
    nq, n = 37, 300
    lengths = [20 + 3 * j for j in range(nq)]
    assert far.range_chunk(nq, sum(lengths), cap, False) == 16 and far.range_chunk(nq, 120, cap, True) == 16
    q, x = make_data(8600, n, 20, nq)
    lims, ids = draw_lists(8601, n, lengths)
    qd, xd, idd, ld = dev(q, x, ids, lims)
    try:
        ra.set_option(far.OPTION_RANGE, cap)
        for ip in (False, True):
            values = frr.all_values(q, x, ip)
            thr = np.array([np.sort(values[j][query_ids(ids, lims, j)])[::-1 if ip else 1][3 + j // 2] for j in range(nq)], np.float32)
            want = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=values)
            counts = np.diff(want[0])
            assert counts.min() >= 4 and len(set(counts.tolist())) > 10 and len(set(thr.tolist())) == nq
            name = "k_flat_ip_range_among" if ip else "k_flat_range_among"
            ra.launch_log(reset=True)
            got = range_among_raw(pq, qd, xd, idd, dev(thr), ip, int(want[0][-1]) + 3, lims=ld)
            assert ra.launch_log(reset=True) == "%s x6 + k_adc_range_scan x3" % name
            assert_csr(got, want[:3])
            shared = far.ref_flat_range_among(q, x, ids[:120], thr, ip=ip, values=values)       # the shared list in chunks
            ra.launch_log(reset=True)
            assert_csr(range_among_raw(pq, qd, xd, idd[:120], dev(thr), ip, int(shared[0][-1])), shared[:3])
            assert ra.launch_log(reset=True) == "%s x6 + k_adc_range_scan x3" % name
    finally:
        ra.set_option(far.OPTION_RANGE, 0)
