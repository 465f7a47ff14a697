"""ADC search over a partitioned code matrix on the GPU (include/pqhip.h: pqhip_adc_search_lists_f32_dev,
pqhip_adc_ip_search_lists_f32_dev): per query the exhaustive search restricted to the rows of the probed lists.
Reference: tests/adc_lists_ref.py (pinned to the exhaustive references by test_adc_lists.py).  Indices exactly, values
bit for bit (NaN as the canonical NaN, similarity zeros as +0), padding, nothing written outside the outputs, the same
result for every number of workgroups per query, bad list ids / offsets reported and never read through, and
qmatrix.PartitionedMatrix on top."""
import ctypes
import io

import numpy as np
import pytest

import synth
from adc_ip_ref import ip_tables, scores
from adc_lists_ref import probed_positions, ref_lists_search
from oracle import pq_oracle as orc

SHAPES = [(15, 256, 20, False), (48, 256, 16, False), (10, 128, 2, False), (3, 7, 5, True)]
OPTION = "adc_lists_wgs_per_query"


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


SENT_V = np.float32(-1234.5)
SENT_I = -777


def search_raw(pq, ip, codes, tables, list_off, probes, k, scales=None, pad=3):
    """The C entry point with row strides k + pad and sentinels around the outputs; checks the sentinels and returns
    (value, idx) as numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n, M = codes.shape
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=codes.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream
    pr = probes if probes.dim() == 2 else probes[None]
    head = (pq._cb(), pq._slot_for(codes), tables.data_ptr(), nq, codes.data_ptr(), codes.element_size(), n,
            codes.stride(0) if n > 1 else max(codes.stride(0), M), list_off.data_ptr(), list_off.shape[0] - 1,
            pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else max(pr.stride(0), pr.shape[1]))
    tail = (k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, ctypes.c_void_p(stream))
    if ip:
        rc = _lib.lib().pqhip_adc_ip_search_lists_f32_dev(*head, scales.data_ptr() if scales is not None else None, *tail)
    else:
        rc = _lib.lib().pqhip_adc_search_lists_f32_dev(*head, *tail)
    assert rc == _lib.OK, rc
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    v = np.stack([vb[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    i = np.stack([ib[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    return v, i


def assert_same(got_v, got_i, want_v, want_i):
    """indices exactly; values bit for bit, NaN as the canonical quiet NaN"""
    got_v = np.asarray(got_v, np.float32)
    want_v = np.asarray(want_v, np.float32)
    assert np.array_equal(got_i, want_i)
    gn, wn = np.isnan(got_v), np.isnan(want_v)
    assert np.array_equal(gn, wn)
    assert (got_v[gn].view(np.uint32) == 0x7fc00000).all()
    assert got_v[~gn].tobytes() == want_v[~wn].tobytes()


def search(pq, ip, cd, t, lo, pr, k, scales=None, check=True):
    if ip:
        return pq.adc_ip_search_lists_device(cd, t, lo, pr, k, scales=scales, check=check)
    return pq.adc_search_lists_device(cd, t, lo, pr, k, check=check)


def check_all(pq, ip, cd, t, lo, pr, values, ks, scales=None):
    """Every k of ks: the Python entry point and the raw one (sentinels) against the reference over `values`."""
    off, probes = lo.cpu().numpy(), pr.cpu().numpy()
    for k in ks:
        want_v, want_i = ref_lists_search(values, off, probes, k, ip=ip)
        v, i = search(pq, ip, cd, t, lo, pr, k, scales=scales)
        if t.dim() == 2:
            assert tuple(v.shape) == (k,) and tuple(i.shape) == (k,)
            v, i = v[None], i[None]
        assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
        assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
        rv, ri = search_raw(pq, ip, cd, t, lo, pr, k, scales=scales)
        assert_same(rv, ri, want_v, want_i)


def make_lists(seed, n, n_lists, empty_every=5):
    """list_off with uneven lists, every empty_every-th one empty"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n + 1, n_lists - 1))
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    for l in range(0, n_lists - 1, empty_every):
        off[l + 1] = off[l]
    return np.maximum.accumulate(off)


def make_probes(seed, nq, n_lists, n_probe):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)


def setup(ra, seed, M, K, dsub, opq, n, nq):
    import torch
    d = M * dsub
    q = synth.normalish(seed, (M, K, dsub))
    P = synth.orthonormal(seed + 1, d) if opq else None
    pq = ra.Pq(P, q)
    yd = torch.from_numpy(synth.normalish(seed + 2, (nq, d))).cuda()
    t_l2 = pq.adc_tables_device(yd)
    t_ip = pq.adc_ip_tables_device(yd)
    assert t_l2.cpu().numpy().tobytes() == orc.adc_tables(q, yd.cpu().numpy(), projection=P).tobytes()
    assert t_ip.cpu().numpy().tobytes() == ip_tables(q, yd.cpu().numpy(), projection=P).tobytes()
    codes = synth.codes_u8(seed + 3, (n, M), K)
    sc = (synth.uniform01(seed + 4, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)   # some negative
    dist = orc.adc_scan(t_l2.cpu().numpy(), codes)
    ipsum = orc.adc_scan(t_ip.cpu().numpy(), codes)
    return pq, t_l2, t_ip, codes, torch.from_numpy(codes).cuda(), sc, torch.from_numpy(sc).cuda(), dist, ipsum


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", SHAPES)
@pytest.mark.parametrize("n,nq,n_lists", [(5003, 5, 13), (120011, 9, 64)])
def test_gpu_lists_search_matches_reference(ra, M, K, dsub, opq, n, nq, n_lists):
    """L2 and IP, with and without scales, k in {1, 10, 64, 65, 1024}, n_probe in {1, 3, n_lists}.  The (3, 7, 5)
    shape has 343 distinct code rows at most: thousands of rows tie and the position decides."""
    import torch
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9400 + M, M, K, dsub, opq, n, nq)
    lo = torch.from_numpy(make_lists(9410 + n, n, n_lists)).cuda()
    ks = (1, 10, 64, 65, 1024)
    for n_probe in (1, 3, n_lists):
        pr = torch.from_numpy(make_probes(9420 + n_probe, nq, n_lists, n_probe)).cuda()
        ra.launch_log(reset=True)
        check_all(pq, False, cd, t_l2, lo, pr, dist, ks)
        log = ra.launch_log(reset=True)
        assert "k_adc_lists_plan" in log and "k_adc_search_lists_u8" in log and "k_adc_search_merge" in log, log
        assert "k_adc_search_u8" not in log and "k_adc_scan" not in log, log
        check_all(pq, True, cd, t_ip, lo, pr, scores(ipsum), ks[:4])
        log = ra.launch_log(reset=True)
        assert "k_adc_ip_search_lists_u8" in log and "k_adc_ip_search_merge" in log, log
        check_all(pq, True, cd, t_ip, lo, pr, scores(ipsum, sc), ks, scales=scd)
    # one query through 2-D tables and a 1-D probe row
    pr1 = torch.from_numpy(make_probes(9430, 1, n_lists, 3)[0]).cuda()
    check_all(pq, False, cd, t_l2[2].contiguous(), lo, pr1, dist[2], (10,))
    check_all(pq, True, cd, t_ip[2].contiguous(), lo, pr1, scores(ipsum[2], sc), (10,), scales=scd)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", [(15, 256, 20, False), (3, 7, 5, True)])
def test_gpu_lists_search_does_not_depend_on_the_grid(ra, M, K, dsub, opq):
    """Forced workgroups per query 1, 2, 7, the CU count, and auto: one result."""
    import torch
    n, nq, n_lists = 90001, 4, 37
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9440 + M, M, K, dsub, opq, n, nq)
    lo = torch.from_numpy(make_lists(9441, n, n_lists)).cuda()
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for g in (1, 2, 7, n_cus, 0):
            ra.set_option(OPTION, g)
            for n_probe in (1, 3, n_lists):
                pr = torch.from_numpy(make_probes(9442 + n_probe, nq, n_lists, n_probe)).cuda()
                check_all(pq, False, cd, t_l2, lo, pr, dist, (1, 65, 1024))
                check_all(pq, True, cd, t_ip, lo, pr, scores(ipsum, sc), (10, 64), scales=scd)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", [(15, 256, 20, False), (3, 7, 5, True)])
def test_gpu_lists_search_is_the_exhaustive_search_of_the_probed_rows(ra, M, K, dsub, opq):
    """On the device: the list search equals adc_search_device / adc_ip_search_device on codes[rows of S_q], indices
    mapped back to positions."""
    import torch
    n, nq, n_lists = 60013, 3, 29
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9450 + M, M, K, dsub, opq, n, nq)
    off = make_lists(9451, n, n_lists)
    lo = torch.from_numpy(off).cuda()
    for n_probe in (1, 3, n_lists):
        probes = make_probes(9452 + n_probe, nq, n_lists, n_probe)
        pr = torch.from_numpy(probes).cuda()
        for k in (1, 10, 1024):
            d, i = pq.adc_search_lists_device(cd, t_l2, lo, pr, k)
            s, j = pq.adc_ip_search_lists_device(cd, t_ip, lo, pr, k, scales=scd)
            for q in range(nq):
                rows = torch.from_numpy(np.sort(probed_positions(off, probes[q], n))).cuda()
                wd, wi = pq.adc_search_device(cd[rows].contiguous(), t_l2[q].contiguous(), k)
                ws, wj = pq.adc_ip_search_device(cd[rows].contiguous(), t_ip[q].contiguous(), k,
                                                 scales=scd[rows].contiguous())
                back = lambda x: torch.where(x < 0, x, rows[x.clamp(min=0)]) if rows.numel() else x
                assert torch.equal(i[q], back(wi)) and torch.equal(j[q], back(wj))
                assert d[q].cpu().numpy().tobytes() == wd.cpu().numpy().tobytes()
                assert s[q].cpu().numpy().tobytes() == ws.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_gpu_lists_search_edges(ra):
    """Empty lists, -1 padding, a probe row of only -1, fewer probed rows than k, no rows, no lists, strided codes and
    a strided probe matrix."""
    import torch
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 40003, 6, 21
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9460, M, K, dsub, False, n, nq)
    off = make_lists(9461, n, n_lists, empty_every=2)
    off[n_lists - 1] = n - 40                              # the last list holds 40 rows
    off = np.maximum.accumulate(np.minimum(off, n))
    off[n_lists - 1] = n - 40
    lo = torch.from_numpy(off).cuda()
    probes = make_probes(9462, nq, n_lists, 6)
    probes[0, [1, 4]] = -1                                 # padding in the middle of a row
    probes[1] = -1                                         # nothing probed: padding only
    probes[2] = [n_lists - 1, -1, -1, -1, -1, -1]          # 40 rows < k
    probes[3] = [0, 2, 4, -1, 6, 8]                        # empty lists only
    assert all(off[l + 1] == off[l] for l in (0, 2, 4, 6, 8))
    pr = torch.from_numpy(probes).cuda()
    check_all(pq, False, cd, t_l2, lo, pr, dist, (1, 64, 1024))
    check_all(pq, True, cd, t_ip, lo, pr, scores(ipsum, sc), (10, 65), scales=scd)
    d, i = pq.adc_search_lists_device(cd, t_l2, lo, pr, 64)
    assert (i[1] == -1).all() and torch.isposinf(d[1]).all() and (i[3] == -1).all()
    assert (i[2, :40] >= n - 40).all() and (i[2, 40:] == -1).all()
    # a probe matrix with a row stride (columns 1 .. 4 of a wider matrix)
    wide = torch.full((nq, 9), 0, dtype=torch.int64, device="cuda")
    wide[:, 1:5] = pr[:, :4]
    check_all(pq, False, cd, t_l2, lo, wide[:, 1:5], dist, (10,))
    # unaligned first row and an odd row stride of the codes
    wc = synth.codes_u8(9463, (n + 3, M + 6), K)
    wcd = torch.from_numpy(wc).cuda()
    for r0, c0 in ((1, 3), (2, 5), (3, 0)):
        view = wcd[r0:r0 + n, c0:c0 + M]
        sub = np.ascontiguousarray(wc[r0:r0 + n, c0:c0 + M])
        check_all(pq, False, view, t_l2, lo, pr, orc.adc_scan(t_l2.cpu().numpy(), sub), (7, 100))
        check_all(pq, True, view, t_ip, lo, pr, scores(orc.adc_scan(t_ip.cpu().numpy(), sub), sc), (7,), scales=scd)
    # n_codes == 0 (every list empty) and n_lists == 0: the padding only
    z = torch.zeros(n_lists + 1, dtype=torch.int64, device="cuda")
    d, i = pq.adc_search_lists_device(cd[:0], t_l2, z, pr, 5, check=True)
    assert (i == -1).all() and torch.isposinf(d).all()
    s, i = pq.adc_ip_search_lists_device(cd[:0], t_ip, z, pr, 5, check=True)
    assert (i == -1).all() and torch.isneginf(s).all()
    pad = torch.full((nq, 2), -1, dtype=torch.int64, device="cuda")
    d, i = pq.adc_search_lists_device(cd, t_l2, z[:1], pad, 5, check=True)
    assert (i == -1).all() and torch.isposinf(d).all()
    s, i = pq.adc_ip_search_lists_device(cd, t_ip, z[:1], pad, 5, scales=scd, check=True)
    assert (i == -1).all() and torch.isneginf(s).all()


@pytest.mark.gpu
def test_gpu_lists_search_reports_bad_ids_and_offsets(ra):
    """A list id outside [0, n_lists) other than -1, an offset past n_codes, a negative offset and an inverted range
    raise the stream's range flag; the call returns what the clamped input defines.  An argument check: the kernel that
    reads the offsets clamps them, no row outside the matrix is formed."""
    import torch
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 20011, 3, 9
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9470, M, K, dsub, False, n, nq)
    off = make_lists(9471, n, n_lists, empty_every=100)
    lo = torch.from_numpy(off).cuda()
    good = make_probes(9472, nq, n_lists, 4)
    cases = []
    bad_id = good.copy()
    bad_id[1, 2] = n_lists                                  # one past the last list
    cases.append((off, bad_id))
    neg_id = good.copy()
    neg_id[0, 0] = -2
    cases.append((off, neg_id))
    past = off.copy()
    past[-1] = n + 100000                                   # the last list runs past the matrix
    cases.append((past, np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))))
    negative = off.copy()
    negative[0] = -5
    cases.append((negative, np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))))
    inverted = off.copy()
    inverted[4] = off[5] + 3 if off[5] + 3 <= n else off[5]
    inverted[5] = off[4]
    cases.append((inverted, np.tile(np.array([4], np.int64), (nq, 1))))
    for o, p in cases:
        od, pd_ = torch.from_numpy(o).cuda(), torch.from_numpy(p).cuda()
        for ip in (False, True):
            t, vals = (t_ip, scores(ipsum, sc)) if ip else (t_l2, dist)
            with pytest.raises(ra.PanicError, match="index out of bounds"):
                search(pq, ip, cd, t, od, pd_, 10, scales=scd if ip else None)
            v, i = search(pq, ip, cd, t, od, pd_, 10, scales=scd if ip else None, check=False)
            want_v, want_i = ref_lists_search(vals, o, p, 10, ip=ip)
            assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            from reductive_amd import _lib
            s = torch.cuda.current_stream().cuda_stream
            assert _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
    search(pq, False, cd, t_l2, lo, torch.from_numpy(good).cuda(), 10)      # flag consumed, good input passes
    # a code >= K inside a probed list is reported as by the exhaustive search
    pq_small = ra.Pq(None, synth.normalish(9473, (M, 200, 4)))
    ts = pq_small.adc_tables_device(torch.from_numpy(synth.normalish(9474, (nq, M * 4))).cuda())
    bad = cd % 200
    pr = torch.from_numpy(good).cuda()
    pq_small.adc_search_lists_device(bad, ts, lo, pr, 10, check=True)
    bad[int(off[good[0, 0]]), 3] = 200
    if off[good[0, 0] + 1] > off[good[0, 0]]:
        with pytest.raises(ra.PanicError, match="index out of bounds"):
            pq_small.adc_search_lists_device(bad, ts, lo, pr, 10, check=True)


@pytest.mark.gpu
def test_gpu_lists_search_status_codes(ra):
    import torch
    from reductive_amd import _lib
    M, K, n, n_lists = 15, 256, 100, 4
    pq = ra.Pq(None, synth.normalish(9480, (M, K, 4)))
    yd = torch.from_numpy(synth.normalish(9481, (2, M * 4))).cuda()
    t = pq.adc_tables_device(yd)
    cd = torch.from_numpy(synth.codes_u8(9482, (n, M), K)).cuda()
    lo = torch.tensor([0, 10, 50, 50, 100], dtype=torch.int64, device="cuda")
    pr = torch.tensor([[0, 1], [2, 3]], dtype=torch.int64, device="cuda")
    for k, want in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        for ip in (False, True):
            with pytest.raises(_lib.PqHipError) as e:
                search(pq, ip, cd, t, lo, pr, k)
            assert e.value.status == want
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")

    def call(ip, slot=0, nq=1, cb=1, nn=n, c_rs=M, off=lo.data_ptr(), nl=n_lists, probes=pr.data_ptr(), n_probe=2, p_rs=2,
             k=10, v_rs=10, i_rs=10):
        head = (pq._cb(), slot, t.data_ptr(), nq, cd.data_ptr(), cb, nn, c_rs, off, nl, probes, n_probe, p_rs)
        tail = (k, out_v.data_ptr(), v_rs, out_i.data_ptr(), i_rs, ctypes.c_void_p(s))
        if ip:
            return L.pqhip_adc_ip_search_lists_f32_dev(*head, None, *tail)
        return L.pqhip_adc_search_lists_f32_dev(*head, *tail)
    for ip in (False, True):
        assert call(ip) == _lib.OK
        assert call(ip, nl=-1) == _lib.EINVAL
        assert call(ip, n_probe=0) == _lib.EINVAL
        assert call(ip, off=None) == _lib.EINVAL
        assert call(ip, probes=None) == _lib.EINVAL
        assert call(ip, slot=7) == _lib.ENODEV
        assert call(ip, slot=7, k=0) == _lib.EINVAL                   # EINVAL before ENODEV
        assert call(ip, cb=4) == _lib.EUNSUPPORTED                    # 1-byte codes only
        assert call(ip, cb=2) == _lib.EUNSUPPORTED
        assert call(ip, cb=4, slot=7) == _lib.ENODEV                  # ENODEV before EUNSUPPORTED
        assert call(ip, cb=4, k=0) == _lib.EINVAL
        assert call(ip, nn=(1 << 32) - 1) == _lib.EUNSUPPORTED        # more rows than 32-bit positions hold
        assert call(ip, p_rs=1) == _lib.ESHAPE
        assert call(ip, v_rs=9) == _lib.ESHAPE
        assert call(ip, i_rs=9) == _lib.ESHAPE
        assert call(ip, c_rs=M - 1) == _lib.ESHAPE
        assert call(ip, k=1025, v_rs=9) == _lib.EUNSUPPORTED          # EUNSUPPORTED before ESHAPE
        assert call(ip, cb=4, p_rs=1) == _lib.EUNSUPPORTED
        torch.cuda.synchronize()
        ra.launch_log(reset=True)
        assert call(ip, nq=0) == _lib.OK                              # n_queries == 0 launches nothing
        assert call(ip, nq=0, off=None, probes=None) == _lib.OK
        assert ra.launch_log(reset=True) == ""
    # a table that does not fit the LDS beside the queues: unsupported, not a silent other path
    big = ra.Pq(None, synth.normalish(9483, (48, 1024, 2)))
    tb = big.adc_tables_device(torch.from_numpy(synth.normalish(9484, (2, 96))).cuda())
    cb48 = torch.from_numpy(synth.codes_u8(9485, (n, 48), 256)).cuda()
    with pytest.raises(_lib.PqHipError) as e:
        big.adc_search_lists_device(cb48, tb, lo, pr, 10)
    assert e.value.status == _lib.EUNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_lists_search_many_probes_and_queries(ra):
    """More probes than one plan pass of 1,024 and more queries than workgroups per query can share CUs: n_lists =
    3,000 short lists, all probed in a shuffled order, 300 queries."""
    import torch
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 50021, 300, 3000
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9490, M, K, dsub, False, n, nq)
    lo = torch.from_numpy(make_lists(9491, n, n_lists, empty_every=3)).cuda()
    pr = torch.from_numpy(make_probes(9492, nq, n_lists, n_lists)).cuda()
    check_all(pq, False, cd, t_l2, lo, pr, dist, (10, 1024))
    pr = torch.from_numpy(make_probes(9493, nq, n_lists, 1500)).cuda()
    check_all(pq, True, cd, t_ip, lo, pr, scores(ipsum, sc), (100,), scales=scd)


def same_up_to_ties(got_v, got_i, want_v, want_i):
    """values bit for bit; ids equal as sets within each group of equal value, the group cut by k left out"""
    assert got_v.tobytes() == want_v.tobytes()
    for q in range(got_v.shape[0]):
        v = want_v[q]
        full = v != v[-1]                                   # the last group may be cut by the k boundary
        for u in np.unique(v[full]):
            g = v == u
            assert sorted(got_i[q][g].tolist()) == sorted(want_i[q][g].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("opq,from_vectors", [(False, True), (True, False), (False, False)])
def test_gpu_partitioned_matrix(ra, opq, from_vectors):
    """partition() from given vectors and from the reconstructions: every row in exactly one list; probes() against
    numpy on the oracle's coarse tables; with nprobe = n_lists the values of nearest / most_similar equal the
    exhaustive search's bit for bit and the ids agree within ties; fewer probes against the reference restricted to the
    probed lists; embeddings() keeps original row numbers."""
    import torch
    from reductive_amd import qmatrix
    from test_gpu_adc_search import ref_search
    M, K, dsub, N, n_lists = 15, 256, 4, 30011, 24
    d = M * dsub
    q = synth.normalish(9500, (M, K, dsub))
    P = synth.orthonormal(9501, d) if opq else None
    pq = ra.Pq(P, q)
    centres = synth.normalish(9502, (40, d)) * np.float32(3.0)
    x = (centres[np.random.default_rng(9503).integers(0, 40, N)] + synth.normalish(9504, (N, d))).astype(np.float32)
    codes = pq.quantize_batch(x)
    norms = synth.uniform01(9505, (N,)) + np.float32(0.5)
    qm = qmatrix.QuantizedMatrix.load(io.BytesIO(qmatrix.dumps(pq, codes, norms)))
    rng = np.random.default_rng(9506)
    pm = qm.partition(n_lists, n_iterations=5, vectors=x if from_vectors else None,
                      train_rows=None if opq else 20000, rng=rng)
    assert len(pm) == N and pm.centroids.shape == (n_lists, d)
    ids, off = pm.ids.cpu().numpy(), pm.list_off.cpu().numpy()
    assert sorted(ids.tolist()) == list(range(N)) and off[0] == 0 and off[-1] == N and (np.diff(off) >= 0).all()
    assert off.size == n_lists + 1 and (np.diff(off) > 0).sum() > 1
    assert np.array_equal(pm.codes.cpu().numpy(), codes[ids]) and np.array_equal(pm.norms.cpu().numpy(), norms[ids])
    # every row sits in the list of its nearest centroid (of the vectors the partition was built from)
    src = x if from_vectors else orc.reconstruct_batch(q, codes, projection=P)
    want_assign = orc.cluster_assignments(pm.centroids, src)
    for l in range(n_lists):
        assert (want_assign[ids[off[l]:off[l + 1]]] == l).all()
        assert (np.diff(ids[off[l]:off[l + 1]]) > 0).all()
    ys = synth.normalish(9507, (5, d)) + centres[:5]
    yd = torch.from_numpy(ys).cuda()
    # probes(): the first lists by (key(dist), id) over the oracle's tables of the one-subquantizer codebook
    coarse = orc.adc_tables(pm.centroids[None], ys)[:, 0, :]
    for nprobe in (1, 3, n_lists, n_lists + 5):
        want = ref_search(coarse, min(nprobe, n_lists))[1]
        assert np.array_equal(pm.probes(yd, nprobe).cpu().numpy(), want)
        assert np.array_equal(pm.probes(yd[1], nprobe).cpu().numpy(), want[1])
    t_l2, t_ip = pq.adc_tables_device(yd), pq.adc_ip_tables_device(yd)
    for k in (1, 10, 200):
        wd, wi = pq.adc_search_device(qm.codes, t_l2, k)
        dd, ii = pm.nearest(yd, k, n_lists)
        same_up_to_ties(dd.cpu().numpy(), ii.cpu().numpy(), wd.cpu().numpy(), wi.cpu().numpy())
        for use_norms in (True, False):
            ws, wj = qm.most_similar(yd, k, use_norms=use_norms)
            ss, jj = pm.most_similar(yd, k, n_lists, use_norms=use_norms)
            same_up_to_ties(ss.cpu().numpy(), jj.cpu().numpy(), ws.cpu().numpy(), wj.cpu().numpy())
    # fewer probes: the reference over the permuted matrix restricted to the probed lists, ids mapped back
    pcodes = codes[ids]
    dist = orc.adc_scan(t_l2.cpu().numpy(), pcodes)
    score = scores(orc.adc_scan(t_ip.cpu().numpy(), pcodes), norms[ids])
    for nprobe in (1, 3):
        probes = pm.probes(yd, nprobe).cpu().numpy()
        for k in (10, 500):
            wv, wp = ref_lists_search(dist, off, probes, k)
            dd, ii = pm.nearest(yd, k, nprobe)
            assert_same(dd.cpu().numpy(), ii.cpu().numpy(), wv, np.where(wp < 0, -1, ids[np.clip(wp, 0, None)]))
            wv, wp = ref_lists_search(score, off, probes, k, ip=True)
            ss, jj = pm.most_similar(yd, k, nprobe)
            assert_same(ss.cpu().numpy(), jj.cpu().numpy(), wv, np.where(wp < 0, -1, ids[np.clip(wp, 0, None)]))
            d1, i1 = pm.nearest(yd[2], k, nprobe)
            assert torch.equal(d1, dd[2]) and torch.equal(i1, ii[2])
    rows = torch.tensor([0, 17, N - 1, 12345], device="cuda")
    assert torch.equal(pm.embeddings(rows), qm.embeddings(rows))
    with pytest.raises(ra.ReductiveError):
        qm.partition(0)
    with pytest.raises(ra.ReductiveError):
        qm.partition(16385)
