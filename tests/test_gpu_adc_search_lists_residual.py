"""ADC list searches over residual codes on the GPU (include/pqhip.h: pqhip_adc_search_lists_residual_f32_dev,
pqhip_adc_ip_search_lists_residual_f32_dev) and qmatrix.ResidualPartitionedMatrix on top.  Reference:
tests/adc_residual_ref.py (pinned by test_adc_residual.py).  Indices exactly, values bit for bit (NaN as the canonical
NaN, zeros as +0), padding, nothing written outside the outputs, one result for every number of workgroups per query,
bad list ids / offsets reported and never read through, the bias of a skipped probe never surfacing.  Shapes, list and
probe generators and the comparison are those of test_gpu_adc_search_lists.py."""
import ctypes
import io

import numpy as np
import pytest

import synth
from adc_ip_ref import ip_tables
from adc_residual_ref import ref_residual_search, scan
from oracle import pq_oracle as orc
from test_gpu_adc_search_lists import OPTION, SENT_I, SENT_V, SHAPES, assert_same, make_lists, make_probes, ra, setup  # noqa: F401


def search_raw(pq, ip, codes, tables, list_off, probes, bias, k, extra=None, pad=3):
    """The C entry point with row strides k + pad and sentinels around the outputs; checks the sentinels and returns
    (value, idx) as numpy [nq, k].  extra: the row terms (distance) or the scales / None (similarity)."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n, M = codes.shape
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=codes.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream
    pr = probes if probes.dim() == 2 else probes[None]
    pb = bias if bias.dim() == 2 else bias[None]
    head = (pq._cb(), pq._slot_for(codes), tables.data_ptr(), nq, codes.data_ptr(), codes.element_size(), n,
            codes.stride(0) if n > 1 else max(codes.stride(0), M), list_off.data_ptr(), list_off.shape[0] - 1,
            pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else max(pr.stride(0), pr.shape[1]),
            pb.data_ptr(), pb.stride(0) if nq > 1 else max(pb.stride(0), pr.shape[1]),
            extra.data_ptr() if extra is not None else None)
    tail = (k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, ctypes.c_void_p(stream))
    fn = _lib.lib().pqhip_adc_ip_search_lists_residual_f32_dev if ip else _lib.lib().pqhip_adc_search_lists_residual_f32_dev
    rc = fn(*head, *tail)
    assert rc == _lib.OK, rc
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    v = np.stack([vb[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    i = np.stack([ib[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    return v, i


def search(pq, ip, cd, t, lo, pr, bias, k, extra=None, check=True):
    if ip:
        return pq.adc_ip_search_lists_residual_device(cd, t, lo, pr, bias, k, scales=extra, check=check)
    return pq.adc_search_lists_residual_device(cd, t, lo, pr, bias, extra, k, check=check)


def check_all(pq, ip, cd, t, lo, pr, bias, s, ks, extra=None):
    """Every k of ks: the Python entry point and the raw one (sentinels) against the reference over the scan s."""
    off, probes, b = lo.cpu().numpy(), pr.cpu().numpy(), bias.cpu().numpy()
    ex = None if extra is None else extra.cpu().numpy()
    for k in ks:
        want_v, want_i = ref_residual_search(s, off, probes, b, k, terms=None if ip else ex, scales=ex if ip else None, ip=ip)
        v, i = search(pq, ip, cd, t, lo, pr, bias, k, extra=extra)
        if t.dim() == 2:
            assert tuple(v.shape) == (k,) and tuple(i.shape) == (k,)
            v, i = v[None], i[None]
        assert str(v.dtype) == "torch.float32" and str(i.dtype) == "torch.int64"
        assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
        rv, ri = search_raw(pq, ip, cd, t, lo, pr, bias, k, extra=extra)
        assert_same(rv, ri, want_v, want_i)


def make_bias(seed, nq, n_probe):
    """some negative, a few times the spread of a scan"""
    import torch
    return torch.from_numpy((synth.normalish(seed, (nq, n_probe)) * np.float32(3.0)).astype(np.float32)).cuda()


def make_terms(seed, n):
    import torch
    return torch.from_numpy((synth.normalish(seed, (n,)) * np.float32(2.0) + np.float32(1.0)).astype(np.float32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", SHAPES)
@pytest.mark.parametrize("n,nq,n_lists", [(5003, 5, 13), (120011, 9, 64)])
def test_gpu_residual_search_matches_reference(ra, M, K, dsub, opq, n, nq, n_lists):
    """Distance and similarity, with and without scales (some negative), negative biases, k in {1, 10, 64, 65, 1024},
    n_probe in {1, 3, n_lists}; the (3, 7, 5) shape ties thousands of rows within a list, and the position decides."""
    import torch
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9700 + M, M, K, dsub, opq, n, nq)
    lo = torch.from_numpy(make_lists(9710 + n, n, n_lists)).cuda()
    terms = make_terms(9711, n)
    ks = (1, 10, 64, 65, 1024)
    for n_probe in (1, 3, n_lists):
        pr = torch.from_numpy(make_probes(9720 + n_probe, nq, n_lists, n_probe)).cuda()
        bias = make_bias(9730 + n_probe, nq, n_probe)
        ra.launch_log(reset=True)
        check_all(pq, False, cd, t_ip, lo, pr, bias, ipsum, ks, extra=terms)
        log = ra.launch_log(reset=True)
        assert "k_adc_lists_plan" in log and "k_adc_search_lists_residual_u8" in log and "k_adc_search_merge" in log, log
        assert "k_adc_search_u8" not in log and "k_adc_scan" not in log and "k_adc_search_lists_u8" not in log, log
        check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, ks[:4])
        log = ra.launch_log(reset=True)
        assert "k_adc_lists_plan" in log and "k_adc_ip_search_lists_residual_u8" in log and "k_adc_ip_search_merge" in log, log
        assert "k_adc_ip_search_u8" not in log and "k_adc_scan" not in log and "k_adc_ip_search_lists_u8" not in log, log
        check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, ks, extra=scd)
    # one query through 2-D tables, a 1-D probe row and a 1-D bias row
    pr1 = torch.from_numpy(make_probes(9740, 1, n_lists, 3)[0]).cuda()
    b1 = make_bias(9741, 1, 3)[0].contiguous()
    check_all(pq, False, cd, t_ip[2].contiguous(), lo, pr1, b1, ipsum[2], (10,), extra=terms)
    check_all(pq, True, cd, t_ip[2].contiguous(), lo, pr1, b1, ipsum[2], (10,), extra=scd)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,dsub,opq", [(15, 256, 20, False), (3, 7, 5, True)])
def test_gpu_residual_search_does_not_depend_on_the_grid(ra, M, K, dsub, opq):
    """Forced workgroups per query 1, 2, 7, the CU count, and auto: one result."""
    import torch
    n, nq, n_lists = 90001, 4, 37
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9750 + M, M, K, dsub, opq, n, nq)
    lo = torch.from_numpy(make_lists(9751, n, n_lists)).cuda()
    terms = make_terms(9752, n)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for g in (1, 2, 7, n_cus, 0):
            ra.set_option(OPTION, g)
            for n_probe in (1, 3, n_lists):
                pr = torch.from_numpy(make_probes(9753 + n_probe, nq, n_lists, n_probe)).cuda()
                bias = make_bias(9760 + n_probe, nq, n_probe)
                check_all(pq, False, cd, t_ip, lo, pr, bias, ipsum, (1, 65, 1024), extra=terms)
                check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, (10, 64), extra=scd)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
def test_gpu_residual_search_edges(ra):
    """Empty lists, -1 padding in the middle of a row under a NaN bias that must not surface, a probe row of only -1,
    fewer probed rows than k, strided bias / probe matrices and codes, no rows, no lists, and a NaN and +-Inf bias on
    probed lists, ordered and returned as the key rules say."""
    import torch
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 40003, 6, 21
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9770, M, K, dsub, False, n, nq)
    off = make_lists(9771, n, n_lists, empty_every=2)
    off[n_lists - 1] = n - 40                              # the last list holds 40 rows
    off = np.maximum.accumulate(np.minimum(off, n))
    off[n_lists - 1] = n - 40
    lo = torch.from_numpy(off).cuda()
    terms = make_terms(9772, n)
    probes = make_probes(9773, nq, n_lists, 6)
    b = (synth.normalish(9774, (nq, 6)) * np.float32(3.0)).astype(np.float32)
    probes[0, [1, 4]] = -1                                 # padding in the middle of a row ...
    b[0, [1, 4]] = np.nan                                  # ... whose bias is a NaN
    probes[1] = -1                                         # nothing probed: padding only
    b[1] = np.nan
    probes[2] = [n_lists - 1, -1, -1, -1, -1, -1]          # 40 rows < k
    probes[3] = [0, 2, 4, -1, 6, 8]                        # empty lists only, under NaN biases
    b[3] = np.nan
    assert all(off[l + 1] == off[l] for l in (0, 2, 4, 6, 8))
    pr, bias = torch.from_numpy(probes).cuda(), torch.from_numpy(b).cuda()
    check_all(pq, False, cd, t_ip, lo, pr, bias, ipsum, (1, 64, 1024), extra=terms)
    check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, (10, 65), extra=scd)
    check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, (10,))
    d, i = search(pq, False, cd, t_ip, lo, pr, bias, 64, extra=terms)
    assert (i[1] == -1).all() and torch.isposinf(d[1]).all() and (i[3] == -1).all()
    assert (i[2, :40] >= n - 40).all() and (i[2, 40:] == -1).all()
    assert not torch.isnan(d[0]).any()                     # the NaN biases of row 0 sit at skipped slots
    # a probe matrix and a bias matrix with row strides (columns of wider matrices)
    wide = torch.full((nq, 9), 0, dtype=torch.int64, device="cuda")
    wide[:, 1:5] = pr[:, :4]
    wb = torch.full((nq, 11), float("nan"), dtype=torch.float32, device="cuda")
    wb[:, 2:6] = bias[:, :4]
    check_all(pq, False, cd, t_ip, lo, wide[:, 1:5], wb[:, 2:6], ipsum, (10,), extra=terms)
    check_all(pq, True, cd, t_ip, lo, wide[:, 1:5], wb[:, 2:6], ipsum, (10,), extra=scd)
    # unaligned first row and an odd row stride of the codes
    wc = synth.codes_u8(9775, (n + 3, M + 6), K)
    wcd = torch.from_numpy(wc).cuda()
    for r0, c0 in ((1, 3), (2, 5), (3, 0)):
        view = wcd[r0:r0 + n, c0:c0 + M]
        s = orc.adc_scan(t_ip.cpu().numpy(), np.ascontiguousarray(wc[r0:r0 + n, c0:c0 + M]))
        check_all(pq, False, view, t_ip, lo, pr, bias, s, (7, 100), extra=terms)
        check_all(pq, True, view, t_ip, lo, pr, bias, s, (7,), extra=scd)
    # n_codes == 0 (every list empty) and n_lists == 0: the padding only
    z = torch.zeros(n_lists + 1, dtype=torch.int64, device="cuda")
    d, i = search(pq, False, cd[:0], t_ip, z, pr, bias, 5, extra=terms[:0])
    assert (i == -1).all() and torch.isposinf(d).all()
    s, i = search(pq, True, cd[:0], t_ip, z, pr, bias, 5)
    assert (i == -1).all() and torch.isneginf(s).all()
    pad = torch.full((nq, 2), -1, dtype=torch.int64, device="cuda")
    d, i = search(pq, False, cd, t_ip, z[:1], pad, bias[:, :2].contiguous(), 5, extra=terms)
    assert (i == -1).all() and torch.isposinf(d).all()
    s, i = search(pq, True, cd, t_ip, z[:1], pad, bias[:, :2].contiguous(), 5, extra=scd)
    assert (i == -1).all() and torch.isneginf(s).all()
    # NaN, +Inf and -Inf biases on probed, non-empty lists
    full = [l for l in range(n_lists) if off[l + 1] > off[l]]
    assert len(full) >= 4
    probes = np.tile(np.array(full[:4], np.int64), (nq, 1))
    b = (synth.normalish(9776, (nq, 4)) * np.float32(3.0)).astype(np.float32)
    b[0, 1] = np.nan
    b[1, 0] = np.inf
    b[2, 2] = -np.inf
    b[3] = [np.nan, np.inf, -np.inf, 1.0]
    b[4] = np.nan                                          # every probed row is a NaN: ordered by position
    pr, bias = torch.from_numpy(probes).cuda(), torch.from_numpy(b).cuda()
    rows4 = int(sum(off[l + 1] - off[l] for l in full[:4]))
    ks = (1, 10, 1024) if rows4 > 1024 else (1, 10, rows4)
    check_all(pq, False, cd, t_ip, lo, pr, bias, ipsum, ks, extra=terms)
    check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, ks, extra=scd)
    check_all(pq, True, cd, t_ip, lo, pr, bias, ipsum, ks)
    d, i = search(pq, False, cd, t_ip, lo, pr, bias, 10, extra=terms)
    assert torch.isneginf(d[2, 0]) and torch.isnan(d[4]).all()
    assert i[4].tolist() == sorted(i[4].tolist()) and i[4, 0] == min(int(off[l]) for l in full[:4])


@pytest.mark.gpu
def test_gpu_residual_search_reports_bad_ids_and_offsets(ra):
    """A list id outside [0, n_lists) other than -1, an offset past n_codes, a negative offset and an inverted range
    raise the stream's range flag; the call returns what the clamped input defines (the bias of a bad id is a NaN that
    does not surface) and writes nothing outside the outputs."""
    import torch
    from reductive_amd import _lib
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 20011, 3, 9
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9780, M, K, dsub, False, n, nq)
    off = make_lists(9781, n, n_lists, empty_every=100)
    lo = torch.from_numpy(off).cuda()
    terms = make_terms(9782, n)
    good = make_probes(9783, nq, n_lists, 4)
    allp = np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))
    cases = []
    bad_id = good.copy()
    bad_id[1, 2] = n_lists                                  # one past the last list
    cases.append((off, bad_id, (1, 2)))
    neg_id = good.copy()
    neg_id[0, 0] = -2
    cases.append((off, neg_id, (0, 0)))
    past = off.copy()
    past[-1] = n + 100000                                   # the last list runs past the matrix
    cases.append((past, allp, None))
    negative = off.copy()
    negative[0] = -5
    cases.append((negative, allp, None))
    inverted = off.copy()
    inverted[4] = off[5] + 3 if off[5] + 3 <= n else off[5]
    inverted[5] = off[4]
    cases.append((inverted, np.tile(np.array([4], np.int64), (nq, 1)), None))
    s = torch.cuda.current_stream().cuda_stream
    for o, p, nan_at in cases:
        b = (synth.normalish(9784, p.shape) * np.float32(3.0)).astype(np.float32)
        if nan_at is not None:
            b[nan_at] = np.nan
        od, pd_, bd = torch.from_numpy(o).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(b).cuda()
        for ip in (False, True):
            extra = scd if ip else terms
            with pytest.raises(ra.PanicError, match="index out of bounds"):
                search(pq, ip, cd, t_ip, od, pd_, bd, 10, extra=extra)
            v, i = search(pq, ip, cd, t_ip, od, pd_, bd, 10, extra=extra, check=False)
            ex = extra.cpu().numpy()
            want_v, want_i = ref_residual_search(ipsum, o, p, b, 10, terms=None if ip else ex, scales=ex if ip else None, ip=ip)
            assert_same(v.cpu().numpy(), i.cpu().numpy(), want_v, want_i)
            assert _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
            rv, ri = search_raw(pq, ip, cd, t_ip, od, pd_, bd, 10, extra=extra)      # sentinels intact
            assert_same(rv, ri, want_v, want_i)
            assert _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(s)) == _lib.ECODE_RANGE
    gb = make_bias(9785, nq, 4)
    search(pq, False, cd, t_ip, lo, torch.from_numpy(good).cuda(), gb, 10, extra=terms)      # flag consumed, good input passes
    # a code >= K inside a probed list is reported as by the plain searches
    pq_small = ra.Pq(None, synth.normalish(9786, (M, 200, 4)))
    ts = pq_small.adc_ip_tables_device(torch.from_numpy(synth.normalish(9787, (nq, M * 4))).cuda())
    bad = cd % 200
    pr = torch.from_numpy(good).cuda()
    search(pq_small, False, bad, ts, lo, pr, gb, 10, extra=terms)
    bad[int(off[good[0, 0]]), 3] = 200
    if off[good[0, 0] + 1] > off[good[0, 0]]:
        for ip in (False, True):
            with pytest.raises(ra.PanicError, match="index out of bounds"):
                search(pq_small, ip, bad, ts, lo, pr, gb, 10, extra=scd if ip else terms)


@pytest.mark.gpu
def test_gpu_residual_search_status_codes(ra):
    import torch
    from reductive_amd import _lib
    M, K, n, n_lists = 15, 256, 100, 4
    pq = ra.Pq(None, synth.normalish(9790, (M, K, 4)))
    yd = torch.from_numpy(synth.normalish(9791, (2, M * 4))).cuda()
    t = pq.adc_ip_tables_device(yd)
    cd = torch.from_numpy(synth.codes_u8(9792, (n, M), K)).cuda()
    lo = torch.tensor([0, 10, 50, 50, 100], dtype=torch.int64, device="cuda")
    pr = torch.tensor([[0, 1], [2, 3]], dtype=torch.int64, device="cuda")
    bias = make_bias(9793, 2, 2)
    terms = make_terms(9794, n)
    for k, want in ((0, _lib.EINVAL), (1025, _lib.EUNSUPPORTED)):
        for ip in (False, True):
            with pytest.raises(_lib.PqHipError) as e:
                search(pq, ip, cd, t, lo, pr, bias, k, extra=None if ip else terms)
            assert e.value.status == want
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    out_v = torch.empty(20, dtype=torch.float32, device="cuda")
    out_i = torch.empty(20, dtype=torch.int64, device="cuda")
    UNSET = object()

    def call(ip, slot=0, nq=1, cb=1, nn=n, c_rs=M, off=lo.data_ptr(), nl=n_lists, probes=pr.data_ptr(), n_probe=2, p_rs=2,
             b=bias.data_ptr(), b_rs=2, extra=UNSET, k=10, v_rs=10, i_rs=10):
        if extra is UNSET:
            extra = None if ip else terms.data_ptr()
        head = (pq._cb(), slot, t.data_ptr(), nq, cd.data_ptr(), cb, nn, c_rs, off, nl, probes, n_probe, p_rs, b, b_rs, extra)
        tail = (k, out_v.data_ptr(), v_rs, out_i.data_ptr(), i_rs, ctypes.c_void_p(s))
        fn = L.pqhip_adc_ip_search_lists_residual_f32_dev if ip else L.pqhip_adc_search_lists_residual_f32_dev
        return fn(*head, *tail)
    for ip in (False, True):
        assert call(ip) == _lib.OK
        assert call(ip, nl=-1) == _lib.EINVAL
        assert call(ip, n_probe=0) == _lib.EINVAL
        assert call(ip, off=None) == _lib.EINVAL
        assert call(ip, probes=None) == _lib.EINVAL
        assert call(ip, b=None) == _lib.EINVAL                        # new: no probe bias
        assert call(ip, slot=7) == _lib.ENODEV
        assert call(ip, slot=7, k=0) == _lib.EINVAL                   # EINVAL before ENODEV
        assert call(ip, slot=7, b=None) == _lib.ENODEV                # the null checks come after, as for the other pointers
        assert call(ip, cb=4) == _lib.EUNSUPPORTED                    # 1-byte codes only
        assert call(ip, cb=2) == _lib.EUNSUPPORTED
        assert call(ip, cb=4, slot=7) == _lib.ENODEV                  # ENODEV before EUNSUPPORTED
        assert call(ip, cb=4, k=0) == _lib.EINVAL
        assert call(ip, cb=4, b=None) == _lib.EUNSUPPORTED            # EUNSUPPORTED before the null checks
        assert call(ip, nn=(1 << 32) - 1) == _lib.EUNSUPPORTED        # more rows than 32-bit positions hold
        assert call(ip, p_rs=1) == _lib.ESHAPE
        assert call(ip, b_rs=1) == _lib.ESHAPE                        # new: bias rows shorter than n_probe
        assert call(ip, b_rs=1, b=None) == _lib.EINVAL                # EINVAL (null) before ESHAPE
        assert call(ip, v_rs=9) == _lib.ESHAPE
        assert call(ip, i_rs=9) == _lib.ESHAPE
        assert call(ip, c_rs=M - 1) == _lib.ESHAPE
        assert call(ip, k=1025, v_rs=9) == _lib.EUNSUPPORTED          # EUNSUPPORTED before ESHAPE
        assert call(ip, k=1025, b_rs=1) == _lib.EUNSUPPORTED
        assert call(ip, cb=4, p_rs=1) == _lib.EUNSUPPORTED
        torch.cuda.synchronize()
        ra.launch_log(reset=True)
        assert call(ip, nq=0) == _lib.OK                              # n_queries == 0 launches nothing
        assert call(ip, nq=0, off=None, probes=None, b=None, extra=None) == _lib.OK
        assert ra.launch_log(reset=True) == ""
    assert call(False, extra=None) == _lib.EINVAL                     # new: the distance call needs the row terms
    assert call(False, extra=None, b_rs=1) == _lib.EINVAL
    assert call(True, extra=None) == _lib.OK                          # the similarity call takes no scales
    # a table that does not fit the LDS beside the queues: unsupported, not a silent other path
    big = ra.Pq(None, synth.normalish(9795, (48, 1024, 2)))
    tb = big.adc_ip_tables_device(torch.from_numpy(synth.normalish(9796, (2, 96))).cuda())
    cb48 = torch.from_numpy(synth.codes_u8(9797, (n, 48), 256)).cuda()
    with pytest.raises(_lib.PqHipError) as e:
        big.adc_search_lists_residual_device(cb48, tb, lo, pr, bias, terms, 10)
    assert e.value.status == _lib.EUNSUPPORTED
    # the wrappers check the shapes of the new inputs
    with pytest.raises(ra.PanicError):
        pq.adc_search_lists_residual_device(cd, t, lo, pr, bias[:, :1].contiguous(), terms, 10)
    with pytest.raises(ra.PanicError):
        pq.adc_search_lists_residual_device(cd, t, lo, pr, bias, terms[:-1].contiguous(), 10)
    with pytest.raises(ra.PanicError):
        pq.adc_ip_search_lists_residual_device(cd, t, lo, pr, None, 10)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_residual_search_many_probes_and_queries(ra):
    """More probes than one plan pass of 1,024 and more queries than workgroups per query can share CUs."""
    import torch
    M, K, dsub, n, nq, n_lists = 15, 256, 20, 50021, 300, 3000
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = setup(ra, 9800, M, K, dsub, False, n, nq)
    lo = torch.from_numpy(make_lists(9801, n, n_lists, empty_every=3)).cuda()
    terms = make_terms(9802, n)
    pr = torch.from_numpy(make_probes(9803, nq, n_lists, n_lists)).cuda()
    check_all(pq, False, cd, t_ip, lo, pr, make_bias(9804, nq, n_lists), ipsum, (10, 1024), extra=terms)
    pr = torch.from_numpy(make_probes(9805, nq, n_lists, 1500)).cuda()
    check_all(pq, True, cd, t_ip, lo, pr, make_bias(9806, nq, 1500), ipsum, (100,), extra=scd)


def _mapped(ids, pos):
    return np.where(pos < 0, -1, ids[np.clip(pos, 0, None)])


@pytest.mark.gpu
@pytest.mark.parametrize("given_opq,from_vectors", [(False, True), (True, False), (False, False)])
def test_gpu_residual_partitioned_matrix(ra, given_opq, from_vectors):
    """partition_residual() with a trained residual quantizer and with a given OPQ one, from given vectors and from the
    reconstructions: the lists of partition(), residual codes, row terms, probes, both searches bit for bit against the
    reference evaluated on the matrix's own tensors, embeddings()."""
    import torch
    from reductive_amd import qmatrix
    M, K, dsub, N, n_lists = 15, 256, 4, 30011, 24
    d = M * dsub
    q = synth.normalish(9810, (M, K, dsub))
    pq = ra.Pq(None, q)
    centres = synth.normalish(9812, (40, d)) * np.float32(3.0)
    x = (centres[np.random.default_rng(9813).integers(0, 40, N)] + synth.normalish(9814, (N, d))).astype(np.float32)
    codes = pq.quantize_batch(x)
    norms = synth.uniform01(9815, (N,)) + np.float32(0.5)
    qm = qmatrix.QuantizedMatrix.load(io.BytesIO(qmatrix.dumps(pq, codes, norms)))
    given = None
    if given_opq:
        given = ra.Pq(synth.orthonormal(9816, d), synth.normalish(9817, (5, 64, d // 5)) * np.float32(0.7))
    kw = dict(n_iterations=5, vectors=x if from_vectors else None, train_rows=20000)
    rm = qm.partition_residual(n_lists, n_subquantizer_bits=6, pq_iterations=4, residual_pq=given,
                               rng=np.random.default_rng(9818), **kw)
    pm = qm.partition(n_lists, rng=np.random.default_rng(9818), **kw)
    assert isinstance(rm, qmatrix.ResidualPartitionedMatrix) and len(rm) == N
    rq, rP = rm.pq.subquantizers(), rm.pq.projection()
    if given_opq:
        assert rm.pq is given
    else:
        assert rq.shape == (M, 64, dsub) and rP is None
    # the lists are those of partition() under the same seed, and so are the probes
    ids, off = rm.ids.cpu().numpy(), rm.list_off.cpu().numpy()
    assert np.array_equal(rm.centroids, pm.centroids) and np.array_equal(ids, pm.ids.cpu().numpy())
    assert np.array_equal(off, pm.list_off.cpu().numpy())
    assert np.array_equal(rm.positions.cpu().numpy(), pm.positions.cpu().numpy())
    assert np.array_equal(rm.norms.cpu().numpy(), norms[ids])
    src = x if from_vectors else orc.reconstruct_batch(q, codes)
    want_assign = orc.cluster_assignments(rm.centroids, src)
    lists = np.searchsorted(off[1:], np.arange(N), side="right")
    assert np.array_equal(want_assign[ids], lists) and np.array_equal(rm.lists.cpu().numpy(), lists)
    # stored codes: the oracle's codes of the f32 residuals under the stored residual quantizer
    resid = (src[ids] - rm.centroids[lists]).astype(np.float32)
    rcodes = rm.codes.cpu().numpy()
    assert np.array_equal(rcodes, orc.quantize_batch(rq, resid, projection=rP))
    # row terms: one f32 rounding of the float64 sum, plus the float64 accumulation bound of both evaluations
    rec = orc.reconstruct_batch(rq, rcodes, projection=rP)
    r64, c64 = rec.astype(np.float64), rm.centroids[lists].astype(np.float64)
    t64 = (r64 * r64 + 2.0 * c64 * r64).sum(1)
    t_abs = (r64 * r64 + np.abs(2.0 * c64 * r64)).sum(1)
    got_t = rm.row_terms.cpu().numpy()
    assert got_t.dtype == np.float32
    assert (np.abs(got_t.astype(np.float64) - t64) <= 2.0 ** -24 * np.abs(t64) + d * 2.0 ** -52 * t_abs).all()
    ys = (synth.normalish(9819, (5, d)) + centres[:5]).astype(np.float32)
    yd = torch.from_numpy(ys).cuda()
    for nprobe in (1, 3, n_lists, n_lists + 5):
        assert torch.equal(rm.probes(yd, nprobe), pm.probes(yd, nprobe))
        assert torch.equal(rm.probes(yd[1], nprobe), pm.probes(yd[1], nprobe))
    # both searches against the reference on the matrix's own tensors
    s = scan(rq, ys, rcodes, projection=rP)
    coarse_l2 = orc.adc_tables(rm.centroids[None], ys)[:, 0, :]
    coarse_ip = ip_tables(rm.centroids[None], ys)[:, 0, :]
    nrm = rm.norms.cpu().numpy()
    for nprobe in (1, 3, n_lists):
        probes = rm.probes(yd, nprobe).cpu().numpy()
        b_l2 = np.take_along_axis(coarse_l2, probes, 1)
        b_ip = np.take_along_axis(coarse_ip, probes, 1)
        for k in (10, 500):
            wv, wp = ref_residual_search(s, off, probes, b_l2, k, terms=got_t)
            dd, ii = rm.nearest(yd, k, nprobe)
            assert_same(dd.cpu().numpy(), ii.cpu().numpy(), wv, _mapped(ids, wp))
            wv, wp = ref_residual_search(s, off, probes, b_ip, k, scales=nrm, ip=True)
            ss, jj = rm.most_similar(yd, k, nprobe)
            assert_same(ss.cpu().numpy(), jj.cpu().numpy(), wv, _mapped(ids, wp))
            wv, wp = ref_residual_search(s, off, probes, b_ip, k, ip=True)
            ss, jj = rm.most_similar(yd, k, nprobe, use_norms=False)
            assert_same(ss.cpu().numpy(), jj.cpu().numpy(), wv, _mapped(ids, wp))
            d1, i1 = rm.nearest(yd[2], k, nprobe)
            assert torch.equal(d1, dd[2]) and torch.equal(i1, ii[2])
            s1, j1 = rm.most_similar(yd[2], k, nprobe, use_norms=False)
            assert torch.equal(s1, ss[2]) and torch.equal(j1, jj[2])
    # embeddings(): fl(fl(r^ + c_l) * norm) of original row numbers
    rows = np.array([0, 17, N - 1, 12345])
    pos = rm.positions.cpu().numpy()[rows]
    want = ((rec[pos] + rm.centroids[lists[pos]]).astype(np.float32) * nrm[pos][:, None]).astype(np.float32)
    assert rm.embeddings(torch.from_numpy(rows).cuda()).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ra.ReductiveError):
        qm.partition_residual(0)
    with pytest.raises(ra.ReductiveError):
        qm.partition_residual(n_lists, n_subquantizer_bits=9)


@pytest.mark.gpu
def test_gpu_residual_encoding_is_more_accurate_than_flat_codes(ra):
    """The point of the feature, on a clustered fixture: 20,000 x 32 around 40 centres of scale 3, M = 8, 4 bits, 64
    lists, 200 queries near data points, k = 10, nprobe = 8, fixed seeds.  partition_residual() has strictly lower mean
    squared reconstruction error than the flat quantizer trained by the same train_pq call on the vectors, and strictly
    higher recall@10 against the true float64 neighbours than partition() over the flat codes.  (A float64 numpy model
    of the same fixture gave 12.9 against 62.3 and 0.39 against 0.10.)"""
    import torch
    from reductive_amd import qmatrix
    N, d, M, bits, n_lists, nq, k, nprobe = 20000, 32, 8, 4, 64, 200, 10, 8
    rng = np.random.default_rng(9830)
    centres = (rng.standard_normal((40, d)) * 3.0).astype(np.float32)
    x = (centres[rng.integers(0, 40, N)] + rng.standard_normal((N, d))).astype(np.float32)
    ys = (x[rng.choice(N, nq, replace=False)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    flat = ra.train_pq(M, bits, 10, 1, x, rng=np.random.default_rng(9831))
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x))
    pm = qm.partition(n_lists, vectors=x, rng=np.random.default_rng(9832))
    rm = qm.partition_residual(n_lists, vectors=x, rng=np.random.default_rng(9832))
    assert rm.pq.subquantizers().shape == (M, 1 << bits, d // M)
    allrows = torch.arange(N, device="cuda")
    x64 = x.astype(np.float64)
    mse_flat = float(((qm.embeddings(allrows).cpu().numpy().astype(np.float64) - x64) ** 2).sum(1).mean())
    mse_res = float(((rm.embeddings(allrows).cpu().numpy().astype(np.float64) - x64) ** 2).sum(1).mean())
    y64 = ys.astype(np.float64)
    d2 = (y64 ** 2).sum(1)[:, None] - 2.0 * y64 @ x64.T + (x64 ** 2).sum(1)[None]
    truth = np.argsort(d2, axis=1, kind="stable")[:, :k]
    yd = torch.from_numpy(ys).cuda()

    def recall(found):
        f = found.cpu().numpy()
        return float(np.mean([len(set(f[q].tolist()) & set(truth[q].tolist())) / k for q in range(nq)]))
    rec_flat = recall(pm.nearest(yd, k, nprobe)[1])
    rec_res = recall(rm.nearest(yd, k, nprobe)[1])
    print("mse flat %.4f residual %.4f; recall@10 flat %.4f residual %.4f" % (mse_flat, mse_res, rec_flat, rec_res))
    assert mse_res < mse_flat
    assert rec_res > rec_flat
