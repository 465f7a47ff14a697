"""ADC range searches on the GPU (include/pqhip.h: pqhip_adc_*range*_f32_dev) and within() / similar_above() of the
three matrix classes.  Reference: tests/adc_range_ref.py (pinned by test_adc_range.py), fed with what adc_scan_device
writes for the same tables and codes.  Everything is bit-exact: lims, indices and the order exactly, values byte for byte.
Covered: row counts around the wave and workgroup sizes, code widths, every number of queries per pass, thresholds on a
row's value / below every row / +-Inf / NaN, the capacity protocol with canaries, NaN tables and the range flag, masks,
the list forms with bad probes, and one result for every forced grid (options "adc_range_wgs",
"adc_range_wgs_per_query")."""
import ctypes

import numpy as np
import pytest

import synth
from adc_masked_ref import pack_ref
from adc_range_ref import ref_range, ref_range_lists, ref_range_residual

SENT_V = np.float32(-1234.5)
SENT_I = -777


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


_PQS = {}


def make_pq(ra, M, K):
    if (M, K) not in _PQS:
        _PQS[(M, K)] = ra.Pq(None, synth.normalish(8800 + M, (M, K, 4)))
    return _PQS[(M, K)]


def draw_tables(seed, nq, M, K, integer=False):
    """[nq, M, K] f32 on the device: integer-valued (many equal row sums) or uniform in [-1, 1)"""
    import torch
    rng = np.random.default_rng(seed)
    t = rng.integers(-2, 3, (nq, M, K)).astype(np.float32) if integer else (rng.random((nq, M, K), np.float32) * 2 - 1)
    return torch.from_numpy(np.ascontiguousarray(t, np.float32)).cuda()


def scan(pq, cd, tables):
    """what the references are fed with: adc_scan_device of the same tables, [nq, n]"""
    if cd.shape[0] == 0:
        return np.zeros((tables.shape[0], 0), np.float32)
    return pq.adc_scan_device(cd, tables).cpu().numpy()


def scaled(s, sc):
    with np.errstate(invalid="ignore", over="ignore"):
        return (s * sc[None]).astype(np.float32)


def dev_words(allow):
    import torch
    w = pack_ref(allow)
    if w.size == 0:
        return torch.zeros(1, dtype=torch.int32, device="cuda")[:0]
    return torch.from_numpy(w.view(np.int32).copy()).cuda()


def thresholds(values, seed, ip=False, specials=True):
    """one threshold per query: the exact value of a row (the boundary is included); with specials the queries from 1 on
    cycle through a value below (ip: above) every row, +Inf, NaN, -Inf and row values again"""
    rng = np.random.default_rng(seed)
    nq, n = values.shape
    thr = np.zeros(nq, np.float32)
    for q in range(nq):
        fin = values[q][np.isfinite(values[q])]
        thr[q] = fin[rng.integers(fin.size)] if fin.size else 0.0
        if specials and q >= 1:
            kind = q % 5
            if kind == 1 and fin.size:
                thr[q] = (fin.max() + 1) if ip else (fin.min() - 1)
            elif kind == 2:
                thr[q] = np.inf
            elif kind == 3:
                thr[q] = np.nan
            elif kind == 4:
                thr[q] = -np.inf
    return thr


def same(got, want, what=""):
    gl, gv, gi = [np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got]
    wl, wv, wi = want
    print("%s rows per query: got %s want %s" % (what, np.diff(gl).tolist(), np.diff(wl).tolist()))
    assert gl.dtype == np.int64 and gi.dtype == np.int64 and gv.dtype == np.float32
    assert np.array_equal(gl, wl), what
    assert np.array_equal(gi, wi), what
    assert gv.tobytes() == np.asarray(wv, np.float32).tobytes(), what


def fn_name(ip, lists=False, residual=False):
    return "pqhip_adc_%srange_%s%sf32_dev" % ("ip_" if ip else "", "lists_" if lists else "", "residual_" if residual else "")


def call_raw(pq, name, cd, tables, thr, capacity, words=None, lists=None, bias=None, extra=None, has_extra=False, want_rc=0,
             null_out=False, pad=5, c_rs=None, code_bytes=None):
    """A range entry point through the C ABI with canaries: lims has a sentinel on each side, val / idx hold `capacity`
    entries followed by `pad` canaries that must survive.  Returns (lims, val, idx) as numpy, val / idx cut to
    min(total, capacity)."""
    import torch
    from reductive_amd import _lib
    nq = tables.shape[0]
    n, M = cd.shape
    dev = tables.device
    lbuf = torch.full((nq + 3,), SENT_I, dtype=torch.int64, device=dev)
    vbuf = torch.full((capacity + pad,), float(SENT_V), dtype=torch.float32, device=dev)
    ibuf = torch.full((capacity + pad,), SENT_I, dtype=torch.int64, device=dev)
    td = torch.from_numpy(np.asarray(thr, np.float32).reshape(-1).copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = [pq._cb(), 0, tables.data_ptr(), nq, cd.data_ptr() if n else None, cd.element_size() if code_bytes is None else code_bytes,
            n, (cd.stride(0) if n > 1 else max(cd.stride(0), M)) if c_rs is None else c_rs,
            None if words is None else words.data_ptr()]
    if lists is not None:
        lo, pr = lists
        args += [lo.data_ptr(), lo.shape[0] - 1, pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else max(pr.stride(0), pr.shape[1])]
        if bias is not None:
            args += [bias.data_ptr(), bias.stride(0) if nq > 1 else max(bias.stride(0), pr.shape[1])]
    if has_extra:
        args.append(extra.data_ptr() if extra is not None else None)
    args += [td.data_ptr(), lbuf.data_ptr() + 8, None if null_out else vbuf.data_ptr(), None if null_out else ibuf.data_ptr(),
             capacity, ctypes.c_void_p(stream)]
    rc = getattr(_lib.lib(), name)(*args)
    assert rc == want_rc, (name, rc)
    if rc != _lib.OK:
        return None
    lb, vb, ib = lbuf.cpu().numpy(), vbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert lb[0] == SENT_I and lb[-1] == SENT_I, "write outside lims"
    lims = lb[1:-1].copy()
    total = int(lims[-1])
    wrote = min(total, capacity)
    assert (vb[wrote:] == SENT_V).all() and (ib[wrote:] == SENT_I).all(), "write at or beyond the capacity"
    return lims, vb[:wrote].copy(), ib[:wrote].copy()


def check_codes(pq):
    import torch
    from reductive_amd import _lib
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


# ---- exhaustive calls ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_range_row_counts(ra):
    """n around the wave (64) and the workgroup trip (1,024), n = 0 and one n beyond a workgroup's minimum range"""
    import torch
    M, K, nq = 15, 256, 3
    pq = make_pq(ra, M, K)
    t = draw_tables(8801, nq, M, K)
    ra.launch_log(reset=True)
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000):
        codes = synth.codes_u8(8802 + n, (n, M), K)
        cd = torch.from_numpy(codes).cuda()
        sc = (synth.uniform01(8803 + n, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
        s = scan(pq, cd, t)
        for ip, values, scd in ((False, s, None), (True, s, None), (True, scaled(s, sc), torch.from_numpy(sc).cuda())):
            thr = thresholds(values, 8804 + n, ip, specials=False) if n else np.zeros(nq, np.float32)
            if ip:
                got = pq.adc_ip_range_device(cd, t, thr, scales=scd, check=True)
            else:
                got = pq.adc_range_device(cd, t, thr, check=True)
            same(got, ref_range(values, thr, ip=ip), "n %d ip %s scales %s" % (n, ip, scd is not None))
    log = ra.launch_log(reset=True)
    assert "k_adc_range_u8" in log and "k_adc_ip_range_u8" in log and "k_adc_range_scan" in log, log
    assert "k_adc_search" not in log, log
    # 2-D tables: lims is [2]
    lims, d, i = pq.adc_range_device(cd, t[1].contiguous(), float(thr[0]))
    assert tuple(lims.shape) == (2,) and int(lims[0]) == 0 and int(lims[1]) == d.shape[0] == i.shape[0]


@pytest.mark.gpu
def test_gpu_range_does_not_depend_on_the_grid(ra):
    import torch
    M, K, nq, n = 15, 256, 5, 40013
    pq = make_pq(ra, M, K)
    t = draw_tables(8810, nq, M, K)
    cd = torch.from_numpy(synth.codes_u8(8811, (n, M), K)).cuda()
    s = scan(pq, cd, t)
    thr = thresholds(s, 8812)
    want = ref_range(s, thr)
    want_ip = ref_range(s, thr, ip=True)
    try:
        for wgs in (1, 2, 7, 0):
            ra.set_option("adc_range_wgs", wgs)
            same(pq.adc_range_device(cd, t, thr), want, "wgs %d" % wgs)
            same(pq.adc_ip_range_device(cd, t, thr), want_ip, "ip wgs %d" % wgs)
    finally:
        ra.set_option("adc_range_wgs", 0)


@pytest.mark.gpu
def test_gpu_range_row_stride_and_unaligned_base(ra):
    import torch
    M, K, nq, n = 15, 256, 4, 1500
    pq = make_pq(ra, M, K)
    t = draw_tables(8820, nq, M, K)
    codes = synth.codes_u8(8821, (n + 1, M), K)
    wide = torch.zeros((n, 20), dtype=torch.uint8, device="cuda")
    wide[:, :M] = torch.from_numpy(codes[:n]).cuda()
    for what, cd in (("stride 20", wide[:, :M]), ("base + 15", torch.from_numpy(codes).cuda()[1:])):
        assert cd.stride(1) == 1 and (cd.stride(0) > M or cd.data_ptr() % 4 != 0)
        s = scan(pq, cd.contiguous(), t)
        thr = thresholds(s, 8822, specials=False)
        same(pq.adc_range_device(cd, t, thr), ref_range(s, thr), what)
        same(pq.adc_ip_range_device(cd, t, thr), ref_range(s, thr, ip=True), what + " ip")


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,integer", [(3, 16, False), (8, 16, True), (15, 256, False), (16, 256, False), (30, 32, False),
                                             (33, 64, False), (100, 16, False)])
def test_gpu_range_code_widths(ra, M, K, integer):
    """every dword bucket of the row fetch; (8, 16) with integer tables: many values tie with the threshold"""
    import torch
    nq, n = 9, 1500                                            # 9 queries: a pass of 8 and a pass of 1
    pq = make_pq(ra, M, K)
    t = draw_tables(8830 + M, nq, M, K, integer=integer)
    cd = torch.from_numpy(synth.codes_u8(8831 + M, (n, M), K)).cuda()
    sc = (synth.uniform01(8832 + M, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    s = scan(pq, cd, t)
    thr = thresholds(s, 8833, specials=False)
    same(pq.adc_range_device(cd, t, thr, check=True), ref_range(s, thr), "l2")
    if integer:
        assert (s == thr[:, None]).sum() > 10 * nq             # ties on the boundary
    v = scaled(s, sc)
    thr = thresholds(v, 8834, ip=True, specials=False)
    same(pq.adc_ip_range_device(cd, t, thr, scales=torch.from_numpy(sc).cuda(), check=True), ref_range(v, thr, ip=True), "ip")


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 8, 9, 13])
def test_gpu_range_queries_per_pass(ra, nq):
    """8 / 4 / 1 queries per pass and their remainders, each query its own threshold: a row's exact value, below every
    row, +Inf, NaN, -Inf; and the same with one query per pass (option adc_single_query)"""
    import torch
    M, K, n = 15, 256, 3000
    pq = make_pq(ra, M, K)
    t = draw_tables(8840 + nq, nq, M, K)
    t[0, 2, 5] = -0.0
    cd = torch.from_numpy(synth.codes_u8(8841, (n, M), K)).cuda()
    s = scan(pq, cd, t)
    ra.launch_log(reset=True)
    for ip in (False, True):
        thr = thresholds(s, 8842 + nq, ip)
        want = ref_range(s, thr, ip=ip)
        fn = pq.adc_ip_range_device if ip else pq.adc_range_device
        same(fn(cd, t, thr), want, "ip %s" % ip)
        try:
            ra.set_option("adc_single_query", 1)
            same(fn(cd, t, thr), want, "single, ip %s" % ip)
        finally:
            ra.set_option("adc_single_query", 0)
    log = ra.launch_log(reset=True)
    if nq >= 8:
        assert "k_adc_range_u8_mq<8 queries>" in log, log
    if nq % 8 >= 4:
        assert "k_adc_range_u8_mq<4 queries>" in log, log


@pytest.mark.gpu
def test_gpu_range_capacity_protocol(ra):
    import torch
    M, K, nq, n = 15, 256, 5, 3000
    pq = make_pq(ra, M, K)
    t = draw_tables(8850, nq, M, K)
    cd = torch.from_numpy(synth.codes_u8(8851, (n, M), K)).cuda()
    s = scan(pq, cd, t)
    thr = thresholds(s, 8852, specials=False)
    wl, wv, wi = ref_range(s, thr)
    total = int(wl[-1])
    assert total > 100
    ra.launch_log(reset=True)
    lims, v, i = call_raw(pq, fn_name(False), cd, t, thr, 0, null_out=True)          # a pure count call
    assert np.array_equal(lims, wl) and v.size == 0
    log = ra.launch_log(reset=True)
    assert log == "k_adc_range_u8_mq<4 queries> + k_adc_range_scan x2 + k_adc_range_u8", log   # no fill pass was launched
    for cap in (total - 1, total // 2, 1, total, total + 7):
        lims, v, i = call_raw(pq, fn_name(False), cd, t, thr, cap)
        w = min(cap, total)
        assert np.array_equal(lims, wl), cap                                           # the true counts, whatever the capacity
        assert np.array_equal(i, wi[:w]) and v.tobytes() == wv[:w].tobytes(), cap      # a valid prefix
    same(pq.adc_range_device(cd, t, thr, capacity=1), (wl, wv, wi), "retry from capacity 1")
    same(pq.adc_range_device(cd, t, thr, capacity=0), (wl, wv, wi), "count, then fill")
    same(pq.adc_range_device(cd, t, thr, capacity=total), (wl, wv, wi), "exact capacity")


@pytest.mark.gpu
def test_gpu_range_nan_tables_and_range_flag(ra):
    import torch
    from reductive_amd import _lib
    M, K, nq, n = 15, 256, 4, 2000
    pq = make_pq(ra, M, K)
    t = draw_tables(8860, nq, M, K)
    t[0, 3, :64] = float("nan")                                # a quarter of the rows of query 0 sum to NaN
    t[1, 0, 7], t[2, 1, 9] = float("inf"), float("-inf")
    codes = synth.codes_u8(8861, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    s = scan(pq, cd, t)
    assert np.isnan(s[0]).sum() > 100
    for ip in (False, True):
        thr = np.array([np.inf, np.inf, -np.inf, 0.0], np.float32) * (-1 if ip else 1)
        fn = pq.adc_ip_range_device if ip else pq.adc_range_device
        got = fn(cd, t, thr, check=True)                       # a clean run raises no flag
        same(got, ref_range(s, thr, ip=ip), "nan ip %s" % ip)
        assert not np.isnan(got[1].cpu().numpy()).any()
        assert int(got[0][1]) == n - int(np.isnan(s[0]).sum())  # +-Inf: every non-NaN row
    K2 = 16
    pq2 = make_pq(ra, 8, K2)
    t2 = draw_tables(8862, 2, 8, K2)
    bad = synth.codes_u8(8863, (500, 8), K2)
    bad[123, 4] = K2                                            # reads entry 0 and raises the flag
    bd = torch.from_numpy(bad).cuda()
    fixed = bad.copy()
    fixed[123, 4] = 0
    s2 = scan(pq2, torch.from_numpy(fixed).cuda(), t2)
    thr = thresholds(s2, 8864, specials=False)
    assert check_codes(pq2) == _lib.OK
    same(pq2.adc_range_device(bd, t2, thr), ref_range(s2, thr), "code >= K reads entry 0")
    assert check_codes(pq2) == _lib.ECODE_RANGE
    assert check_codes(pq2) == _lib.OK
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq2.adc_ip_range_device(bd, t2, thr, check=True)


@pytest.mark.gpu
def test_gpu_range_masks(ra):
    import torch
    from reductive_amd import _lib
    M, K, nq, n = 15, 256, 9, 5003
    pq = make_pq(ra, M, K)
    t = draw_tables(8870, nq, M, K)
    codes = synth.codes_u8(8871, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    sc = (synth.uniform01(8872, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    s = scan(pq, cd, t)
    thr = thresholds(s, 8873)
    rng = np.random.default_rng(8875)
    plain = pq.adc_range_device(cd, t, thr)
    pq_small = make_pq(ra, M, 200)                             # K = 200: code 255 is out of range there
    t_small = t[:, :, :200].contiguous()
    cs = np.minimum(codes, 199)
    v_small = scaled(scan(pq_small, torch.from_numpy(cs).cuda(), t_small), sc)
    thr_ip = thresholds(v_small, 8874, ip=True)
    for what, allow in (("ones", np.ones(n, bool)), ("zeros", np.zeros(n, bool)), ("half", rng.random(n) < 0.5),
                        ("1 %", rng.random(n) < 0.01)):
        wd = dev_words(allow)
        got = pq.adc_range_device(cd, t, thr, allow=wd, check=True)
        same(got, ref_range(s, thr, allow=allow), what)
        if what == "ones":
            same(got, [a.cpu().numpy() for a in plain], "all ones equals NULL")
        if what == "zeros":
            assert int(got[0][-1]) == 0
        # a code >= K and a NaN scale in a disallowed row: not read, no flag, nothing changes
        cs_bad, sbad = cs.copy(), sc.copy()
        off = np.flatnonzero(~allow)
        if off.size:
            cs_bad[off[0], 3] = 255
            sbad[off] = np.nan
        assert check_codes(pq_small) == _lib.OK
        got = pq_small.adc_ip_range_device(torch.from_numpy(cs_bad).cuda(), t_small, thr_ip, scales=torch.from_numpy(sbad).cuda(),
                                           allow=wd)
        assert check_codes(pq_small) == _lib.OK, what
        same(got, ref_range(v_small, thr_ip, ip=True, allow=allow), what + " ip, poisoned disallowed rows")


# ---- list calls ---------------------------------------------------------------------------------------------------
def lists_setup(seed, n, n_lists=16):
    """offsets with empty lists, a list of one row and one of more than 1,024 rows"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 300, n_lists)
    sizes[[2, 9]] = 0
    sizes[5] = 1
    sizes[11] = 1500
    sizes[-1] += n - sizes.sum()
    assert sizes[-1] > 0
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("n_probe", [1, 3, 16])
def test_gpu_range_lists(ra, n_probe):
    """flat and residual, L2 and IP, with and without scales, unmasked and masked, for every forced number of workgroups
    per query: -1 padding in the middle of a probe row, a bad list id (flag raised, the others served), probes in
    non-ascending list order, a different bias per probe slot and a NaN bias on every skipped probe"""
    import torch
    from reductive_amd import _lib
    M, K, nq, n, n_lists = 15, 256, 5, 4000, 16
    pq = make_pq(ra, M, K)
    t = draw_tables(8880, nq, M, K)
    codes = synth.codes_u8(8881, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    off = lists_setup(8882, n, n_lists)
    rng = np.random.default_rng(8883 + n_probe)
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    pr[0, 0] = 11                                              # the long list, and for n_probe == 1 a one-row list
    pr[1, 0] = 5
    bad_id = n_probe >= 3
    if bad_id:
        pr[2, 1] = -1                                          # padding in the middle
        pr[3, 1] = n_lists + 3                                 # a bad id: skipped, flag raised
        pr[4, :3] = [12, 7, 3]                                 # non-ascending
    bias = rng.standard_normal(pr.shape).astype(np.float32)
    bias[(pr < 0) | (pr >= n_lists)] = np.nan                  # never read into a result
    bias[np.isin(pr, [2, 9])] = np.nan                         # empty lists are skipped probes too
    terms = rng.standard_normal(n).astype(np.float32)
    sc = (synth.uniform01(8884, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    allow = rng.random(n) < 0.5
    s = scan(pq, cd, t)
    od, pd, bd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda(), torch.from_numpy(bias).cuda()
    td, scd, wd = torch.from_numpy(terms).cuda(), torch.from_numpy(sc).cuda(), dev_words(allow)
    full = np.broadcast_to(np.arange(n_lists, dtype=np.int64), (nq, n_lists))
    zero_bias = np.zeros((nq, n_lists), np.float32)

    def pick(csr_all_lists, seed, ip):
        """thresholds from the values of all rows: a row's value, then the special ones"""
        vals = np.stack([csr_all_lists[1][csr_all_lists[0][q]:csr_all_lists[0][q + 1]][:n] for q in range(nq)])
        return thresholds(vals, seed, ip)

    cases = []
    inf = np.full(nq, np.inf, np.float32)
    for ip in (False, True):
        every = -inf if ip else inf
        v = s
        cases.append(("flat ip %s" % ip, ip, lambda a, ip=ip: pq.adc_ip_range_lists_device(cd, t, od, pd, a["thr"], allow=a["w"])
                      if ip else pq.adc_range_lists_device(cd, t, od, pd, a["thr"], allow=a["w"]),
                      lambda thr, al, ip=ip: ref_range_lists(s, off, pr, thr, ip=ip, allow=al),
                      pick(ref_range_lists(v, off, full, every, ip=ip), 8885, ip)))
    vs = scaled(s, sc)
    cases.append(("flat ip scaled", True, lambda a: pq.adc_ip_range_lists_device(cd, t, od, pd, a["thr"], scales=scd, allow=a["w"]),
                  lambda thr, al: ref_range_lists(vs, off, pr, thr, ip=True, allow=al),
                  pick(ref_range_lists(vs, off, full, -inf, ip=True), 8886, True)))
    cases.append(("residual l2", False,
                  lambda a: pq.adc_range_lists_residual_device(cd, t, od, pd, bd, td, a["thr"], allow=a["w"]),
                  lambda thr, al: ref_range_residual(s, off, pr, bias, thr, terms=terms, allow=al),
                  pick(ref_range_residual(s, off, full, zero_bias, inf, terms=terms), 8887, False)))
    for name, scl, scl_d in (("residual ip", None, None), ("residual ip scaled", sc, scd)):
        cases.append((name, True,
                      lambda a, scl_d=scl_d: pq.adc_ip_range_lists_residual_device(cd, t, od, pd, bd, a["thr"], scales=scl_d, allow=a["w"]),
                      lambda thr, al, scl=scl: ref_range_residual(s, off, pr, bias, thr, scales=scl, ip=True, allow=al),
                      pick(ref_range_residual(s, off, full, zero_bias, -inf, scales=scl, ip=True), 8888, True)))
    ra.launch_log(reset=True)
    assert check_codes(pq) == _lib.OK
    try:
        for G in (1, 2, 5, 64, 0):
            ra.set_option("adc_range_wgs_per_query", G)
            for name, ip, run, ref, thr in cases:
                for al, w in ((None, None), (allow, wd)):
                    got = run({"thr": thr, "w": w})
                    want = ref(thr, al)
                    same(got, want, "%s, G %d, masked %s" % (name, G, al is not None))
                    assert (got[2] < n).all() and (got[2] >= 0).all()
                    assert check_codes(pq) == (_lib.ECODE_RANGE if bad_id else _lib.OK)
    finally:
        ra.set_option("adc_range_wgs_per_query", 0)
    log = ra.launch_log(reset=True)
    for k in ("k_adc_lists_plan", "k_adc_range_lists_u8", "k_adc_ip_range_lists_u8", "k_adc_range_lists_residual_u8",
              "k_adc_ip_range_lists_residual_u8", "k_adc_range_scan"):
        assert k in log, (k, log)
    assert "k_adc_search" not in log, log
    if n_probe == 3:
        # a capacity below the total: the true lims and a valid prefix, canaries intact; and a pure count call
        thr = cases[0][4]
        wl, wv, wi = ref_range_lists(s, off, pr, thr)
        total = int(wl[-1])
        assert total > 10
        for cap in (total // 2, total - 1):
            lims, v, i = call_raw(pq, fn_name(False, lists=True), cd, t, thr, cap, lists=(od, pd))
            assert np.array_equal(lims, wl) and np.array_equal(i, wi[:cap]) and v.tobytes() == wv[:cap].tobytes()
        lims, v, i = call_raw(pq, fn_name(True, lists=True, residual=True), cd, t, cases[-1][4], 0, lists=(od, pd), bias=bd,
                              extra=scd, has_extra=True, null_out=True)
        assert np.array_equal(lims, ref_range_residual(s, off, pr, bias, cases[-1][4], scales=sc, ip=True)[0])
        check_codes(pq)
        # a list named twice returns its rows twice
        twice = torch.tensor([[11, 5, 11]] * nq, dtype=torch.int64, device="cuda")
        same(pq.adc_range_lists_device(cd, t, od, twice, thr), ref_range_lists(s, off, twice.cpu().numpy(), thr), "a list named twice")
        # n_lists == 0 and n_codes == 0 write all-zero lims
        lims, v, i = call_raw(pq, fn_name(False, lists=True), cd[:0], t, thr, 4, lists=(od, pd))
        assert lims.tolist() == [0] * (nq + 1)
        lims, v, i = call_raw(pq, fn_name(False, lists=True), cd, t, thr, 4, lists=(od[:1], pd))
        assert lims.tolist() == [0] * (nq + 1)
    check_codes(pq)                                            # leave the stream's flag clear


@pytest.mark.gpu
@pytest.mark.parametrize("n_probe", [1, 16])
def test_gpu_range_lists_do_not_read_disallowed_rows(ra, n_probe):
    """the list kernels test the mask bit before they fetch: with a code >= K, a NaN row term and a NaN scale in EVERY
    disallowed row of every list, the masked result is that of the clean inputs and the range flag stays clear
    (K = 200, so a code 255 is out of range; no bad probe, so nothing else raises the flag)"""
    import torch
    from reductive_amd import _lib
    M, K, nq, n, n_lists = 15, 200, 5, 4000, 16
    pq = make_pq(ra, M, K)
    t = draw_tables(8900, nq, M, K)
    codes = synth.codes_u8(8901, (n, M), K)
    assert codes.max() < K
    off = lists_setup(8902, n, n_lists)
    rng = np.random.default_rng(8903 + n_probe)
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    pr[0, 0] = 11                                              # the long list
    bias = rng.standard_normal(pr.shape).astype(np.float32)
    terms = rng.standard_normal(n).astype(np.float32)
    sc = (synth.uniform01(8904, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    allow = rng.random(n) < 0.5
    allow[off[11]:off[11] + 64] = False                        # a whole wave trip of disallowed rows
    bad_codes, bad_terms, bad_sc = codes.copy(), terms.copy(), sc.copy()
    bad_codes[~allow, 3] = 255
    bad_terms[~allow] = np.nan
    bad_sc[~allow] = np.nan
    s = scan(pq, torch.from_numpy(codes).cuda(), t)            # the clean inputs feed the reference
    cd = torch.from_numpy(bad_codes).cuda()                    # the poisoned ones the calls
    od, pd, bd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda(), torch.from_numpy(bias).cuda()
    td, scd, wd = torch.from_numpy(bad_terms).cuda(), torch.from_numpy(bad_sc).cuda(), dev_words(allow)
    inf = np.full(nq, np.inf, np.float32)

    def middle(csr):
        """per query the median of its allowed probed values: about half of them qualify"""
        lims, v, _ = csr
        return np.array([np.median(v[lims[q]:lims[q + 1]]) if lims[q + 1] > lims[q] else 0.0 for q in range(nq)], np.float32)

    cases = [("residual l2", lambda thr: pq.adc_range_lists_residual_device(cd, t, od, pd, bd, td, thr, allow=wd),
              lambda thr: ref_range_residual(s, off, pr, bias, thr, terms=terms, allow=allow), inf),
             ("residual ip scaled", lambda thr: pq.adc_ip_range_lists_residual_device(cd, t, od, pd, bd, thr, scales=scd, allow=wd),
              lambda thr: ref_range_residual(s, off, pr, bias, thr, scales=sc, ip=True, allow=allow), -inf),
             ("residual ip", lambda thr: pq.adc_ip_range_lists_residual_device(cd, t, od, pd, bd, thr, allow=wd),
              lambda thr: ref_range_residual(s, off, pr, bias, thr, ip=True, allow=allow), -inf),
             ("flat ip scaled", lambda thr: pq.adc_ip_range_lists_device(cd, t, od, pd, thr, scales=scd, allow=wd),
              lambda thr: ref_range_lists(scaled(s, sc), off, pr, thr, ip=True, allow=allow), -inf),
             ("flat l2", lambda thr: pq.adc_range_lists_device(cd, t, od, pd, thr, allow=wd),
              lambda thr: ref_range_lists(s, off, pr, thr, allow=allow), inf)]
    assert check_codes(pq) == _lib.OK
    try:
        for G in (0, 5):
            ra.set_option("adc_range_wgs_per_query", G)
            for name, run, ref, every in cases:
                thr = middle(ref(every))
                want = ref(thr)
                assert 0 < want[0][-1] < ref(every)[0][-1], name   # some rows qualify and some do not
                got = run(thr)
                same(got, want, "%s, G %d" % (name, G))
                assert not np.isnan(got[1].cpu().numpy()).any()
                assert allow[got[2].cpu().numpy()].all()
                assert check_codes(pq) == _lib.OK, name        # no disallowed row was read
    finally:
        ra.set_option("adc_range_wgs_per_query", 0)
        check_codes(pq)                                        # leave the stream's flag clear


# ---- status codes that need a codebook handle ------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_range_status_codes_and_precedence(ra):
    import torch
    from reductive_amd import _lib
    M, K, nq, n = 15, 256, 2, 100
    pq = make_pq(ra, M, K)
    t = draw_tables(8890, nq, M, K)
    cd = torch.from_numpy(synth.codes_u8(8891, (n, M), K)).cuda()
    thr = np.zeros(nq, np.float32)
    od = torch.tensor([0, 50, 100], dtype=torch.int64, device="cuda")
    pd = torch.zeros((nq, 1), dtype=torch.int64, device="cuda")
    for name, kw in ((fn_name(False), {}), (fn_name(True), dict(has_extra=True)), (fn_name(False, lists=True), dict(lists=(od, pd))),
                     (fn_name(True, lists=True), dict(lists=(od, pd), has_extra=True))):
        call_raw(pq, name, cd, t, thr, 8, want_rc=_lib.OK, **kw)
        call_raw(pq, name, cd, t, thr, 8, code_bytes=4, want_rc=_lib.EUNSUPPORTED, **kw)
        call_raw(pq, name, cd, t, thr, 8, c_rs=M - 1, want_rc=_lib.ESHAPE, **kw)
        call_raw(pq, name, cd, t, thr, 8, code_bytes=4, c_rs=M - 1, want_rc=_lib.EUNSUPPORTED, **kw)   # the scope before the shape
        call_raw(pq, name, cd, t, thr, 8, null_out=True, want_rc=_lib.EINVAL, **kw)                    # null outputs, capacity > 0
        call_raw(pq, name, cd, t, thr, 8, null_out=True, c_rs=M - 1, want_rc=_lib.EINVAL, **kw)        # null pointers before the shape
    L = _lib.lib()
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lims = torch.full((nq + 1,), SENT_I, dtype=torch.int64, device="cuda")
    td = torch.zeros(nq, dtype=torch.float32, device="cuda")
    head = (pq._cb(), 0, t.data_ptr(), nq, cd.data_ptr(), 1, n, M, None)
    assert L.pqhip_adc_range_f32_dev(*head, td.data_ptr(), lims.data_ptr(), None, None, -1, z) == _lib.EINVAL
    assert L.pqhip_adc_range_f32_dev(*head, td.data_ptr(), None, None, None, 0, z) == _lib.EINVAL
    assert L.pqhip_adc_range_f32_dev(*head, None, lims.data_ptr(), None, None, 0, z) == _lib.EINVAL
    assert L.pqhip_adc_range_f32_dev(pq._cb(), 7, *head[2:], td.data_ptr(), lims.data_ptr(), None, None, 0, z) == _lib.ENODEV
    assert L.pqhip_adc_range_f32_dev(pq._cb(), 7, *head[2:5], 4, *head[6:], td.data_ptr(), lims.data_ptr(), None, None, 0, z) == _lib.ENODEV
    ra.launch_log(reset=True)
    assert L.pqhip_adc_range_f32_dev(pq._cb(), 0, None, 0, None, 1, n, M, None, None, None, None, None, 0, z) == _lib.OK
    assert ra.launch_log(reset=True) == ""                     # n_queries == 0 launches nothing
    assert (lims.cpu().numpy() == SENT_I).all()                # and nothing was written so far
    for opt in ("adc_range_wgs", "adc_range_wgs_per_query"):
        ra.set_option(opt, 0)


# ---- qmatrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_qmatrix_within_and_similar_above(ra):
    import torch
    from reductive_amd.qmatrix import QuantizedMatrix
    M, K, dsub, n, nq, n_lists = 6, 32, 4, 3000, 4, 8
    q = synth.normalish(8895, (M, K, dsub))
    pq = ra.Pq(None, q)
    x = synth.normalish(8896, (n, M * dsub))
    codes = pq.quantize_batch_device(torch.from_numpy(x).cuda()).cpu().numpy()
    norms = (synth.uniform01(8897, (n,)) + np.float32(0.5)).astype(np.float32)
    qm = QuantizedMatrix(pq, codes, norms)
    qd = torch.from_numpy(synth.normalish(8898, (nq, M * dsub))).cuda()
    dist = qm.distances(qd).cpu().numpy()
    sims = qm.inner_products(qd).cpu().numpy()
    radius = np.sort(dist, 1)[:, 40].copy()                    # about 40 rows per query
    level = -np.sort(-sims, 1)[:, 25].copy()
    allow = np.random.default_rng(8899).random(n) < 0.5
    for al in (None, allow):
        same(qm.within(qd, radius, allow=al), ref_range(dist, radius, allow=al), "within")
        same(qm.similar_above(qd, level, allow=al), ref_range(sims, level, ip=True, allow=al), "similar_above")
    lims, d, idx = qm.within(qd, radius, sort=True)
    lims, d, idx = lims.cpu().numpy(), d.cpu().numpy(), idx.cpu().numpy()
    for qi in range(nq):
        seg = slice(lims[qi], lims[qi + 1])
        order = np.lexsort((np.arange(n), dist[qi]))
        want = order[:lims[qi + 1] - lims[qi]]
        assert np.array_equal(idx[seg], want) and d[seg].tobytes() == dist[qi, want].tobytes()
    lims, sc, idx = qm.similar_above(qd[0], float(level[0]), sort=True)
    assert tuple(lims.shape) == (2,) and (np.diff(sc.cpu().numpy()) <= 0).all()
    assert int(lims[1]) == int((sims[0] >= level[0]).sum()) >= 26
    # partitioned: indices are original rows; with every list probed the set per query is the exhaustive one
    pm = qm.partition(n_lists, n_iterations=3, rng=np.random.default_rng(1))
    for al in (None, allow):
        for name, thr, ip, values in (("within", radius, False, dist), ("similar_above", level, True, sims)):
            lims, v, rows = [a.cpu().numpy() for a in getattr(pm, name)(qd, thr, n_lists, allow=al)]
            wl, wv, wi = ref_range(values, thr, ip=ip, allow=al)
            assert np.array_equal(lims, wl)
            for qi in range(nq):
                seg = slice(lims[qi], lims[qi + 1])
                o = np.argsort(rows[seg], kind="stable")
                assert np.array_equal(rows[seg][o], wi[seg]) and v[seg][o].tobytes() == wv[seg].tobytes()
    lims, v, rows = pm.within(qd, radius, 2, sort=True)
    v = v.cpu().numpy()
    lims = lims.cpu().numpy()
    probed = pm.probes(qd, 2).cpu().numpy()
    assign = np.empty(n, np.int64)
    off = pm.list_off.cpu().numpy()
    ids = pm.ids.cpu().numpy()
    for l in range(n_lists):
        assign[ids[off[l]:off[l + 1]]] = l
    for qi in range(nq):
        seg = slice(lims[qi], lims[qi + 1])
        assert (np.diff(v[seg]) >= 0).all()
        want = np.flatnonzero(np.isin(assign, probed[qi]) & (dist[qi] <= radius[qi]))
        assert sorted(rows.cpu().numpy()[seg].tolist()) == want.tolist()
    # residual codes: the values are those of nearest() / most_similar() with every row requested
    rm = qm.partition_residual(n_lists, n_iterations=3, pq_iterations=2, rng=np.random.default_rng(2))
    for name, topk, ip in (("within", "nearest", False), ("similar_above", "most_similar", True)):
        tv, ti = [a.cpu().numpy() for a in getattr(rm, topk)(qd, 60, 3)]
        thr = tv[:, 30].copy()
        for al in (None, allow):
            if al is not None:
                tv, ti = [a.cpu().numpy() for a in getattr(rm, topk)(qd, 60, 3, allow=al)]
                thr = tv[:, 30].copy()
            lims, v, rows = [a.cpu().numpy() for a in getattr(rm, name)(qd, thr, 3, allow=al, sort=True)]
            for qi in range(nq):
                seg = slice(lims[qi], lims[qi + 1])
                c = lims[qi + 1] - lims[qi]
                assert 31 <= c <= 60
                assert sorted(rows[seg].tolist()) == sorted(ti[qi, :c].tolist())
                assert np.array_equal(v[seg] + np.float32(0), tv[qi, :c])          # the searches return a zero as +0
                if al is not None:
                    assert al[rows[seg]].all()
