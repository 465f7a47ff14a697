"""Masked ADC searches on the GPU (include/pqhip.h: pqhip_adc_*search*_masked_f32_dev, pqhip_pack_row_mask_dev) and
qmatrix.RowFilter on top.  Reference: tests/adc_masked_ref.py (pinned by test_adc_masked.py) -- the unmasked references
on the allowed rows alone, indices mapped back.  Through the C entry points with padded row strides and sentinels
around the outputs: indices exactly, values bit for bit (NaN as NaN), padding from |A| on, no index of a disallowed row
or at or beyond n, a NULL mask being the unmasked call (outputs and launch log), disallowed rows never read (a code
>= K or a NaN row term there changes nothing), one result for every number of workgroups per query."""
import ctypes

import numpy as np
import pytest

import synth
from adc_ip_ref import scores
from adc_masked_ref import pack_ref, ref_masked_lists_search, ref_masked_residual_search, ref_masked_search
from oracle import pq_oracle as orc

OPTION = "adc_lists_wgs_per_query"
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


def dev_words(words):
    import torch
    w = np.ascontiguousarray(np.asarray(words, np.uint32))
    if w.size == 0:
        return torch.zeros(1, dtype=torch.int32, device="cuda")[:0]
    return torch.from_numpy(w.view(np.int32).copy()).cuda()


def call_raw(pq, name, codes, tables, words, k, lists=None, bias=None, extra=None, has_extra=False, pad=3, want_rc=0):
    """A masked (or, with words=False, the unmasked) C entry point with row strides k + pad and sentinels around the
    outputs; checks the sentinels and returns (value, idx) as numpy [nq, k].  words: device int32 tensor, None (a NULL
    mask) or False (the entry point without the mask argument).  lists: (list_off, probes) device tensors."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n, M = codes.shape
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device=codes.device)
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream
    args = [pq._cb(), pq._slot_for(codes), tables.data_ptr(), nq, codes.data_ptr(), codes.element_size(), n,
            codes.stride(0) if n > 1 else max(codes.stride(0), M)]
    if words is not False:
        args.append(None if words is None else words.data_ptr())
    if lists is not None:
        lo, pr = lists
        args += [lo.data_ptr(), lo.shape[0] - 1, pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else max(pr.stride(0), pr.shape[1])]
        if bias is not None:
            args += [bias.data_ptr(), bias.stride(0) if nq > 1 else max(bias.stride(0), pr.shape[1])]
    if has_extra:
        args.append(extra.data_ptr() if extra is not None else None)
    args += [k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, ctypes.c_void_p(stream)]
    rc = getattr(_lib.lib(), name)(*args)
    assert rc == want_rc, (name, rc)
    if rc != _lib.OK:
        return None
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    v = np.stack([vb[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    i = np.stack([ib[pad + q * rs: pad + q * rs + k] for q in range(nq)])
    return v, i


def fn_name(ip, lists=False, residual=False, masked=True):
    return "pqhip_adc_%ssearch_%s%s%sf32_dev" % ("ip_" if ip else "", "lists_" if lists else "", "residual_" if residual else "",
                                                 "masked_" if masked else "")


def assert_same(got, want_v, want_i, allow=None, n=None):
    got_v, got_i = got
    print("rows returned per query: got %s want %s" % ((got_i >= 0).sum(1).tolist(), (want_i >= 0).sum(1).tolist()))
    assert np.array_equal(got_i, want_i)
    gn, wn = np.isnan(got_v), np.isnan(want_v)
    assert np.array_equal(gn, wn)
    assert (got_v[gn].view(np.uint32) == 0x7fc00000).all()
    assert got_v[~gn].tobytes() == np.asarray(want_v, np.float32)[~wn].tobytes()
    if allow is not None:
        live = got_i[got_i >= 0]
        assert (live < n).all() and allow[live].all()


def check_codes(pq):
    import torch
    from reductive_amd import _lib
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def make_masks(seed, n):
    """[(name, allow bool [n], words uint32)]: all ones, all zeros, only row 0, only row n - 1, alternating bits, random
    of density 0.5 and 0.01, seven rows (fewer than most k), and a random one whose last word has every bit at or beyond
    n set"""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, a, tail=False):
        w = pack_ref(a)
        if tail and n % 32:
            w = w.copy()
            w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
        out.append((name, a, w))
    add("ones", np.ones(n, bool))
    add("zeros", np.zeros(n, bool))
    a = np.zeros(n, bool)
    a[0] = True
    add("row 0", a)
    a = np.zeros(n, bool)
    a[n - 1] = True
    add("row n-1", a)
    add("alternating", (np.arange(n) & 1).astype(bool))
    add("random 0.5", rng.random(n) < 0.5)
    add("random 0.01", rng.random(n) < 0.01)
    a = np.zeros(n, bool)
    a[rng.choice(n, min(7, n), replace=False)] = True
    add("seven rows", a)
    add("tail bits set", rng.random(n) < 0.5, tail=True)
    add("ones, tail bits set", np.ones(n, bool), tail=True)
    return out


# ---- the pack kernel -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pack_row_mask(ra):
    import torch
    from reductive_amd import _lib
    pq = ra.Pq(None, synth.normalish(9960, (3, 7, 2)))
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(9961)
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 1023, 1025, 100003):
        for with_perm in (False, True):
            n_src = n + 5 if with_perm else n
            allow = rng.random(n_src) < 0.5
            perm = rng.permutation(n_src)[:n].astype(np.int64) if with_perm else None
            want = pack_ref(allow[:n] if perm is None else allow, perm)
            ad = torch.from_numpy(allow).cuda()
            pd = None if perm is None else torch.from_numpy(perm).cuda()
            # the wrapper, with bool and with uint8 flags
            for a in (ad, ad.to(torch.uint8) * 3):
                got = pq.pack_row_mask_device(a[:n] if perm is None else a, perm=pd, check=True)
                assert got.dtype == torch.int32 and tuple(got.shape) == ((n + 31) // 32,)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (n, with_perm)
            # the C entry point over a buffer of all ones with a sentinel word on each side: the tail bits come back 0
            nw = (n + 31) // 32
            buf = torch.full((nw + 2,), -1, dtype=torch.int32, device="cuda")
            a8 = ad.view(torch.uint8) if n_src else torch.zeros(1, dtype=torch.uint8, device="cuda")
            rc = L.pqhip_pack_row_mask_dev(pq._cb(), 0, a8.data_ptr(), n_src, pd.data_ptr() if pd is not None and n else None, n,
                                           buf.data_ptr() + 4, ctypes.c_void_p(stream))
            assert rc == _lib.OK
            b = buf.cpu().numpy().view(np.uint32)
            assert b[0] == 0xffffffff and b[-1] == 0xffffffff and np.array_equal(b[1:-1], want), (n, with_perm)
            if n % 32:
                assert b[nw] >> (n % 32) == 0
            assert check_codes(pq) == _lib.OK
    # a perm entry of -1 and one of n_src each clear their bit and raise the range flag
    n = 100
    ad = torch.ones(n, dtype=torch.bool, device="cuda")
    for bad in (-1, n):
        perm = np.arange(n, dtype=np.int64)
        perm[37] = bad
        got = pq.pack_row_mask_device(ad, perm=torch.from_numpy(perm).cuda())
        want = np.ones(n, bool)
        want[37] = False
        assert np.array_equal(got.cpu().numpy().view(np.uint32), pack_ref(want))
        assert check_codes(pq) == _lib.ECODE_RANGE
        assert check_codes(pq) == _lib.OK
        with pytest.raises(ra.PanicError, match="index out of bounds"):
            pq.pack_row_mask_device(ad, perm=torch.from_numpy(perm).cuda(), check=True)
    ra.launch_log(reset=True)
    z = ctypes.c_void_p(stream)
    assert L.pqhip_pack_row_mask_dev(pq._cb(), 0, None, 0, None, 0, None, z) == _lib.OK      # n == 0 launches nothing
    assert ra.launch_log(reset=True) == ""
    assert L.pqhip_pack_row_mask_dev(pq._cb(), 0, ad.data_ptr(), n, None, -1, ad.data_ptr(), z) == _lib.EINVAL
    assert L.pqhip_pack_row_mask_dev(pq._cb(), 0, None, n, None, n, ad.data_ptr(), z) == _lib.EINVAL
    assert L.pqhip_pack_row_mask_dev(pq._cb(), 0, ad.data_ptr(), n, None, n, None, z) == _lib.EINVAL
    assert L.pqhip_pack_row_mask_dev(pq._cb(), 7, ad.data_ptr(), n, None, n, ad.data_ptr(), z) == _lib.ENODEV


# ---- exhaustive searches -----------------------------------------------------------------------------------------
QK = [(1, 10), (8, 1), (8, 100), (5, 200), (2, 300), (1, 1024)]     # 8 / 4 / 1 queries per pass, L = 1 .. 16


def exhaustive_setup(ra, M, K, n):
    import torch
    dsub = 2
    q = synth.normalish(9970 + M, (M, K, dsub))
    pq = ra.Pq(None, q)
    yd = torch.from_numpy(synth.normalish(9971 + M, (8, M * dsub))).cuda()
    t_l2, t_ip = pq.adc_tables_device(yd).clone(), pq.adc_ip_tables_device(yd).clone()
    if K == 256:                                   # a few non-finite and signed-zero entries: NaN, +-Inf, -0 rows
        for t in (t_l2, t_ip):
            t[1, 2, 5], t[2, 0, 9], t[3, 7, 200], t[4, 1, 17] = float("nan"), float("inf"), float("-inf"), -0.0
    codes = synth.codes_u8(9972 + n, (n, M), K)
    sc = (synth.uniform01(9973 + n, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)    # some negative
    with np.errstate(invalid="ignore"):
        dist = orc.adc_scan(t_l2.cpu().numpy(), codes)
        ipsum = orc.adc_scan(t_ip.cpu().numpy(), codes)
    return pq, t_l2, t_ip, codes, torch.from_numpy(codes).cuda(), sc, torch.from_numpy(sc).cuda(), dist, ipsum


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(15, 256), (3, 7)])
@pytest.mark.parametrize("n", [1, 33, 1025, 20011])
def test_gpu_masked_search_matches_reference(ra, M, K, n):
    """Distance, inner product and scaled inner product under every mask of make_masks, for every (queries, k) of QK.
    n = 20,011 is beyond one workgroup's range of 4,096 rows: several partial lists are merged."""
    import torch
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = exhaustive_setup(ra, M, K, n)
    if n == 20011:
        n_cus = torch.cuda.get_device_properties(0).multi_processor_count
        rows_per_wg = max(-(-(-(-n // n_cus)) // 1024) * 1024, 4096)
        assert -(-n // rows_per_wg) >= 2                     # the launch configuration of adc_search: a grid of several workgroups
    forms = [(False, t_l2, None, dist), (True, t_ip, None, scores(ipsum)), (True, t_ip, scd, scores(ipsum, sc))]
    ra.launch_log(reset=True)
    for name, allow, words in make_masks(9974 + n, n):
        wd = dev_words(words)
        for ip, t, scales, values in forms:
            sdev = scales
            if scales is not None and not allow.all():       # a NaN scale in a disallowed row is never read
                sdev = scales.clone()
                sdev[int(np.flatnonzero(~allow)[0])] = float("nan")
            for nq, k in QK:
                want_v, want_i = ref_masked_search(values[:nq], allow, k, ip=ip)
                print("mask %s, ip %s, scales %s, nq %d, k %d" % (name, ip, scales is not None, nq, k))
                got = call_raw(pq, fn_name(ip), cd, t[:nq].contiguous(), wd, k, extra=sdev, has_extra=ip)
                assert_same(got, want_v, want_i, allow, n)
                assert (want_i >= 0).sum(1).tolist() == [min(k, int(allow.sum()))] * nq
    log = ra.launch_log(reset=True)
    assert "k_adc_search_masked_u8" in log and "k_adc_ip_search_masked_u8" in log and "k_adc_search_merge" in log, log
    assert "k_adc_search_u8" not in log and "k_adc_ip_search_u8" not in log and "k_adc_search_any" not in log, log
    assert "k_adc_search_masked_u8_mq<8 queries>" in log and "k_adc_search_masked_u8_mq<4 queries>" in log, log
    # the Python entry point: 3-D and 2-D tables
    name, allow, words = make_masks(9974 + n, n)[5]
    wd = dev_words(words)
    d, i = pq.adc_search_device(cd, t_l2, 10, allow=wd, check=True)
    assert_same((d.cpu().numpy(), i.cpu().numpy()), *ref_masked_search(dist, allow, 10), allow, n)
    s, i = pq.adc_ip_search_device(cd, t_ip[3].contiguous(), 10, scales=scd, allow=wd, check=True)
    assert tuple(s.shape) == (10,)
    assert_same((s[None].cpu().numpy(), i[None].cpu().numpy()), *ref_masked_search(scores(ipsum, sc)[3], allow, 10, ip=True), allow, n)


@pytest.mark.gpu
def test_gpu_null_mask_is_the_unmasked_call(ra):
    """d_allow == NULL: outputs and launch log of the unmasked entry points, for all six"""
    import torch
    n, n_lists, nq = 5003, 13, 5
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = exhaustive_setup(ra, 15, 256, n)
    t_l2, t_ip = t_l2[:nq].contiguous(), t_ip[:nq].contiguous()
    lo = torch.from_numpy(np.linspace(0, n, n_lists + 1).astype(np.int64)).cuda()
    pr = torch.from_numpy(np.stack([np.random.default_rng(9975 + q).permutation(n_lists)[:4] for q in range(nq)])).cuda()
    bias = torch.from_numpy(synth.normalish(9976, (nq, 4))).cuda()
    cases = [(False, False, False, t_l2, None, False), (True, False, False, t_ip, scd, True),
             (False, True, False, t_l2, None, False), (True, True, False, t_ip, scd, True),
             (False, True, True, t_ip, scd, True), (True, True, True, t_ip, scd, True)]
    for ip, lists, residual, t, extra, has_extra in cases:
        kw = dict(lists=(lo, pr) if lists else None, bias=bias if residual else None, extra=extra, has_extra=has_extra)
        for k in (10, 200):
            ra.launch_log(reset=True)
            a = call_raw(pq, fn_name(ip, lists, residual), cd, t, None, k, **kw)
            log_a = ra.launch_log(reset=True)
            b = call_raw(pq, fn_name(ip, lists, residual, masked=False), cd, t, False, k, **kw)
            log_b = ra.launch_log(reset=True)
            assert log_a == log_b and "masked" not in log_a and log_a != "", (log_a, log_b)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.gpu
def test_gpu_masked_search_scope_and_status(ra):
    """A mask with 4-byte codes or a table beyond LDS: PQHIP_EUNSUPPORTED, never another path; precedence as unmasked."""
    import torch
    from reductive_amd import _lib
    n = 100
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = exhaustive_setup(ra, 15, 256, n)
    wd = dev_words(pack_ref(np.ones(n, bool)))
    c32 = cd.to(torch.int32)
    for ip, t in ((False, t_l2), (True, t_ip)):
        call_raw(pq, fn_name(ip), c32, t, wd, 10, has_extra=ip, want_rc=_lib.EUNSUPPORTED)
        got = call_raw(pq, fn_name(ip), c32, t, None, 10, has_extra=ip)              # without a mask 4-byte codes are served
        assert_same(got, *(ref_masked_search(scores(ipsum) if ip else dist, np.ones(n, bool), 10, ip=ip)))
        call_raw(pq, fn_name(ip), cd, t, wd, 0, has_extra=ip, want_rc=_lib.EINVAL)
        call_raw(pq, fn_name(ip), cd, t, wd, 1025, has_extra=ip, want_rc=_lib.EUNSUPPORTED)
    big = ra.Pq(None, synth.normalish(9977, (48, 1024, 2)))          # 192 KB of table
    tb = big.adc_tables_device(torch.from_numpy(synth.normalish(9978, (2, 96))).cuda())
    c48 = torch.from_numpy(synth.codes_u8(9979, (n, 48), 256)).cuda()
    call_raw(big, fn_name(False), c48, tb, wd, 10, want_rc=_lib.EUNSUPPORTED)
    assert call_raw(big, fn_name(False), c48, tb, None, 10) is not None
    with pytest.raises(ra.PanicError):
        pq.adc_search_device(cd, t_l2, 10, allow=wd[:0])                              # words for another row count
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_disallowed_rows_are_not_read(ra):
    """A code >= K in a disallowed row: results unchanged and no range flag; the same code in an allowed row raises it.
    Exhaustive and list searches."""
    import torch
    from reductive_amd import _lib
    M, K, n, n_lists = 15, 200, 5003, 13
    pq = ra.Pq(None, synth.normalish(9980, (M, K, 2)))
    yd = torch.from_numpy(synth.normalish(9981, (4, M * 2))).cuda()
    t = pq.adc_tables_device(yd)
    codes = synth.codes_u8(9982, (n, M), K)
    allow = np.random.default_rng(9983).random(n) < 0.5
    off_row, on_row = int(np.flatnonzero(~allow)[40]), int(np.flatnonzero(allow)[40])
    wd = dev_words(pack_ref(allow))
    lo = torch.from_numpy(np.linspace(0, n, n_lists + 1).astype(np.int64)).cuda()
    pr = torch.arange(n_lists, dtype=torch.int64, device="cuda")[None].expand(4, -1).contiguous()
    dist = orc.adc_scan(t.cpu().numpy(), codes)
    want = ref_masked_search(dist, allow, 50)
    for lists in (None, (lo, pr)):
        name = fn_name(False, lists is not None)
        bad = codes.copy()
        bad[off_row, 3] = K
        assert_same(call_raw(pq, name, torch.from_numpy(bad).cuda(), t, wd, 50, lists=lists), *want, allow, n)
        assert check_codes(pq) == _lib.OK
        bad = codes.copy()
        bad[on_row, 3] = K
        call_raw(pq, name, torch.from_numpy(bad).cuda(), t, wd, 50, lists=lists)
        assert check_codes(pq) == _lib.ECODE_RANGE
        assert check_codes(pq) == _lib.OK


# ---- list searches ---------------------------------------------------------------------------------------------------
LISTS_N, LISTS_NL, LISTS_NQ = 5003, 37, 4


def lists_layout():
    """37 lists over 5,003 rows: empty lists, one-row lists and lists shorter than 32 rows, so that one mask word spans
    several lists; the rest uneven"""
    rng = np.random.default_rng(9984)
    sizes = [0, 1, 1, 5, 0, 31, 3, 17, 1, 0, 9, 2]
    rest = LISTS_N - sum(sizes)
    cuts = np.sort(rng.integers(0, rest + 1, LISTS_NL - len(sizes) - 1))
    sizes += np.diff(np.concatenate([[0], cuts, [rest]])).tolist()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off.size == LISTS_NL + 1 and off[-1] == LISTS_N
    return off


def lists_probes(seed, n_probe):
    """every list of a row once, -1 padding at a fifth of the slots"""
    rng = np.random.default_rng(seed)
    pr = np.stack([rng.permutation(LISTS_NL)[:n_probe] for _ in range(LISTS_NQ)]).astype(np.int64)
    if n_probe > 1:
        pr[rng.random(pr.shape) < 0.2] = -1
    return pr


@pytest.fixture(scope="module")
def lists_data(ra):
    import torch
    pq, t_l2, t_ip, codes, cd, sc, scd, dist, ipsum = exhaustive_setup(ra, 15, 256, LISTS_N)
    nq = LISTS_NQ
    terms = (synth.normalish(9985, (LISTS_N,)) * np.float32(2.0) + np.float32(1.0)).astype(np.float32)
    return dict(pq=pq, t_l2=t_l2[:nq].contiguous(), t_ip=t_ip[:nq].contiguous(), cd=cd, sc=sc, terms=terms, dist=dist[:nq],
                ipsum=ipsum[:nq], off=lists_layout())


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("G", [1, 2, 7, 0])
def test_gpu_masked_lists_search_matches_reference(ra, lists_data, G, residual):
    """Distance, inner product and scaled inner product over probed lists (residual: with probe biases and row terms)
    under every mask, n_probe in {1, 5, 37} with -1 padding, forced workgroups per query 1, 2, 7 and auto."""
    import torch
    D = lists_data
    pq, cd, off, n = D["pq"], D["cd"], D["off"], LISTS_N
    lo = torch.from_numpy(off).cuda()
    try:
        ra.set_option(OPTION, G)
        ra.launch_log(reset=True)
        for n_probe in (1, 5, 37):
            probes = lists_probes(9986 + n_probe, n_probe)
            pr = torch.from_numpy(probes).cuda()
            b = (synth.normalish(9987 + n_probe, probes.shape) * np.float32(3.0)).astype(np.float32)
            bias = torch.from_numpy(b).cuda()
            masks = make_masks(9988, n)
            l0 = int(probes[0][probes[0] >= 0][0]) if (probes[0] >= 0).any() else 0
            a = np.ones(n, bool)
            a[off[l0]:off[l0 + 1]] = False
            masks.append(("a probed list cleared", a, pack_ref(a)))
            a = np.zeros(n, bool)                                       # three rows left in every list that has them
            for l in range(LISTS_NL):
                a[off[l]:min(off[l] + 3, off[l + 1])] = True
            masks.append(("fewer than k rows in S_q", a, pack_ref(a)))
            for name, allow, words in masks:
                wd = dev_words(words)
                for ip, scaled in ((False, False), (True, False), (True, True)):
                    ex = None
                    if residual and not ip:
                        ex = D["terms"].copy()
                    elif scaled:
                        ex = D["sc"].copy()
                    exd = None
                    if ex is not None:
                        exd = ex.copy()
                        exd[np.flatnonzero(~allow)[:5]] = np.nan        # a NaN row term / scale in a disallowed row changes nothing
                        exd = torch.from_numpy(exd).cuda()
                    for k in (10, 300):
                        print("G %d, n_probe %d, mask %s, ip %s, scaled %s, k %d" % (G, n_probe, name, ip, scaled, k))
                        if residual:
                            want = ref_masked_residual_search(D["ipsum"], allow, off, probes, b, k, terms=None if ip else ex,
                                                              scales=ex if ip else None, ip=ip)
                            got = call_raw(pq, fn_name(ip, True, True), cd, D["t_ip"], wd, k, lists=(lo, pr), bias=bias,
                                           extra=exd, has_extra=True)
                        else:
                            values = scores(D["ipsum"], ex) if ip else D["dist"]
                            want = ref_masked_lists_search(values, allow, off, probes, k, ip=ip)
                            got = call_raw(pq, fn_name(ip, True), cd, D["t_ip"] if ip else D["t_l2"], wd, k, lists=(lo, pr),
                                           extra=exd, has_extra=ip)
                        assert_same(got, *want, allow, n)
        log = ra.launch_log(reset=True)
        stem = "search_lists_residual_masked_u8" if residual else "search_lists_masked_u8"
        assert "k_adc_lists_plan" in log and "k_adc_" + stem in log and "k_adc_ip_" + stem in log, log
        assert "search_lists_u8" not in log and "search_lists_residual_u8" not in log and "k_adc_search_u8" not in log, log
    finally:
        ra.set_option(OPTION, 0)
    # the Python entry points
    probes = lists_probes(9989, 5)
    pr = torch.from_numpy(probes).cuda()
    name, allow, words = make_masks(9988, n)[5]
    wd = dev_words(words)
    if residual:
        b = synth.normalish(9990, probes.shape)
        d, i = pq.adc_search_lists_residual_device(cd, D["t_ip"], lo, pr, torch.from_numpy(b).cuda(), torch.from_numpy(D["terms"]).cuda(),
                                                   10, allow=wd, check=True)
        want = ref_masked_residual_search(D["ipsum"], allow, off, probes, b, 10, terms=D["terms"])
    else:
        d, i = pq.adc_search_lists_device(cd, D["t_l2"], lo, pr, 10, allow=wd, check=True)
        want = ref_masked_lists_search(D["dist"], allow, off, probes, 10)
    assert_same((d.cpu().numpy(), i.cpu().numpy()), *want, allow, n)


# ---- qmatrix ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(ra):
    """20,000 x 32 around 40 centres, M = 8, 4 bits, 64 lists: the flat matrix, its partition and its residual partition"""
    import torch
    from reductive_amd import qmatrix
    N, d, M, bits, n_lists, nq = 20000, 32, 8, 4, 64, 6
    rng = np.random.default_rng(9991)
    centres = (rng.standard_normal((40, d)) * 3.0).astype(np.float32)
    x = (centres[rng.integers(0, 40, N)] + rng.standard_normal((N, d))).astype(np.float32)
    ys = (x[rng.choice(N, nq, replace=False)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    flat = ra.train_pq(M, bits, 4, 1, x, rng=np.random.default_rng(9992))
    norms = (rng.random(N) + 0.5).astype(np.float32)
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x), norms)
    pm = qm.partition(n_lists, n_iterations=4, vectors=x, rng=np.random.default_rng(9993))
    rm = qm.partition_residual(n_lists, n_iterations=4, pq_iterations=4, vectors=x, rng=np.random.default_rng(9993))
    allow = rng.random(N) < 0.3
    return dict(x=x, yd=torch.from_numpy(ys).cuda(), qm=qm, pm=pm, rm=rm, allow=allow, N=N, n_lists=n_lists)


def _sub_matrices(T):
    """the three matrices built from the allowed rows alone, with the same quantizers, centroids and lists"""
    import torch
    from reductive_amd import qmatrix
    allow, qm, pm, rm = T["allow"], T["qm"], T["pm"], T["rm"]
    sel = torch.from_numpy(np.flatnonzero(allow)).cuda()
    off = pm.list_off.cpu().numpy()
    list_of_pos = np.searchsorted(off[1:], np.arange(T["N"]), side="right")
    assign = list_of_pos[pm.positions.cpu().numpy()]                     # the list of each original row
    sq = qmatrix.QuantizedMatrix(qm.pq, qm.codes[sel].cpu().numpy(), qm.norms[sel].cpu().numpy())
    sp = qmatrix.PartitionedMatrix(sq, pm.centroids, assign[allow])
    pos = rm.positions[sel]
    sr = qmatrix.ResidualPartitionedMatrix(rm.pq, rm.codes[pos].contiguous(), rm.norms[pos].contiguous(),
                                           rm.row_terms[pos].contiguous(), rm.centroids, assign[allow])
    return sq, sp, sr


@pytest.mark.gpu
def test_gpu_row_filter_on_all_three_matrices(ra, trained):
    """nearest / most_similar with allow= return allowed original rows only and equal the same call on a matrix built
    from the allowed rows alone (same quantizer, same lists), row numbers mapped back; a filter and flags packed on the
    spot agree; refine= re-ranks the filtered shortlist; a filter of another matrix is refused."""
    import torch
    from reductive_amd import qmatrix
    T = trained
    allow, yd, N = T["allow"], T["yd"], T["N"]
    rows = torch.from_numpy(np.flatnonzero(allow)).cuda()
    subs = _sub_matrices(T)
    ad = torch.from_numpy(allow).cuda()

    def back(idx):
        return torch.where(idx < 0, idx, rows[idx.clamp(min=0)])
    for full, sub in zip((T["qm"], T["pm"], T["rm"]), subs):
        f = full.row_filter(allow)
        assert isinstance(f, qmatrix.RowFilter) and f.matrix is full and f.n_allowed == int(allow.sum())
        perm = getattr(full, "ids", None)
        assert np.array_equal(f.words.cpu().numpy().view(np.uint32), pack_ref(allow, None if perm is None else perm.cpu().numpy()))
        f_rows = full.row_filter(rows=np.flatnonzero(allow))
        f_not = full.row_filter(rows=np.flatnonzero(~allow), allowed=False)
        assert torch.equal(f_rows.words, f.words) and torch.equal(f_not.words, f.words)
        for kw in ((dict(),) if full is T["qm"] else (dict(nprobe=1), dict(nprobe=8), dict(nprobe=T["n_lists"]))):
            for k in (10, 300):
                for q in (yd, yd[2]):
                    d, i = full.nearest(q, k, allow=f, **kw)
                    wd, wi = sub.nearest(q, k, **kw)
                    live = i[i >= 0]
                    assert ad[live].all()
                    assert torch.equal(i, back(wi)) and d.cpu().numpy().tobytes() == wd.cpu().numpy().tobytes()
                    for use_norms in (True, False):
                        s, i = full.most_similar(q, k, use_norms=use_norms, allow=f, **kw)
                        ws, wi = sub.most_similar(q, k, use_norms=use_norms, **kw)
                        assert ad[i[i >= 0]].all()
                        assert torch.equal(i, back(wi)) and s.cpu().numpy().tobytes() == ws.cpu().numpy().tobytes()
            d1, i1 = full.nearest(yd, 10, allow=allow, **kw)               # numpy flags packed on the spot
            d2, i2 = full.nearest(yd, 10, allow=ad, **kw)                  # torch flags
            d3, i3 = full.nearest(yd, 10, allow=f, **kw)
            assert torch.equal(i1, i3) and torch.equal(i2, i3) and torch.equal(d1, d3) and torch.equal(d2, d3)
        # refine= with allow=: the re-ranking of the filtered shortlist
        full.attach_vectors(T["x"])
        kw = dict() if full is T["qm"] else dict(nprobe=8)
        for ip in (False, True):
            search = full.most_similar if ip else full.nearest
            _, short = search(yd, 200, allow=f, **kw)
            want_v, want_i = full.pq.rerank_device(yd, full.vectors, short, 10, ip=ip)
            v, i = search(yd, 10, refine=200, allow=f, **kw)
            assert torch.equal(i, want_i) and torch.equal(v, want_v) and ad[i[i >= 0]].all()
        # a filter belongs to its matrix
        for other in (T["qm"], T["pm"], T["rm"]) + subs:
            if other is not full:
                with pytest.raises(ra.PanicError, match="another matrix"):
                    other.nearest(yd, 10, allow=f, **(dict() if isinstance(other, qmatrix.QuantizedMatrix) else dict(nprobe=2)))
    with pytest.raises(ra.PanicError):
        T["qm"].row_filter(allow[:-1])
    with pytest.raises(ra.PanicError):
        T["qm"].row_filter(rows=[N])
    with pytest.raises(ra.PanicError):
        T["qm"].row_filter()
