"""ADC search among given rows on the GPU (include/pqhip.h: pqhip_adc_among_f32_dev, pqhip_adc_ip_among_f32_dev).
References: tests/adc_among_ref.py (pinned by test_adc_among.py) AND the existing masked entry points run per query in
the same process.  Through the C entry points with padded output strides and sentinels around both outputs: indices
exactly, values bit for bit (NaN as the canonical NaN), the range flag after every call.  Every NV bucket edge (M), every
list length L (k), per-query lengths around the 64-lane, 1,024-place and 4,096-place edges mixed in one CSR, every order
of the ids, every number of workgroups per query; rows that are not named carry poison throughout."""
import ctypes

import numpy as np
import pytest

import synth
from adc_among_ref import candidates, ref_among
from adc_masked_ref import pack_ref
from oracle import pq_oracle as orc
from test_gpu_adc_masked import SENT_I, SENT_V, assert_same, call_raw, check_codes, dev_words, fn_name

OPTION = "adc_among_wgs_per_query"
LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
KS = [1, 64, 65, 128, 129, 257, 513, 1024]
GUARD = 64                      # valid-looking ids behind d_ids[0 .. n_ids) that must never be read


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda")[:0]
    return torch.from_numpy(a).cuda()


def among_raw(pq, ip, codes, tables, ids, k, lims=None, n_ids=None, row_list=None, bias=None, extra=None, n_lists=None, pad=3,
              want_rc=0, n=None):
    """The C entry point with output row strides k + pad and sentinels around both outputs -> (value, idx) numpy [nq, k].
    ids: device int64, its first n_ids entries are the call's (what follows is guard); codes may be a strided view."""
    import torch
    from reductive_amd import _lib
    nq = 1 if tables.dim() == 2 else tables.shape[0]
    n = codes.shape[0] if n is None else n
    M = codes.shape[1]
    n_ids = ids.shape[0] if n_ids is None else n_ids
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device="cuda")
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if bias is not None and n_lists is None:
        n_lists = bias.shape[1]
    name = "pqhip_adc_%samong_f32_dev" % ("ip_" if ip else "")
    rc = getattr(_lib.lib(), name)(
        pq._cb(), 0, tables.data_ptr(), nq, codes.data_ptr(), 1, n, codes.stride(0) if codes.shape[0] > 1 else max(codes.stride(0), M),
        None if lims is None else lims.data_ptr(), ids.data_ptr() if ids.shape[0] else None, n_ids,
        None if row_list is None else row_list.data_ptr(), n_lists or 0, None if bias is None else bias.data_ptr(),
        0 if bias is None else (bias.stride(0) if nq > 1 else max(bias.stride(0), n_lists)),
        None if extra is None else extra.data_ptr(), k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs,
        ctypes.c_void_p(stream))
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


def flag(pq, want):
    from reductive_amd import _lib
    assert check_codes(pq) == (_lib.ECODE_RANGE if want else _lib.OK)
    assert check_codes(pq) == _lib.OK


def integer_tables(rng, nq, M, K, special):
    """integer-valued entries, so that ties sit at the k-th place; special: NaN, +-Inf and -0 planted"""
    t = rng.integers(-2, 3, (nq, M, K)).astype(np.float32)
    if special:
        for value in (np.nan, np.inf, -np.inf, -0.0):
            for _ in range(2):
                t[rng.integers(nq), rng.integers(M), rng.integers(K)] = value
    return t


def draw_csr(rng, nq, n, order, start=0):
    """query q names LENGTHS[(start + q) mod 9] distinct rows (cut to n) in the given order, -1 padding sprinkled in"""
    lengths = LENGTHS[start:] + LENGTHS[:start]
    parts = []
    shuffle = np.random.default_rng(9499)                      # apart from rng: the same sets in every order
    for q in range(nq):
        rows = np.sort(rng.choice(n, min(lengths[q % len(lengths)], n), replace=False)).astype(np.int64)
        rows = rows[::-1] if order == "reversed" else shuffle.permutation(rows) if order == "shuffled" else rows
        parts.append(np.insert(rows, rng.integers(0, rows.size + 1, int(rng.integers(0, 3))), -1))
    lims = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return lims, np.concatenate(parts).astype(np.int64)


def with_guard(rng, ids, n):
    """ids followed by GUARD valid-looking ids that no call may read"""
    return np.concatenate([ids, rng.integers(0, n, GUARD)]).astype(np.int64)


def poisoned(rng, codes, K, named, *per_row):
    """copies in which every row that is not named carries a code >= K (K < 256) resp. NaN / list id -5"""
    off = np.ones(codes.shape[0], bool)
    off[named] = False
    out = [codes.copy()]
    if K < 256:
        out[0][off] = rng.integers(K, 256, (int(off.sum()), codes.shape[1])).astype(np.uint8)
    for a in per_row:
        b = a.copy()
        b[off] = -5 if a.dtype == np.int64 else np.nan
        out.append(b)
    return out


def masked_per_query(pq, ip, cd, t, ids, lims, k, n, extra=None):
    """the existing masked exhaustive entry point, one call per query with the mask of C_q"""
    vs, is_ = [], []
    for q in range(t.shape[0]):
        allow = np.zeros(n, bool)
        allow[candidates(ids, lims, q, n)[0]] = True
        v, i = call_raw(pq, fn_name(ip), cd, t[q].contiguous(), dev_words(pack_ref(allow)), k, extra=extra, has_extra=ip)
        vs.append(v[0])
        is_.append(i[0])
    return np.stack(vs), np.stack(is_)


# ---- plain forms: every NV bucket edge, K, n, nq, L, order of the ids ---------------------------------------------------
SHAPES = [(1, 256, 5000, 13), (3, 2, 65, 3), (15, 16, 5000, 3), (16, 256, 1, 1), (17, 256, 5000, 13), (32, 16, 5000, 1),
          (33, 256, 65, 13), (52, 2, 5000, 3), (53, 256, 5000, 1), (100, 256, 5000, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,n,nq", SHAPES)
def test_gpu_among_matches_reference_and_masked_search(ra, M, K, n, nq):
    """distance, inner product and scaled inner product; sorted, reversed and shuffled ids give one answer, which is the
    reference's and the masked search's per query; rows that are not named are poisoned; the flag stays down"""
    import torch
    rng = np.random.default_rng(9400 + M)
    pq = ra.Pq(None, synth.normalish(9401 + M, (M, K, 1)))
    codes = synth.codes_u8(9402 + M, (n, M), K)
    sc = (rng.random(n) * 3 - 0.5).astype(np.float32)
    ra.launch_log(reset=True)
    for special in (False, True):
        t = integer_tables(rng, nq, M, K, special)
        td = to_dev(t)
        with np.errstate(invalid="ignore"):
            s = orc.adc_scan(t, codes)
        cd = to_dev(codes)
        first = {}
        for order in ("sorted", "reversed", "shuffled"):
            # the same sets in every order; with fewer than nine queries the shapes share the lengths out among them
            lims, ids = draw_csr(np.random.default_rng(9403 + M), nq, n, order, start=M % 9)
            named = ids[ids >= 0]
            pc, psc = poisoned(rng, codes, K, named, sc)
            pcd, pscd, scd = to_dev(pc), to_dev(psc), to_dev(sc)
            idd, ld = to_dev(with_guard(rng, ids, n)), to_dev(lims)
            for ip, extra in ((False, None), (True, None), (True, sc)):
                for k in KS if order == "shuffled" and not special else (1, 129, 1024):
                    print("M %d K %d n %d nq %d special %s order %s ip %s scaled %s k %d" % (M, K, n, nq, special, order, ip, extra is not None, k))
                    want_v, want_i, flagged = ref_among(s, ids, k, lims=lims, ip=ip, extra=extra)
                    assert not flagged
                    got = among_raw(pq, ip, pcd, td, idd, k, lims=ld, n_ids=ids.size, extra=None if extra is None else pscd)
                    flag(pq, False)
                    assert_same(got, want_v, want_i)
                    key = (ip, extra is not None, k)
                    if key in first:
                        assert first[key][0].tobytes() == got[0].tobytes() and np.array_equal(first[key][1], got[1])
                    else:
                        first[key] = got
                        mv, mi = masked_per_query(pq, ip, cd, td, ids, lims, k, n, extra=None if extra is None else scd)
                        assert got[0].tobytes() == mv.tobytes() and np.array_equal(got[1], mi)
    log = ra.launch_log(reset=True)
    assert "k_adc_among_u8" in log and "k_adc_ip_among_u8" in log and "k_adc_search_merge" in log, log
    assert "residual" not in log and "k_adc_lists_plan" not in log, log


# ---- the grid, the shared list, the memory layout -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(ra):
    M, K, n, nq = 15, 256, 5000, 13
    rng = np.random.default_rng(9410)
    pq = ra.Pq(None, synth.normalish(9411, (M, K, 1)))
    codes = synth.codes_u8(9412, (n, M), K)
    t = integer_tables(rng, nq, M, K, True)
    with np.errstate(invalid="ignore"):
        s = orc.adc_scan(t, codes)
    sc = (rng.random(n) * 3 - 0.5).astype(np.float32)
    return dict(pq=pq, M=M, K=K, n=n, nq=nq, codes=codes, t=t, s=s, sc=sc, rng=rng)


@pytest.mark.gpu
def test_gpu_among_does_not_depend_on_the_grid(ra, base):
    """forced workgroups per query 1, 2, 7, 16 and the automatic choice: one answer, the reference's"""
    B = base
    pq, n, nq = B["pq"], B["n"], B["nq"]
    lims, ids = draw_csr(np.random.default_rng(9413), nq, n, "shuffled")
    idd, ld, cd, td, scd = to_dev(with_guard(B["rng"], ids, n)), to_dev(lims), to_dev(B["codes"]), to_dev(B["t"]), to_dev(B["sc"])
    try:
        for ip in (False, True):
            for k in (1, 65, 1024):
                want_v, want_i, _ = ref_among(B["s"], ids, k, lims=lims, ip=ip, extra=B["sc"] if ip else None)
                for G in (1, 2, 7, 16, 0):
                    ra.set_option(OPTION, G)
                    got = among_raw(pq, ip, cd, td, idd, k, lims=ld, n_ids=ids.size, extra=scd if ip else None)
                    flag(pq, False)
                    assert_same(got, want_v, want_i)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
def test_gpu_shared_list_is_the_csr_that_repeats_it(ra, base):
    B = base
    pq, n, nq = B["pq"], B["n"], B["nq"]
    cd, td, scd = to_dev(B["codes"]), to_dev(B["t"]), to_dev(B["sc"])
    for length in (0, 1, 65, 1025, 4097):
        rng = np.random.default_rng(9414 + length)
        shared = rng.permutation(n)[:length].astype(np.int64)
        rep = np.tile(shared, nq)
        rep_lims = np.arange(nq + 1, dtype=np.int64) * length
        for ip in (False, True):
            for k in (1, 129):
                a = among_raw(pq, ip, cd, td, to_dev(with_guard(rng, shared, n)), k, n_ids=length, extra=scd if ip else None)
                flag(pq, False)
                b = among_raw(pq, ip, cd, td, to_dev(with_guard(rng, rep, n)), k, lims=to_dev(rep_lims), n_ids=rep.size,
                              extra=scd if ip else None)
                flag(pq, False)
                assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
                assert_same(a, *ref_among(B["s"], shared, k, ip=ip, extra=B["sc"] if ip else None)[:2])
    # one query with 2-D tables through the wrapper
    import torch
    shared = np.random.default_rng(9415).permutation(n)[:300].astype(np.int64)
    d, i = pq.adc_among_device(cd, td[2].contiguous(), to_dev(shared), 10, check=True)
    assert tuple(d.shape) == (10,)
    assert_same((d[None].cpu().numpy(), i[None].cpu().numpy()), *ref_among(B["s"][2], shared, 10)[:2])
    lims, ids = draw_csr(np.random.default_rng(9416), nq, n, "shuffled")
    sv, si = pq.adc_ip_among_device(cd, td, to_dev(ids), 65, lims=to_dev(lims), scales=scd, check=True)
    assert_same((sv.cpu().numpy(), si.cpu().numpy()), *ref_among(B["s"], ids, 65, lims=lims, ip=True, extra=B["sc"])[:2])


@pytest.mark.gpu
def test_gpu_odd_code_addresses_and_padded_row_strides(ra, base):
    """the code matrix at base addresses 1, 2, 3 mod 4 with row strides M, M + 1, M + 6: one answer"""
    import torch
    B = base
    pq, n, nq, M = B["pq"], B["n"], B["nq"], B["M"]
    lims, ids = draw_csr(np.random.default_rng(9417), nq, n, "shuffled")
    # the first and the last row named, where the fetch falls back to byte loads
    ids[lims[3]] = 0
    ids[lims[3] + 1] = n - 1
    idd, ld, td = to_dev(ids), to_dev(lims), to_dev(B["t"])
    want_v, want_i, _ = ref_among(B["s"], ids, 65, lims=lims)
    for shift in (0, 1, 2, 3):
        for stride in (M, M + 1, M + 6):
            buf = torch.full((n * stride + 8,), 255, dtype=torch.uint8, device="cuda")
            view = buf[shift: shift + n * stride].view(n, stride)[:, :M]
            view.copy_(to_dev(B["codes"]))
            assert view.data_ptr() % 4 == (buf.data_ptr() + shift) % 4
            got = among_raw(pq, False, view, td, idd, 65, lims=ld)
            flag(pq, False)
            assert_same(got, want_v, want_i)


# ---- residual forms -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_lists", [1, 2, 37, 300])
def test_gpu_residual_among_matches_reference_and_masked_lists_search(ra, base, n_lists):
    """the residual forms against the reference and against the masked residual list search probing every list once with
    bias[q][p] = list_bias[q][probe p]; rows that are not named carry a code >= K, a NaN term / scale and list id -5"""
    import torch
    B = base
    pq, n, nq, K = B["pq"], B["n"], B["nq"], 200
    rng = np.random.default_rng(9420 + n_lists)
    pq = ra.Pq(None, synth.normalish(9421, (B["M"], K, 1)))
    codes = synth.codes_u8(9422, (n, B["M"]), K)
    t = integer_tables(rng, nq, B["M"], K, True)
    with np.errstate(invalid="ignore"):
        s = orc.adc_scan(t, codes)
    td = to_dev(t)
    sizes = rng.multinomial(n, np.ones(n_lists) / n_lists)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    row_list = np.repeat(np.arange(n_lists), sizes).astype(np.int64)
    terms = rng.integers(-3, 4, n).astype(np.float32)
    bias = rng.integers(-5, 6, (nq, n_lists + 2)).astype(np.float32)[:, :n_lists]           # a padded bias stride
    probes = np.stack([rng.permutation(n_lists) for _ in range(nq)]).astype(np.int64)
    pbias = np.take_along_axis(bias, probes, 1)
    lims, ids = draw_csr(np.random.default_rng(9423), nq, n, "shuffled")
    named = ids[ids >= 0]
    idd, ld = to_dev(with_guard(rng, ids, n)), to_dev(lims)
    bd = to_dev(np.ascontiguousarray(rng.integers(-5, 6, (nq, n_lists + 2)).astype(np.float32)))
    bd[:, :n_lists] = to_dev(bias)
    bd = bd[:, :n_lists]
    ra.launch_log(reset=True)
    for ip, extra in ((False, terms), (True, None), (True, B["sc"])):
        if extra is None:
            pc, pl = poisoned(rng, codes, K, named, row_list)
            pe = None
        else:
            pc, pl, pe = poisoned(rng, codes, K, named, row_list, extra)
        for k in (1, 65, 257, 1024):
            want_v, want_i, flagged = ref_among(s, ids, k, lims=lims, ip=ip, extra=extra, row_list=row_list, bias=bias)
            assert not flagged
            got = among_raw(pq, ip, to_dev(pc), td, idd, k, lims=ld, n_ids=ids.size, row_list=to_dev(pl), bias=bd,
                            extra=None if pe is None else to_dev(pe))
            flag(pq, False)
            assert_same(got, want_v, want_i)
            if k == 257:                                   # the existing entry point, per query
                for q in (0, 4, 8, nq - 1):
                    allow = np.zeros(n, bool)
                    allow[candidates(ids, lims, q, n)[0]] = True
                    m = call_raw(pq, fn_name(ip, True, True), to_dev(codes), td[q].contiguous(), dev_words(pack_ref(allow)), k,
                                 lists=(to_dev(off), to_dev(probes[q:q + 1])), bias=to_dev(pbias[q:q + 1]),
                                 extra=None if extra is None else to_dev(extra), has_extra=True)
                    assert m[0].tobytes() == got[0][q:q + 1].tobytes() and np.array_equal(m[1], got[1][q:q + 1])
    log = ra.launch_log(reset=True)
    assert "k_adc_among_residual_u8" in log and "k_adc_ip_among_residual_u8" in log, log
    # a bad list id on a named row: the row is skipped and the flag is raised
    bad = row_list.copy()
    victim = int(ids[lims[5]:lims[6]][ids[lims[5]:lims[6]] >= 0][7])
    for value in (-1, n_lists, -5):
        bad[victim] = value
        want_v, want_i, flagged = ref_among(s, ids, 65, lims=lims, extra=terms, row_list=bad, bias=bias)
        assert flagged and victim not in want_i
        got = among_raw(pq, False, to_dev(codes), td, idd, 65, lims=ld, n_ids=ids.size, row_list=to_dev(bad), bias=bd,
                        extra=to_dev(terms))
        flag(pq, True)
        assert_same(got, want_v, want_i)
    # through the wrapper
    d, i = pq.adc_among_device(to_dev(codes), td, to_dev(ids), 10, lims=ld, row_list=to_dev(row_list), list_bias=bd,
                               row_terms=to_dev(terms), check=True)
    assert_same((d.cpu().numpy(), i.cpu().numpy()), *ref_among(s, ids, 10, lims=lims, extra=terms, row_list=row_list, bias=bias)[:2])
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.adc_among_device(to_dev(codes), td, to_dev(ids), 10, lims=ld, row_list=to_dev(bad), list_bias=bd,
                            row_terms=to_dev(terms), check=True)


# ---- bad input ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_bad_ids_codes_and_lims_raise_the_flag_and_read_nothing_else(ra, base):
    import torch
    B = base
    n, nq, K = B["n"], B["nq"], 200
    rng = np.random.default_rng(9430)
    pq = ra.Pq(None, synth.normalish(9431, (B["M"], K, 1)))
    codes = synth.codes_u8(9432, (n, B["M"]), K)
    t = integer_tables(rng, nq, B["M"], K, False)
    s = orc.adc_scan(t, codes)
    td, cd = to_dev(t), to_dev(codes)
    lims, ids = draw_csr(np.random.default_rng(9433), nq, n, "shuffled")
    ld = to_dev(lims)
    k = 65
    # a named row with a code >= K reads entry 0 and raises the flag
    victim = int(ids[lims[7]:lims[8]][ids[lims[7]:lims[8]] >= 0][3])
    bad = codes.copy()
    bad[victim, 4] = K + 5
    zero = bad.copy()
    zero[victim, 4] = 0
    want = ref_among(orc.adc_scan(t, zero), ids, k, lims=lims)
    got = among_raw(pq, False, to_dev(bad), td, to_dev(ids), k, lims=ld)
    flag(pq, True)
    assert_same(got, *want[:2])
    # ids -1 (padding: no flag), n and -7 (skipped, flagged)
    for value, raises in ((-1, False), (n, True), (-7, True), (1 << 40, True)):
        odd = ids.copy()
        odd[lims[6] + 100] = value
        want_v, want_i, flagged = ref_among(s, odd, k, lims=lims)
        assert flagged == raises
        got = among_raw(pq, False, cd, td, to_dev(with_guard(rng, odd, n)), k, lims=ld, n_ids=odd.size)
        flag(pq, raises)
        assert_same(got, want_v, want_i)
    # lims inverted, beyond n_ids, negative: clamped, flagged; the guard behind d_ids is not read.  Only ids below
    # n / 2 are named and the guard holds ids from n / 2 on, so a read past n_ids would show in the result.
    half = n // 2
    low = np.concatenate([np.random.default_rng(9434 + q).permutation(half)[:200] for q in range(nq)]).astype(np.int64)
    low_lims = np.arange(nq + 1, dtype=np.int64) * 200
    guard = (half + rng.integers(0, n - half, 4096)).astype(np.int64)
    idd = to_dev(np.concatenate([low, guard]))
    total = low.size
    for changes in ({4: 550},                                   # query 3 inverted (empty), query 4 starts earlier
                    {nq: total + 500},                          # the last end beyond n_ids
                    {nq - 1: total + 5, nq: total + 900},       # both ends of the last query beyond n_ids
                    {0: -40},                                   # a negative begin
                    {5: 1 << 50},                               # a huge end for query 4, a huge begin for query 5
                    {nq: 1 << 62}, {0: -(1 << 62)}):
        bl = low_lims.copy()
        for at, value in changes.items():
            bl[at] = value
        want_v, want_i, flagged = ref_among(s, low, k, lims=bl)
        assert flagged
        got = among_raw(pq, False, cd, td, idd, k, lims=to_dev(bl), n_ids=low.size)
        flag(pq, True)
        assert_same(got, want_v, want_i)
        assert (got[1] < half).all()
    # an in-order CSR over the same data stays clean
    got = among_raw(pq, False, cd, td, idd, k, lims=to_dev(low_lims), n_ids=low.size)
    flag(pq, False)
    assert_same(got, *ref_among(s, low, k, lims=low_lims)[:2])
    # duplicates: checked against the reference only
    dup = np.array([9, 4, 9, 4, 4, 100, -1, 9], np.int64)
    got = among_raw(pq, False, cd, td[:1].contiguous(), to_dev(dup), 10)
    flag(pq, False)
    want_v, want_i, _ = ref_among(s[:1], dup, 10)
    assert sorted(want_i[0][want_i[0] >= 0].tolist()) == [4, 4, 4, 9, 9, 9, 100]
    assert_same(got, want_v, want_i)


@pytest.mark.gpu
def test_gpu_among_status_codes_and_precedence(ra, base):
    import torch
    from reductive_amd import _lib
    B = base
    pq, n, nq = B["pq"], B["n"], B["nq"]
    cd, td = to_dev(B["codes"]), to_dev(B["t"])
    ids = to_dev(np.arange(50, dtype=np.int64))
    rl = to_dev(np.zeros(n, np.int64))
    bias = to_dev(np.zeros((nq, 4), np.float32))
    terms = to_dev(np.zeros(n, np.float32))
    L = _lib.lib()
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_v = torch.zeros((nq, 16), dtype=torch.float32, device="cuda")
    out_i = torch.zeros((nq, 16), dtype=torch.int64, device="cuda")

    def call(ip=False, slot=0, tables=td, nq_=nq, codes=cd, code_bytes=1, n_=n, c_rs=15, lims=None, ids_=ids, n_ids=50, row_list=None,
             n_lists=0, list_bias=None, b_rs=0, extra=None, k=10, v=out_v, v_rs=16, i=out_i, i_rs=16, pq_=pq):
        p = lambda x: None if x is None else x.data_ptr()
        f = L.pqhip_adc_ip_among_f32_dev if ip else L.pqhip_adc_among_f32_dev
        return f(pq_._cb(), slot, p(tables), nq_, p(codes), code_bytes, n_, c_rs, p(lims), p(ids_), n_ids, p(row_list), n_lists,
                 p(list_bias), b_rs, p(extra), k, p(v), v_rs, p(i), i_rs, z)
    for ip in (False, True):
        assert call(ip) == _lib.OK
        for kw in (dict(k=0), dict(nq_=-1), dict(n_=-1), dict(n_ids=-1), dict(n_lists=-1)):
            assert call(ip, **kw) == _lib.EINVAL, kw
            assert call(ip, slot=9, code_bytes=4, **kw) == _lib.EINVAL                # EINVAL before ENODEV and EUNSUPPORTED
        assert call(ip, slot=9) == _lib.ENODEV and call(ip, slot=-1) == _lib.ENODEV
        assert call(ip, slot=9, code_bytes=4) == _lib.ENODEV                          # ENODEV before EUNSUPPORTED
        for kw in (dict(code_bytes=4), dict(code_bytes=2), dict(k=1025), dict(n_=(1 << 32) - 1)):
            assert call(ip, **kw) == _lib.EUNSUPPORTED, kw
            assert call(ip, v=None, c_rs=1, **kw) == _lib.EUNSUPPORTED                # before the null pointers and ESHAPE
        assert call(ip, n_=(1 << 32) - 2, ids_=None, n_ids=0) == _lib.OK              # the largest row count, nothing named
        ra.launch_log(reset=True)
        assert call(ip, nq_=0, v=None, i=None, ids_=None, row_list=rl) == _lib.OK     # nq == 0 launches nothing, checks nothing more
        assert ra.launch_log(reset=True) == ""
        for kw in (dict(v=None), dict(i=None), dict(ids_=None), dict(tables=None), dict(codes=None), dict(row_list=rl, extra=terms),
                   dict(list_bias=bias, b_rs=4, n_lists=4, extra=terms)):
            assert call(ip, **kw) == _lib.EINVAL, kw
            assert call(ip, c_rs=14, **kw) == _lib.EINVAL                             # EINVAL before ESHAPE
        for kw in (dict(c_rs=14), dict(v_rs=9), dict(i_rs=9), dict(row_list=rl, list_bias=bias, n_lists=4, b_rs=3, extra=terms)):
            assert call(ip, **kw) == _lib.ESHAPE, kw
        assert call(ip, row_list=rl, list_bias=bias, n_lists=4, b_rs=4, extra=terms) == _lib.OK
    assert call(False, row_list=rl, list_bias=bias, n_lists=4, b_rs=4) == _lib.EINVAL  # the residual distance needs the row terms
    assert call(True, row_list=rl, list_bias=bias, n_lists=4, b_rs=4) == _lib.OK       # the similarity runs without scales
    # not served: more than 100 subquantizers, a table beyond LDS
    wide = ra.Pq(None, synth.normalish(9440, (101, 4, 1)))
    assert call(pq_=wide, tables=to_dev(np.zeros((nq, 101, 4), np.float32)), codes=to_dev(np.zeros((n, 101), np.uint8)), c_rs=101) == _lib.EUNSUPPORTED
    big = ra.Pq(None, synth.normalish(9441, (48, 1024, 1)))
    assert call(pq_=big, tables=to_dev(np.zeros((nq, 48, 1024), np.float32)), codes=to_dev(np.zeros((n, 48), np.uint8)), c_rs=48) == _lib.EUNSUPPORTED
    # n_ids == 0 and n_codes == 0 write the padding only
    for kw in (dict(n_ids=0, ids_=None), dict(n_=0, codes=None, tables=None)):
        for ip in (False, True):
            got = among_raw(pq, ip, cd[:kw.get("n_", n)] if "n_" in kw else cd, td, ids[:kw.get("n_ids", 50)], 5)
            assert (got[1] == -1).all() and np.isinf(got[0]).all() and (got[0] > 0).all() != ip
            flag(pq, False)
    torch.cuda.synchronize()
