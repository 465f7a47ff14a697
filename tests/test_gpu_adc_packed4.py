"""4-bit packed codes on the GPU (include/pqhip.h: pqhip_pack_codes4_dev, pqhip_unpack_codes4_dev and the six
pqhip_adc_*search*_packed4_f32_dev).  Everything is exact.  The reference of a packed search is, by its definition, the
existing entry point on the unpacked u8 codes in the same process, with the same tables, probes, biases, row terms,
scales and mask: indices are compared with np.array_equal, values by their bit patterns (a NaN is the same NaN), the
stream's range flag must agree, and sentinels surround every output.  The format itself is pinned on the CPU
(test_adc_packed4.py: reductive_amd.pack_codes4 / unpack_codes4 against tests/adc_packed4_ref.py)."""
import ctypes

import numpy as np
import pytest

SENT_V = np.float32(-1234.5)
SENT_I = -777
GUARD = 0xA5
EXHAUSTIVE_MS = (1, 2, 3, 5, 8, 9, 15, 16, 17, 33, 48, 65, 100)   # every bucket of packed dwords {1, 2, 4, 8, 13}, odd and even
# (n, k, nq): every n, k and nq of the issue at least once, k > n included
SHAPES = ((1, 1, 1), (63, 10, 3), (64, 64, 4), (65, 65, 5), (65, 100, 4), (1023, 100, 8), (1024, 1024, 9), (1025, 10, 13),
          (5000, 100, 13), (5000, 1024, 3), (5000, 65, 8), (5000, 1, 9))


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
    """a codebook of the shape alone: the searches read the caller's tables, the converters M and K"""
    if (M, K) not in _PQS:
        _PQS[M, K] = ra.Pq(None, np.random.default_rng(M * 100 + K).standard_normal((M, K, 3)).astype(np.float32))
    return _PQS[M, K]


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def flag(pq):
    """the stream's range flag: reads and clears it"""
    from reductive_amd import _lib
    return _lib.lib().pqhip_check_codes_dev(pq._cb(), 0, stream_ptr())


def draw_tables(rng, nq, M, K, special):
    """integer-valued, so that ties sit at the k-th place; special: NaN, +-Inf and -0 planted"""
    import torch
    t = rng.integers(-3, 4, (nq, M, K)).astype(np.float32)
    if special:
        for s in (np.nan, np.inf, -np.inf, -0.0):
            t[rng.random(t.shape) < 0.03] = s
    return torch.from_numpy(t).cuda()


def dev_packed(ra, codes, K, offset=0, raw=None):
    """the packed rows of `codes` in exactly n PB bytes, `offset` bytes into an allocation; raw: packed bytes as given"""
    import torch
    p = ra.pack_codes4(codes, n_centroids=K) if raw is None else raw
    buf = torch.empty(offset + p.size, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(p.shape[0], p.shape[1])
    view.copy_(torch.from_numpy(p))
    return view


def search(name, pq, tables, codes, allow, k, packed, lists=None, bias=None, extra=None, has_extra=False, stride=None,
           want_rc=0, pad=3):
    """One of the six searches, packed or the existing _masked entry point (d_allow NULL: the unmasked call), with row
    strides k + pad and sentinels around the outputs -> (value, idx) numpy [nq, k], or None for a status != OK."""
    import torch
    from reductive_amd import _lib
    nq = tables.shape[0]
    n, W = codes.shape
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device="cuda")
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device="cuda")
    args = [pq._cb(), 0, tables.data_ptr(), nq, codes.data_ptr()]
    if not packed:
        args.append(1)
    args += [n, (codes.stride(0) if n > 1 else W) if stride is None else stride, None if allow is None else allow.data_ptr()]
    if lists is not None:
        lo, pr = lists
        args += [lo.data_ptr(), lo.shape[0] - 1, pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else pr.shape[1]]
        if bias is not None:
            args += [bias.data_ptr(), bias.stride(0) if nq > 1 else pr.shape[1]]
    if has_extra:
        args.append(None if extra is None else extra.data_ptr())
    args += [k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, stream_ptr()]
    full = "pqhip_%s_%s_f32_dev" % (name, "packed4" if packed else "masked")
    rc = getattr(_lib.lib(), full)(*args)
    assert rc == want_rc, (full, rc)
    if rc != _lib.OK:
        return None
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    return vb[body].reshape(nq, k), ib[body].reshape(nq, k)


def same_pair(name, pq, tables, packed, unpacked, allow, k, want_flag=0, **kw):
    """the packed call against the existing one on the unpacked codes: indices, bit patterns, the flag"""
    got = search(name, pq, tables, packed, allow, k, True, **kw)
    got_flag = flag(pq)
    want = search(name, pq, tables, unpacked, allow, k, False, **kw)
    ref_flag = flag(pq)
    assert np.array_equal(got[1], want[1]), name
    assert got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes(), name
    assert got_flag == ref_flag == want_flag, (name, got_flag, ref_flag)
    return got


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mask_words(allow):
    b = np.packbits(np.asarray(allow, bool), bitorder="little")
    b = np.concatenate([b, np.zeros((-b.size) % 4, np.uint8)])
    return to_dev(b.view(np.int32))


# ---- pack and unpack -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", (1, 2, 3, 5, 15, 16, 17, 48, 100))
def test_gpu_pack_and_unpack(ra, M):
    import torch
    from reductive_amd import _lib
    L = _lib.lib()
    K = (16, 3, 2)[M % 3]
    pq = make_pq(ra, M, K)
    PB = (M + 1) // 2
    rng = np.random.default_rng(4000 + M)
    for n in (0, 1, 63, 64, 65, 1025):
        codes = rng.integers(0, K, (n, M)).astype(np.uint8)
        want = ra.pack_codes4(codes, n_centroids=K)
        for code_bytes, offset, extra_stride in ((1, 0, 0), (4, 1, 3), (1, 3, 3), (4, 0, 0), (1, 1, 0)):
            src = to_dev(codes if code_bytes == 1 else codes.astype(np.int32))
            stride = PB + extra_stride
            size = offset + max(n, 1) * stride + 5
            buf = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
            rc = L.pqhip_pack_codes4_dev(pq._cb(), 0, src.data_ptr() if n else None, code_bytes, n, M,
                                         buf.data_ptr() + offset if n else None, stride, stream_ptr())
            assert rc == _lib.OK and flag(pq) == _lib.OK
            expect = np.full(size, GUARD, np.uint8)
            for j in range(PB):
                expect[offset + j: offset + j + n * stride: stride][:n] = want[:, j]
            assert np.array_equal(buf.cpu().numpy(), expect), (n, code_bytes, offset, stride)
            # unpack the rows just written, into a guarded buffer of its own with the same offset and a padded stride
            o_stride = M + extra_stride
            osize = offset + max(n, 1) * o_stride + 5
            obuf = torch.full((osize,), GUARD, dtype=torch.uint8, device="cuda")
            rc = L.pqhip_unpack_codes4_dev(pq._cb(), 0, buf.data_ptr() + offset if n else None, n, stride, None, 0,
                                           obuf.data_ptr() + offset if n else None, o_stride, stream_ptr())
            assert rc == _lib.OK and flag(pq) == _lib.OK
            expect = np.full(osize, GUARD, np.uint8)
            for m in range(M):
                expect[offset + m: offset + m + n * o_stride: o_stride][:n] = codes[:, m]
            assert np.array_equal(obuf.cpu().numpy(), expect), (n, offset, o_stride)
        # the wrappers round-trip
        packed = pq.pack_codes4_device(to_dev(codes), check=True)
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (n, PB)
        assert np.array_equal(packed.cpu().numpy(), want)
        assert np.array_equal(pq.unpack_codes4_device(packed, check=True).cpu().numpy(), codes)


@pytest.mark.gpu
def test_gpu_pack_out_of_range_code_packs_zero_and_raises_the_flag(ra):
    from reductive_amd import _lib
    M, K = 5, 3
    pq = make_pq(ra, M, K)
    codes = np.random.default_rng(1).integers(0, K, (70, M)).astype(np.uint8)
    bad = codes.copy()
    bad[0, 4], bad[33, 1], bad[69, 0] = 3, 200, 15
    clean = bad.copy()
    clean[bad >= K] = 0
    for src in (bad, bad.astype(np.int32)):
        got = pq.pack_codes4_device(to_dev(src))
        assert flag(pq) == _lib.ECODE_RANGE
        assert np.array_equal(got.cpu().numpy(), ra.pack_codes4(clean, n_centroids=K))
    wide = bad.astype(np.int32)
    wide[5, 2] = 1 << 20                                    # the low nibble alone would look like a valid code
    clean[5, 2] = 0
    assert np.array_equal(pq.pack_codes4_device(to_dev(wide)).cpu().numpy(), ra.pack_codes4(clean, n_centroids=K))
    assert flag(pq) == _lib.ECODE_RANGE
    with pytest.raises(ra.PanicError):
        pq.pack_codes4_device(to_dev(bad), check=True)
    assert flag(pq) == _lib.OK


@pytest.mark.gpu
@pytest.mark.parametrize("M", (1, 5, 16, 17))
def test_gpu_unpack_selected_rows(ra, M):
    import torch
    from reductive_amd import _lib
    K = 16
    pq = make_pq(ra, M, K)
    rng = np.random.default_rng(4100 + M)
    n = 1025
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    raw = ra.pack_codes4(codes, n_centroids=K)
    if M % 2:
        raw[:, -1] |= 0xf0                                  # the pad nibble is not emitted whatever it holds
    packed = dev_packed(ra, codes, K, offset=1, raw=raw)
    rows = np.concatenate([rng.integers(0, n, 200), [7, 7, 7, 0, n - 1]]).astype(np.int64)
    got = pq.unpack_codes4_device(packed, rows=to_dev(rows), check=True)
    assert np.array_equal(got.cpu().numpy(), codes[rows])
    empty = pq.unpack_codes4_device(packed, rows=torch.zeros(0, dtype=torch.int64, device="cuda"), check=True)
    assert tuple(empty.shape) == (0, M)
    bad = rows.copy()
    bad[3], bad[100] = n, -1
    got = pq.unpack_codes4_device(packed, rows=to_dev(bad))
    assert flag(pq) == _lib.ECODE_RANGE
    want = codes[np.clip(bad, 0, n - 1)]
    want[[3, 100]] = 0
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ra.PanicError):
        pq.unpack_codes4_device(packed, rows=to_dev(bad), check=True)


# ---- exhaustive searches -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", EXHAUSTIVE_MS)
def test_gpu_exhaustive_packed_equals_unpacked(ra, M):
    rng = np.random.default_rng(5000 + M)
    try:
        for K in (16, 3, 2):
            pq = make_pq(ra, M, K)
            for si, (n, k, nq) in enumerate(SHAPES):
                codes = rng.integers(0, K, (n, M)).astype(np.uint8)
                unpacked = to_dev(codes)
                packed = dev_packed(ra, codes, K, offset=(0, 1, 3)[si % 3])     # exactly n PB bytes, also at odd addresses
                tables = draw_tables(rng, nq, M, K, special=si % 2 == 1)
                scales = to_dev(rng.standard_normal(n).astype(np.float32))
                for single in ((0, 1) if K == 16 else (0,)):
                    ra.set_option("adc_single_query", single)
                    same_pair("adc_search", pq, tables, packed, unpacked, None, k)
                    same_pair("adc_ip_search", pq, tables, packed, unpacked, None, k, has_extra=True)
                    same_pair("adc_ip_search", pq, tables, packed, unpacked, None, k, extra=scales, has_extra=True)
    finally:
        ra.set_option("adc_single_query", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(5, 16), (17, 3), (33, 16), (1, 2)])
def test_gpu_pad_nibble_is_ignored(ra, M, K):
    """0xF in the pad nibble of every row of an odd-M matrix changes nothing and raises no flag"""
    rng = np.random.default_rng(5100 + M)
    pq = make_pq(ra, M, K)
    n, k, nq = 1025, 10, 5
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    raw = ra.pack_codes4(codes, n_centroids=K)
    raw[:, -1] |= 0xf0
    packed = dev_packed(ra, codes, K, raw=raw)
    tables = draw_tables(rng, nq, M, K, special=False)
    scales = to_dev(rng.standard_normal(n).astype(np.float32))
    same_pair("adc_search", pq, tables, packed, to_dev(codes), None, k)
    same_pair("adc_ip_search", pq, tables, packed, to_dev(codes), None, k, extra=scales, has_extra=True)
    off = to_dev(np.array([0, 400, 400, n], np.int64))
    probes = to_dev(np.tile(np.array([[2, 0]], np.int64), (nq, 1)))
    same_pair("adc_search_lists", pq, tables, packed, to_dev(codes), None, k, lists=(off, probes))


@pytest.mark.gpu
def test_gpu_nibble_out_of_range_raises_the_flag_and_scores_entry_0(ra):
    from reductive_amd import _lib
    M, K = 9, 3
    rng = np.random.default_rng(5200)
    pq = make_pq(ra, M, K)
    n, k, nq = 1025, 64, 4
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.01] = 3
    codes[7, 8], codes[1024, 0] = 15, 9
    raw = ra.pack_codes4(codes, n_centroids=16)            # the nibbles as they are
    packed = dev_packed(ra, codes, K, raw=raw)
    tables = draw_tables(rng, nq, M, K, special=False)
    got = same_pair("adc_search", pq, tables, packed, to_dev(codes), None, k, want_flag=_lib.ECODE_RANGE)
    zeroed = codes.copy()
    zeroed[codes >= K] = 0
    clean = search("adc_search", pq, tables, to_dev(zeroed), None, k, False)
    assert flag(pq) == _lib.OK
    assert np.array_equal(got[1], clean[1]) and got[0].tobytes() == clean[0].tobytes()


@pytest.mark.gpu
def test_gpu_exhaustive_grid_independence(ra):
    import torch
    rng = np.random.default_rng(5300)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for M, K in ((16, 16), (5, 3)):
            pq = make_pq(ra, M, K)
            n, nq = 5000, 9
            codes = rng.integers(0, K, (n, M)).astype(np.uint8)
            packed, unpacked = dev_packed(ra, codes, K, offset=1), to_dev(codes)
            tables = draw_tables(rng, nq, M, K, special=True)
            scales = to_dev(rng.standard_normal(n).astype(np.float32))
            allow = mask_words(rng.random(n) < 0.5)
            for wgs in (1, 2, 7, cus, 0):
                ra.set_option("adc_packed4_wgs", wgs)
                for k in (10, 100):
                    same_pair("adc_search", pq, tables, packed, unpacked, None, k)
                    same_pair("adc_ip_search", pq, tables, packed, unpacked, allow, k, extra=scales, has_extra=True)
    finally:
        ra.set_option("adc_packed4_wgs", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(5, 3), (16, 16), (17, 16), (48, 2)])
def test_gpu_exhaustive_with_a_mask(ra, M, K):
    from reductive_amd import _lib
    rng = np.random.default_rng(5400 + M)
    pq = make_pq(ra, M, K)
    for n, k, nq in ((1025, 10, 5), (5000, 100, 8), (65, 65, 1)):
        codes = rng.integers(0, K, (n, M)).astype(np.uint8)
        tables = draw_tables(rng, nq, M, K, special=True)
        scales = rng.standard_normal(n).astype(np.float32)
        one = np.zeros(n, bool)
        one[n // 2] = True
        for allow in (np.ones(n, bool), rng.random(n) < 0.5, one, np.zeros(n, bool)):
            # a disallowed row holds nibbles >= K and a NaN scale: it is not read
            dirty, sc = codes.copy(), scales.copy()
            if K < 16:
                dirty[~allow] = 15
            sc[~allow] = np.nan
            packed = dev_packed(ra, dirty, K, raw=ra.pack_codes4(dirty, n_centroids=16))
            words = mask_words(allow)
            got = same_pair("adc_search", pq, tables, packed, to_dev(dirty), words, k)
            assert ((got[1] >= 0).sum(1) == min(k, int(allow.sum()))).all()
            live = got[1][got[1] >= 0]
            assert allow[live].all()
            got = same_pair("adc_ip_search", pq, tables, packed, to_dev(dirty), words, k, extra=to_dev(sc), has_extra=True)
            assert allow[got[1][got[1] >= 0]].all()
    assert flag(pq) == _lib.OK


# ---- list searches -------------------------------------------------------------------------------------------------
def draw_lists(rng, n, n_lists):
    """offsets with empty lists, one heavy list and lists shorter than a wave"""
    if n_lists == 1:
        return np.array([0, n], np.int64)
    heavy = n // 2
    cuts = np.sort(rng.integers(heavy, n + 1, n_lists - 2))
    off = np.concatenate([[0, heavy], cuts, [n]]).astype(np.int64)
    for l in range(2, n_lists - 1, 4):
        off[l + 1] = off[l]                                # an empty list
    return np.maximum.accumulate(off)


def draw_probes(rng, nq, n_lists, n_probe):
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    if n_probe > 1:
        pr[rng.random(pr.shape) < 0.15] = -1
    pr[:, 0] = np.where(pr[:, 0] < 0, 0, pr[:, 0])
    pr[0, 0] = 0                                            # the heavy list
    return pr


def all_list_searches(pq, tables, packed, unpacked, allow, k, lists, bias, terms, scales, want_flag=0):
    same_pair("adc_search_lists", pq, tables, packed, unpacked, allow, k, lists=lists, want_flag=want_flag)
    same_pair("adc_ip_search_lists", pq, tables, packed, unpacked, allow, k, lists=lists, has_extra=True, want_flag=want_flag)
    same_pair("adc_ip_search_lists", pq, tables, packed, unpacked, allow, k, lists=lists, extra=scales, has_extra=True,
              want_flag=want_flag)
    same_pair("adc_search_lists_residual", pq, tables, packed, unpacked, allow, k, lists=lists, bias=bias, extra=terms,
              has_extra=True, want_flag=want_flag)
    same_pair("adc_ip_search_lists_residual", pq, tables, packed, unpacked, allow, k, lists=lists, bias=bias, has_extra=True,
              want_flag=want_flag)
    same_pair("adc_ip_search_lists_residual", pq, tables, packed, unpacked, allow, k, lists=lists, bias=bias, extra=scales,
              has_extra=True, want_flag=want_flag)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(5, 3), (16, 16), (17, 2), (48, 16), (65, 16), (100, 3)])
def test_gpu_list_searches_packed_equal_unpacked(ra, M, K):
    from reductive_amd import _lib
    rng = np.random.default_rng(6000 + M)
    pq = make_pq(ra, M, K)
    for n, n_lists, nq, k in ((5000, 300, 5, 10), (3000, 7, 3, 100), (700, 1, 2, 1024), (40, 7, 4, 65)):
        codes = rng.integers(0, K, (n, M)).astype(np.uint8)
        packed, unpacked = dev_packed(ra, codes, K, offset=1), to_dev(codes)
        tables = draw_tables(rng, nq, M, K, special=True)
        off = to_dev(draw_lists(rng, n, n_lists))
        terms = to_dev(rng.standard_normal(n).astype(np.float32))
        scales = to_dev(rng.standard_normal(n).astype(np.float32))
        words = mask_words(rng.random(n) < 0.5)             # in position order: the order of the rows as stored
        for n_probe in sorted({1, min(3, n_lists), n_lists}):
            probes = to_dev(draw_probes(rng, nq, n_lists, n_probe))
            bias = to_dev(rng.standard_normal((nq, n_probe)).astype(np.float32))
            for allow in (None, words):
                all_list_searches(pq, tables, packed, unpacked, allow, k, (off, probes), bias, terms, scales)
        # an out-of-range probe id is skipped and raises the flag, in both
        pr = draw_probes(rng, nq, n_lists, min(3, n_lists))
        pr[-1, -1] = n_lists
        bias = to_dev(rng.standard_normal(pr.shape).astype(np.float32))
        all_list_searches(pq, tables, packed, unpacked, None, k, (off, to_dev(pr)), bias, terms, scales,
                          want_flag=_lib.ECODE_RANGE)


@pytest.mark.gpu
def test_gpu_list_searches_grid_independence(ra):
    rng = np.random.default_rng(6100)
    try:
        for M, K in ((16, 16), (9, 3)):
            pq = make_pq(ra, M, K)
            n, n_lists, nq, k = 5000, 40, 4, 100
            codes = rng.integers(0, K, (n, M)).astype(np.uint8)
            packed, unpacked = dev_packed(ra, codes, K, offset=3), to_dev(codes)
            tables = draw_tables(rng, nq, M, K, special=False)
            off = to_dev(draw_lists(rng, n, n_lists))
            probes = to_dev(draw_probes(rng, nq, n_lists, 9))
            bias = to_dev(rng.standard_normal((nq, 9)).astype(np.float32))
            terms = to_dev(rng.standard_normal(n).astype(np.float32))
            scales = to_dev(rng.standard_normal(n).astype(np.float32))
            words = mask_words(rng.random(n) < 0.7)
            for g in (1, 2, 7, 0):
                ra.set_option("adc_lists_wgs_per_query", g)
                all_list_searches(pq, tables, packed, unpacked, words if g == 7 else None, k, (off, probes), bias, terms, scales)
    finally:
        ra.set_option("adc_lists_wgs_per_query", 0)


# ---- status codes that need a handle -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_status_codes_and_their_precedence(ra):
    import torch
    from reductive_amd import _lib
    L = _lib.lib()
    z = stream_ptr()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    f = torch.zeros(4096, dtype=torch.float32, device="cuda")
    i = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, fp, ip_ = buf.data_ptr(), f.data_ptr(), i.data_ptr()
    of, oi = fp + 4 * 2048, ip_ + 8 * 32                                   # outputs, apart from the inputs

    def all_six(cb, slot, stride, k=5, n=10):
        head = (cb, slot, fp, 1, p, n, stride, None)
        lists = (ip_, 2, ip_, 1, 1)
        return [L.pqhip_adc_search_packed4_f32_dev(*head, k, of, k, oi, k, z),
                L.pqhip_adc_ip_search_packed4_f32_dev(*head, None, k, of, k, oi, k, z),
                L.pqhip_adc_search_lists_packed4_f32_dev(*head, *lists, k, of, k, oi, k, z),
                L.pqhip_adc_ip_search_lists_packed4_f32_dev(*head, *lists, None, k, of, k, oi, k, z),
                L.pqhip_adc_search_lists_residual_packed4_f32_dev(*head, *lists, fp, 1, fp, k, of, k, oi, k, z),
                L.pqhip_adc_ip_search_lists_residual_packed4_f32_dev(*head, *lists, fp, 1, None, k, of, k, oi, k, z)]

    ok = make_pq(ra, 5, 16)
    k32 = make_pq(ra, 4, 32)
    m101 = make_pq(ra, 101, 4)
    assert all_six(ok._cb(), 0, 3) == [_lib.OK] * 6
    assert flag(ok) == _lib.OK
    assert all_six(k32._cb(), 0, 2) == [_lib.EUNSUPPORTED] * 6
    assert all_six(m101._cb(), 0, 51) == [_lib.EUNSUPPORTED] * 6
    assert all_six(ok._cb(), 0, 2) == [_lib.ESHAPE] * 6                      # 5 codes are 3 bytes
    assert all_six(ok._cb(), 0, 3, k=1025) == [_lib.EUNSUPPORTED] * 6
    # precedence: EINVAL, ENODEV, EUNSUPPORTED, ESHAPE
    assert all_six(k32._cb(), 0, 1) == [_lib.EUNSUPPORTED] * 6               # before the stride
    assert all_six(k32._cb(), 99, 1) == [_lib.ENODEV] * 6                    # before the quantizer
    assert all_six(k32._cb(), 99, 1, k=0) == [_lib.EINVAL] * 6               # before the slot
    assert all_six(None, 99, 1) == [_lib.EINVAL] * 6
    # the converters
    assert L.pqhip_pack_codes4_dev(k32._cb(), 0, p, 1, 4, 4, p, 2, z) == _lib.EUNSUPPORTED
    assert L.pqhip_pack_codes4_dev(ok._cb(), 0, p, 2, 4, 5, p, 3, z) == _lib.EUNSUPPORTED
    assert L.pqhip_pack_codes4_dev(ok._cb(), 0, p, 1, 4, 5, p, 2, z) == _lib.ESHAPE
    assert L.pqhip_pack_codes4_dev(ok._cb(), 0, p, 1, 4, 4, p, 3, z) == _lib.ESHAPE
    assert L.pqhip_pack_codes4_dev(ok._cb(), 7, p, 1, 4, 5, p, 3, z) == _lib.ENODEV
    assert L.pqhip_unpack_codes4_dev(k32._cb(), 0, p, 4, 2, None, 0, p, 4, z) == _lib.EUNSUPPORTED
    assert L.pqhip_unpack_codes4_dev(ok._cb(), 0, p, 4, 2, None, 0, p, 5, z) == _lib.ESHAPE
    assert L.pqhip_unpack_codes4_dev(ok._cb(), 0, p, 4, 3, None, 0, p, 4, z) == _lib.ESHAPE
    with pytest.raises(ra.PanicError):
        k32.adc_search_device(buf[:8].view(4, 2), f[:128].view(4, 32), 3, packed4=True)
    with pytest.raises(ra.PanicError):                                      # the packed width is checked
        ok.adc_search_device(buf[:20].view(4, 5), f[:80].view(5, 16), 3, packed4=True)


@pytest.mark.gpu
def test_gpu_wrappers_and_launch_log(ra):
    """packed4=True reaches the packed kernels; packed4=False is the call it was: same launch log"""
    rng = np.random.default_rng(7000)
    M, K, n, nq, k = 16, 16, 3000, 8, 10
    pq = make_pq(ra, M, K)
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    cd = to_dev(codes)
    pk = pq.pack_codes4_device(cd)
    tables = draw_tables(rng, nq, M, K, special=False)
    ra.launch_log(reset=True)
    d0, i0 = pq.adc_search_device(cd, tables, k)
    log_plain = ra.launch_log(reset=True)
    d1, i1 = pq.adc_search_device(cd, tables, k, packed4=False)
    assert ra.launch_log(reset=True) == log_plain and "p4" not in log_plain
    d2, i2 = pq.adc_search_device(pk, tables, k, packed4=True)
    log_packed = ra.launch_log(reset=True)
    print(log_plain, "|", log_packed)
    assert "k_adc_search_p4_mq<8 queries>" in log_packed and "k_adc_search_u8" not in log_packed
    import torch
    assert torch.equal(i0, i2) and torch.equal(d0.view(torch.int32), d2.view(torch.int32)) and torch.equal(i0, i1)
    s0, j0 = pq.adc_ip_search_device(cd, tables[0], k)
    s2, j2 = pq.adc_ip_search_device(pk, tables[0], k, packed4=True)
    assert "k_adc_ip_search_p4" in ra.launch_log(reset=True)
    assert torch.equal(j0, j2) and torch.equal(s0.view(torch.int32), s2.view(torch.int32))
