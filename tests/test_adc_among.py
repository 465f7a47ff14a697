"""ADC search among given rows, CPU side: the reference (tests/adc_among_ref.py) against the references of the masked
searches on distinct ids -- the sentence of include/pqhip.h the GPU tests rest on --; header, EXPORTS, SIGNATURES, library
and rust/pqhip_ffi.rs name the two entry points and the option, and neither name falls under the grammar of the 24
search and range symbols; the statuses a null codebook reaches; the wrappers' checks, which come before any device call;
the matrix methods on a packed matrix.  (Everything that needs a codebook handle: tests/test_gpu_adc_among.py,
tests/test_gpu_qmatrix_among.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from adc_among_ref import candidates, ref_among
from adc_ip_ref import scores
from adc_masked_ref import ref_masked_residual_search, ref_masked_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_adc_among_f32_dev", "pqhip_adc_ip_among_f32_dev")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def same(got_v, got_i, want_v, want_i):
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(np.isnan(got_v), np.isnan(want_v))
    ok = ~np.isnan(want_v)
    assert np.asarray(got_v, np.float32)[ok].tobytes() == np.asarray(want_v, np.float32)[ok].tobytes()


def draw_values(rng, nq, n):
    """integer-valued sums with many ties, a few NaN, +-Inf and -0"""
    s = rng.integers(-4, 5, (nq, n)).astype(np.float32)
    for special in (np.nan, np.inf, -np.inf, -0.0):
        s[rng.random((nq, n)) < 0.03] = special
    return s


def draw_csr(rng, nq, n, lengths, order):
    """per query a list of distinct row ids (of the given length, cut to n), -1 padding sprinkled in -> (lims, ids)"""
    parts = []
    for q in range(nq):
        rows = rng.choice(n, min(int(lengths[q % len(lengths)]), n), replace=False).astype(np.int64)
        rows = np.sort(rows) if order == "sorted" else np.sort(rows)[::-1] if order == "reversed" else rows
        pads = rng.integers(0, 3)
        rows = np.insert(rows, rng.integers(0, rows.size + 1, pads), -1)
        parts.append(rows)
    lims = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return lims, np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)


@pytest.mark.parametrize("order", ["sorted", "reversed", "shuffled"])
@pytest.mark.parametrize("n", [1, 65, 700])
def test_reference_is_the_masked_search_on_distinct_ids(n, order):
    """plain forms: distance, inner product, scaled inner product; per query the masked reference with the mask of C_q;
    shuffled ids, -1 padding and k > |C_q| among the cases"""
    rng = np.random.default_rng(9300 + n)
    nq = 5
    s = draw_values(rng, nq, n)
    sc = (rng.random(n) * 3 - 0.5).astype(np.float32)
    lims, ids = draw_csr(rng, nq, n, [0, 1, 40, 64, 300], order)
    for ip, extra in ((False, None), (True, None), (True, sc)):
        values = scores(s, extra) if ip else s
        for k in (1, 10, 64, 129):
            v, i, flagged = ref_among(s, ids, k, lims=lims, ip=ip, extra=extra)
            assert not flagged
            for q in range(nq):
                allow = np.zeros(n, bool)
                rows, _ = candidates(ids, lims, q, n)
                allow[rows] = True
                assert int(allow.sum()) == rows.size
                wv, wi = ref_masked_search(values[q], allow, k, ip=ip)
                same(v[q:q + 1], i[q:q + 1], wv, wi)
                assert (i[q] >= 0).sum() == min(k, rows.size)
        # the shared list is the CSR that repeats it
        shared = ids[lims[2]:lims[3]]
        a = ref_among(s, shared, 10, ip=ip, extra=extra)
        rep_lims = np.arange(nq + 1, dtype=np.int64) * shared.size
        b = ref_among(s, np.tile(shared, nq), 10, lims=rep_lims, ip=ip, extra=extra)
        same(a[0], a[1], b[0], b[1])


@pytest.mark.parametrize("n_lists", [1, 7, 300])
def test_residual_reference_is_the_masked_residual_search_probing_every_list(n_lists):
    rng = np.random.default_rng(9310 + n_lists)
    nq, n = 4, 900
    s = draw_values(rng, nq, n)
    terms = rng.integers(-3, 4, n).astype(np.float32)
    sc = (rng.random(n) * 3 - 0.5).astype(np.float32)
    bias = rng.integers(-5, 6, (nq, n_lists)).astype(np.float32)
    sizes = rng.multinomial(n, np.ones(n_lists) / n_lists)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    row_list = np.repeat(np.arange(n_lists), sizes).astype(np.int64)
    probes = np.stack([rng.permutation(n_lists) for _ in range(nq)]).astype(np.int64)
    probe_bias = np.take_along_axis(bias, probes, 1)
    lims, ids = draw_csr(rng, nq, n, [3, 100, 513, 0], "shuffled")
    for ip, extra in ((False, terms), (True, None), (True, sc)):
        for k in (1, 65, 257):
            v, i, flagged = ref_among(s, ids, k, lims=lims, ip=ip, extra=extra, row_list=row_list, bias=bias)
            assert not flagged
            for q in range(nq):
                allow = np.zeros(n, bool)
                allow[candidates(ids, lims, q, n)[0]] = True
                wv, wi = ref_masked_residual_search(s[q], allow, off, probes[q], probe_bias[q], k, terms=None if ip else extra,
                                                    scales=extra if ip else None, ip=ip)
                same(v[q:q + 1], i[q:q + 1], wv, wi)


def test_reference_on_bad_input():
    """-1 is padding; other ids outside [0, n), a bad lims and a bad list id of a named row are skipped and flagged;
    duplicates stay"""
    s = np.arange(10, dtype=np.float32)[None]
    v, i, f = ref_among(s, [3, -1, 7], 4)
    assert i.tolist() == [[3, 7, -1, -1]] and not f and np.isinf(v[0, 2])
    for bad in (10, -7):
        v, i, f = ref_among(s, [3, bad, 7], 4)
        assert i.tolist() == [[3, 7, -1, -1]] and f
    v, i, f = ref_among(s, [5, 5, 2], 4)
    assert i.tolist() == [[2, 5, 5, -1]] and not f
    ids = np.array([1, 2, 3, 4], np.int64)
    for lims, want in (([3, 1], []), ([2, 9], [3, 4]), ([-2, 1], [1]), ([7, 9], [])):
        v, i, f = ref_among(s, ids, 2, lims=np.array(lims, np.int64))
        assert f and i[0][i[0] >= 0].tolist() == want[:2]
    v, i, f = ref_among(s, ids, 2, lims=np.array([1, 1], np.int64))
    assert not f and (i == -1).all()
    row_list = np.zeros(10, np.int64)
    row_list[2] = -5
    v, i, f = ref_among(s, ids, 4, extra=np.zeros(10, np.float32), row_list=row_list, bias=np.zeros((1, 1), np.float32))
    assert f and i.tolist() == [[4, 3, 1, -1]]                      # dist = fl(0 + 0) - fl(s + s): the largest s first
    v, i, f = ref_among(s, [1, 3], 4, extra=np.zeros(10, np.float32), row_list=row_list, bias=np.zeros((1, 1), np.float32))
    assert not f                                                           # the bad list id belongs to a row that is not named


def test_header_exports_signatures_library_and_ffi_name_the_entry_points(ra):
    from reductive_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert re.search(r"pub fn %s\(" % name, ffi)
        assert not re.match("pqhip_adc_(ip_)?(search|range)", name)
        argtypes = getattr(L, name).argtypes
        assert len(argtypes) == 22 and argtypes[-1] is ctypes.c_void_p and argtypes[16] is ctypes.c_int32
    assert len([s for s in _lib.SIGNATURES if re.match("pqhip_adc_(ip_)?(search|range)", s)]) == 24
    assert '"adc_among_wgs_per_query"' in hdr and '"adc_among_wgs_per_query"' in ffi
    ctx_src = open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    assert '{"adc_among_wgs_per_query", &o.adc_among_wgs_per_query}' in ctx_src
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "A row that is not named is not read" in flat
    assert "No byte outside d_ids[0 .. n_ids) is read" in flat
    assert "pqhip_adc_among" in open(os.path.join(ROOT, "reductive_amd", "csrc", "Makefile")).read()


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    for name in NAMES:
        f = getattr(L, name)
        assert f(None, 0, None, 0, None, 1, 0, 0, None, None, 0, None, 0, None, 0, None, 1, None, 0, None, 0, z) == _lib.EINVAL
        assert f(None, 0, p, 1, p, 1, 4, 2, p, p, 2, None, 0, None, 0, None, 1, p, 1, p, 1, z) == _lib.EINVAL
        assert f(None, 7, p, -1, p, 4, 4, 2, None, p, -2, p, -1, p, 0, p, 0, p, 1, p, 1, z) == _lib.EINVAL


def test_wrappers_check_shapes_before_any_device_call(ra):
    """CPU tensors throughout: a mismatch must be refused before a wrapper asks for a device, a handle or a stream"""
    import torch
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))                  # M = 2, K = 4
    codes = torch.zeros((9, 2), dtype=torch.uint8)
    tables = torch.zeros((3, 2, 4))
    ids = torch.zeros(5, dtype=torch.int64)
    lims = torch.zeros(4, dtype=torch.int64)
    f9 = torch.zeros(9)
    l9 = torch.zeros(9, dtype=torch.int64)
    bias = torch.zeros((3, 6))
    for call, extra in ((pq.adc_among_device, "row_terms"), (pq.adc_ip_among_device, "scales")):
        with pytest.raises(ra.PanicError, match="uint8"):
            call(codes.to(torch.int32), tables, ids, 3)
        with pytest.raises(ra.PanicError, match="uint8"):
            call(np.zeros((9, 2), np.uint8), tables, ids, 3)
        with pytest.raises(ra.PanicError, match="Quantization length"):
            call(torch.zeros((9, 3), dtype=torch.uint8), tables, ids, 3)
        with pytest.raises(ra.PanicError, match="lookup tables"):
            call(codes, tables.double(), ids, 3)
        with pytest.raises(ra.PanicError, match=re.escape("lookup tables must be [.., 2, 4]")):
            call(codes, torch.zeros((3, 2, 5)), ids, 3)
        with pytest.raises(ra.PanicError, match="candidate ids"):
            call(codes, tables, ids.to(torch.int32), 3)
        with pytest.raises(ra.PanicError, match="candidate ids"):
            call(codes, tables, torch.zeros((3, 5), dtype=torch.int64), 3)
        with pytest.raises(ra.PanicError, match="candidate ids"):
            call(codes, tables, torch.zeros(10, dtype=torch.int64)[::2], 3)
        with pytest.raises(ra.PanicError, match="lims must"):
            call(codes, tables, ids, 3, lims=lims.to(torch.int32))
        with pytest.raises(ra.PanicError, match=re.escape("one offset per query and the end (4)")):
            call(codes, tables, ids, 3, lims=lims[:3])
        with pytest.raises(ra.PanicError, match="positive integer"):
            call(codes, tables, ids, 0)
        with pytest.raises(ra.PanicError, match="%s must hold one value per code row" % extra):
            call(codes, tables, ids, 3, **{extra: f9[:8]})
        with pytest.raises(ra.PanicError, match="%s must be a contiguous float32 vector" % extra):
            call(codes, tables, ids, 3, **{extra: f9.double()})
        for kw in (dict(row_list=l9), dict(list_bias=bias)):
            with pytest.raises(ra.PanicError, match="needs the list of every row and a bias per list"):
                call(codes, tables, ids, 3, **kw)
        with pytest.raises(ra.PanicError, match="row_list must be"):
            call(codes, tables, ids, 3, row_list=l9.to(torch.int32), list_bias=bias, **{extra: f9})
        with pytest.raises(ra.PanicError, match="one list id per code row"):
            call(codes, tables, ids, 3, row_list=l9[:8], list_bias=bias, **{extra: f9})
        with pytest.raises(ra.PanicError, match="list_bias must be"):
            call(codes, tables, ids, 3, row_list=l9, list_bias=bias.double(), **{extra: f9})
        with pytest.raises(ra.PanicError, match="one row of list biases per query"):
            call(codes, tables, ids, 3, row_list=l9, list_bias=bias[:2], **{extra: f9})
        with pytest.raises(ra.PanicError, match="CUDA tensors"):
            call(codes, tables, ids, 3, lims=lims)
    with pytest.raises(ra.PanicError, match="needs the row terms"):
        pq.adc_among_device(codes, tables, ids, 3, row_list=l9, list_bias=bias)


def test_matrix_methods_refuse_bad_rows_and_packed_codes(ra):
    """without a GPU: the matrix lives on the CPU, and every refusal comes before a device call"""
    from reductive_amd import qmatrix
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))
    qm = qmatrix.QuantizedMatrix(pq, np.zeros((9, 2), np.uint8), device="cpu")
    q = np.zeros((3, 6), np.float32)
    for call in (qm.nearest_among, qm.most_similar_among):
        with pytest.raises(ra.PanicError, match="integers"):
            call(q, np.zeros(4, np.float32), 2)
        with pytest.raises(ra.PanicError, match="vector of integers"):
            call(q, np.zeros((2, 2), np.int64), 2)
        with pytest.raises(ra.PanicError, match=re.escape("the pair (lims, rows)")):
            call(q, (np.zeros(4, np.int64),), 2)
        with pytest.raises(ra.PanicError, match="attach_vectors"):
            call(q, np.zeros(4, np.int64), 2, refine=4)
    packed = qm._with_codes(qm.codes[:, :1], True)                      # what pack4() returns, without the device call
    with pytest.raises(ra.PanicError, match=re.escape("nearest_among() does not read 4-bit packed codes: call unpack4() first")):
        packed.nearest_among(q, np.zeros(4, np.int64), 2)
    with pytest.raises(ra.PanicError, match=re.escape("most_similar_among() does not read 4-bit packed codes: call unpack4() first")):
        packed.most_similar_among(q, (np.zeros(4, np.int64), np.zeros(4, np.int64)), 2)
