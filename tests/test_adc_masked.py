"""Masked ADC searches, CPU side: the reference of tests/adc_masked_ref.py (restrict to the allowed rows, call the
unmasked references, map back) equals the unmasked references under an all-ones mask, a brute-force selection over the
allowed rows under random masks (inputs with many ties, NaN, +-Inf and -0), and the padding under an all-zero mask;
pack_ref by hand at the word boundaries; the C ABI declares and exports the seven entry points; the permutation a
RowFilter of a partitioned matrix packs through, bit p = allow[ids[p]], on ivf_layout outputs."""
import ctypes
import os
import re

import numpy as np
import pytest

from adc_ip_ref import ref_ip_search
from adc_lists_ref import probed_positions, ref_lists_search
from adc_masked_ref import (compressed_offsets, pack_ref, ref_masked_lists_search, ref_masked_residual_search,
                            ref_masked_search, unpack_ref)
from adc_residual_ref import ref_residual_search, residual_values
from test_gpu_adc_search import ref_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_adc_search_masked_f32_dev", "pqhip_adc_ip_search_masked_f32_dev",
         "pqhip_adc_search_lists_masked_f32_dev", "pqhip_adc_ip_search_lists_masked_f32_dev",
         "pqhip_adc_search_lists_residual_masked_f32_dev", "pqhip_adc_ip_search_lists_residual_masked_f32_dev",
         "pqhip_pack_row_mask_dev")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def draw_values(rng, nq, n):
    """small integers (many ties) with NaN, +-Inf and -0 planted, as test_gpu_adc_search.py draws them"""
    v = rng.integers(-3, 4, (nq, n)).astype(np.float32)
    for special in (np.nan, np.inf, -np.inf, -0.0):
        v[rng.random((nq, n)) < 0.1] = special
    return v


def draw_lists(rng, n, n_lists):
    """offsets with empty lists, one-row lists and lists shorter than a mask word"""
    cuts = np.sort(rng.integers(0, n + 1, n_lists - 1))
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    for l in range(0, n_lists - 1, 4):
        off[l + 1] = off[l]
    return np.maximum.accumulate(off)


def draw_probes(rng, nq, n_lists, n_probe):
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    pr[rng.random(pr.shape) < 0.2] = -1
    return pr


def brute(values, positions, k, ip):
    """the first k of `positions` under (NaN flag, value or -score, position); -1 and +Inf / -Inf after them"""
    v = values[positions].astype(np.float64)
    nan = np.isnan(v)
    val = (-1.0 if ip else 1.0) * np.where(nan, 0.0, v) + 0.0
    top = positions[np.lexsort((positions, val, nan))[:k]]
    out_i = np.full(k, -1, np.int64)
    out_v = np.full(k, -np.inf if ip else np.inf, np.float32)
    out_i[:top.size] = top
    out_v[:top.size] = values[top] + np.float32(0.0) if ip else values[top]
    return out_v, out_i


def same(got, want):
    (gv, gi), (wv, wi) = got, want
    assert np.array_equal(gi, wi)
    assert np.array_equal(np.isnan(gv), np.isnan(wv))
    ok = ~np.isnan(gv)
    assert np.asarray(gv, np.float32)[ok].tobytes() == np.asarray(wv, np.float32)[ok].tobytes()


@pytest.mark.parametrize("ip", [False, True])
def test_all_ones_mask_is_the_unmasked_reference(ip):
    rng = np.random.default_rng(9950)
    for n in (1, 33, 300):
        v = draw_values(rng, 3, n)
        ones = np.ones(n, bool)
        for k in (1, 10, 400):
            same(ref_masked_search(v, ones, k, ip=ip), ref_ip_search(v, k) if ip else ref_search(v, k))
        off, pr = draw_lists(rng, n, 9), draw_probes(rng, 3, 9, 4)
        assert np.array_equal(compressed_offsets(off, ones), off)
        bias = rng.standard_normal(pr.shape).astype(np.float32)
        terms = rng.standard_normal(n).astype(np.float32)
        for k in (1, 10, 400):
            same(ref_masked_lists_search(v, ones, off, pr, k, ip=ip), ref_lists_search(v, off, pr, k, ip=ip))
            same(ref_masked_residual_search(v, ones, off, pr, bias, k, terms=None if ip else terms, scales=terms if ip else None, ip=ip),
                 ref_residual_search(v, off, pr, bias, k, terms=None if ip else terms, scales=terms if ip else None, ip=ip))


@pytest.mark.parametrize("ip", [False, True])
def test_random_masks_equal_a_brute_force_selection_over_the_allowed_rows(ip):
    rng = np.random.default_rng(9951)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        nq = 3
        v = draw_values(rng, nq, n)
        allow = rng.random(n) < rng.choice([0.01, 0.5, 0.9])
        rows = np.flatnonzero(allow)
        for k in (1, 7, 64):
            gv, gi = ref_masked_search(v, allow, k, ip=ip)
            for q in range(nq):
                same((gv[q], gi[q]), brute(v[q], rows, k, ip))
            assert np.isin(gi[gi >= 0], rows).all() and ((gi >= 0).sum(1) == min(k, rows.size)).all()
        # list form: S_q n A in (key, position) order
        n_lists = 11
        off, pr = draw_lists(rng, n, n_lists), draw_probes(rng, nq, n_lists, 5)
        for k in (1, 7, 64):
            gv, gi = ref_masked_lists_search(v, allow, off, pr, k, ip=ip)
            for q in range(nq):
                pos = probed_positions(off, pr[q], n)
                same((gv[q], gi[q]), brute(v[q], pos[allow[pos]], k, ip))
        # residual form: the values of the full matrix, then the same selection
        bias = rng.integers(-2, 3, pr.shape).astype(np.float32)
        extra = rng.integers(-2, 3, n).astype(np.float32)
        extra[rng.random(n) < 0.05] = np.nan
        kw = dict(scales=extra) if ip else dict(terms=extra)
        vals = residual_values(v, off, pr, bias, ip=ip, **kw)
        for k in (1, 7, 64):
            gv, gi = ref_masked_residual_search(v, allow, off, pr, bias, k, ip=ip, **kw)
            for q in range(nq):
                pos = probed_positions(off, pr[q], n)
                same((gv[q], gi[q]), brute(vals[q], pos[allow[pos]], k, ip))


@pytest.mark.parametrize("ip", [False, True])
def test_all_zero_mask_is_all_padding(ip):
    rng = np.random.default_rng(9952)
    n = 77
    v = draw_values(rng, 2, n)
    zeros = np.zeros(n, bool)
    off, pr = draw_lists(rng, n, 7), draw_probes(rng, 2, 7, 3)
    bias = np.ones(pr.shape, np.float32)
    for got in (ref_masked_search(v, zeros, 5, ip=ip), ref_masked_lists_search(v, zeros, off, pr, 5, ip=ip),
                ref_masked_residual_search(v, zeros, off, pr, bias, 5, terms=np.ones(n, np.float32), scales=None, ip=ip)):
        assert (got[1] == -1).all() and (got[0] == (-np.inf if ip else np.inf)).all()


def test_pack_ref_by_hand():
    assert pack_ref([True]).tolist() == [1]
    assert pack_ref([False]).tolist() == [0]
    assert pack_ref(np.ones(31, bool)).tolist() == [0x7fffffff]
    assert pack_ref(np.ones(32, bool)).tolist() == [0xffffffff]
    assert pack_ref(np.ones(33, bool)).tolist() == [0xffffffff, 1]
    assert pack_ref(np.ones(64, bool)).tolist() == [0xffffffff, 0xffffffff]
    assert pack_ref(np.ones(65, bool)).tolist() == [0xffffffff, 0xffffffff, 1]
    for n in (1, 31, 32, 33, 64, 65):
        a = np.zeros(n, bool)
        a[n - 1] = True                                   # only the last row: bit (n - 1) & 31 of word (n - 1) >> 5
        w = pack_ref(a)
        assert w.dtype == np.uint32 and w.size == (n + 31) // 32
        want = [0] * w.size
        want[(n - 1) >> 5] = 1 << ((n - 1) & 31)
        assert w.tolist() == want
        assert np.array_equal(unpack_ref(w, n), a)
    a = np.zeros(65, bool)
    a[[0, 31, 32, 64]] = True
    assert pack_ref(a).tolist() == [0x80000001, 1, 1]
    assert pack_ref(a, perm=np.arange(64, -1, -1)).tolist() == [1, 3, 1]   # position p holds row 64 - p: 64, 33, 32, 0
    assert pack_ref(np.zeros(0, bool)).size == 0


def test_row_filter_permutation_identity_on_ivf_layout():
    """what a partitioned matrix packs: bit p = allow[ids[p]], ids the permutation of ivf_layout"""
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(9953)
    for n, n_lists in ((1, 1), (65, 3), (1000, 37)):
        assign = rng.integers(0, n_lists, n)
        perm, off = ivf_layout(assign, n_lists)
        allow = rng.random(n) < 0.4
        bits = unpack_ref(pack_ref(allow, perm), n)
        assert np.array_equal(bits, allow[perm])
        for p in (0, n // 2, n - 1):
            assert bits[p] == allow[perm[p]]
        # the allowed rows of list l are the allowed positions of [off[l], off[l + 1]), mapped back
        for l in range(n_lists):
            pos = np.arange(off[l], off[l + 1])
            assert sorted(perm[pos[bits[pos]]].tolist()) == np.flatnonzero(allow & (assign == l)).tolist()


def test_header_exports_and_library_declare_the_masked_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "with every disallowed row removed, indices mapped back" in flat
    assert "Per-query masks are out of scope" in flat
    assert "d_allow == NULL means no filter" in flat


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    head = (None, 0, None, 1, None, 1, 10, 4, None)                   # .., codes_row_stride, d_allow
    lists = (None, 2, None, 1, 1)
    assert L.pqhip_adc_search_masked_f32_dev(*head, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_masked_f32_dev(*head, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_search_lists_masked_f32_dev(*head, *lists, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_masked_f32_dev(*head, *lists, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_search_lists_residual_masked_f32_dev(*head, *lists, None, 1, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_residual_masked_f32_dev(*head, *lists, None, 1, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_pack_row_mask_dev(None, 0, None, 10, None, 10, None, z) == _lib.EINVAL


def test_python_wrappers_take_the_mask():
    import inspect
    from reductive_amd import Pq, qmatrix
    for name in ("adc_search_device", "adc_ip_search_device", "adc_search_lists_device", "adc_ip_search_lists_device",
                 "adc_search_lists_residual_device", "adc_ip_search_lists_residual_device"):
        assert inspect.signature(getattr(Pq, name)).parameters["allow"].default is None, name
    assert hasattr(Pq, "pack_row_mask_device")
    for cls in (qmatrix.QuantizedMatrix, qmatrix.PartitionedMatrix, qmatrix.ResidualPartitionedMatrix):
        assert hasattr(cls, "row_filter")
        for name in ("nearest", "most_similar"):
            assert inspect.signature(getattr(cls, name)).parameters["allow"].default is None, (cls, name)
