"""4-bit packed codes on the CPU (include/pqhip.h, "4-bit packed codes"): the numpy helpers against the reference of
tests/adc_packed4_ref.py, the surface (header, EXPORTS, library, Rust declarations, the option), the status codes that
need no device, and the tie-in of the packed reference to the existing search references -- a packed search is the
existing search on the unpacked codes, so unpack_ref(pack_ref(codes)) fed to them must change nothing."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from adc_ip_ref import ref_ip_search, scores
from adc_lists_ref import ref_lists_search
from adc_masked_ref import ref_masked_lists_search, ref_masked_residual_search, ref_masked_search
from adc_packed4_ref import pack_ref, unpack_ref
from adc_residual_ref import ref_residual_search
from oracle import pq_oracle as orc
from test_gpu_adc_search import ref_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCHES = ("pqhip_adc_search_packed4_f32_dev", "pqhip_adc_ip_search_packed4_f32_dev",
            "pqhip_adc_search_lists_packed4_f32_dev", "pqhip_adc_ip_search_lists_packed4_f32_dev",
            "pqhip_adc_search_lists_residual_packed4_f32_dev", "pqhip_adc_ip_search_lists_residual_packed4_f32_dev")
NAMES = ("pqhip_pack_codes4_dev", "pqhip_unpack_codes4_dev") + SEARCHES
DEFINITION = ("the result of a packed call equals, bit for bit, values and indices and padding, the result of the "
              "corresponding existing entry point on the unpacked u8 codes with the same tables, probes, biases, row terms, "
              "scales and mask")
MS = (1, 2, 3, 15, 16, 17, 100)
KS = (2, 3, 16)


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def draw_codes(seed, n, M, K):
    c = np.random.default_rng(seed).integers(0, K, (n, M)).astype(np.uint8)
    if n:
        c[0] = K - 1           # every nibble at its largest value once
    return c


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_helpers_equal_the_reference_and_round_trip(ra, M, K):
    for n in (0, 1, 37):
        codes = draw_codes(100 * M + K, n, M, K)
        want = pack_ref(codes, K)
        got = ra.pack_codes4(codes, n_centroids=K)
        assert got.dtype == np.uint8 and got.shape == (n, (M + 1) // 2)
        assert np.array_equal(got, want)
        assert np.array_equal(ra.pack_codes4(codes.astype(np.int32), n_centroids=K), want)   # any integer width
        back = ra.unpack_codes4(got, M)
        assert back.dtype == np.uint8 and np.array_equal(back, codes)
        assert np.array_equal(unpack_ref(want, M), codes)
        if M % 2 and n:
            assert (got[:, -1] >> 4 == 0).all(), "the pad nibble is written as 0"
            dirty = got.copy()
            dirty[:, -1] |= 0xf0
            assert np.array_equal(ra.unpack_codes4(dirty, M), codes), "the pad nibble is ignored"
            assert np.array_equal(unpack_ref(dirty, M), codes)
    one = draw_codes(7, 1, M, K)[0]
    assert np.array_equal(ra.unpack_codes4(ra.pack_codes4(one, n_centroids=K), M), one)            # a single row


def test_format_by_hand(ra):
    codes = np.array([[1, 2, 3, 4, 5]], np.uint8)
    want = np.array([[0x21, 0x43, 0x05]], np.uint8)
    assert np.array_equal(pack_ref(codes), want) and np.array_equal(ra.pack_codes4(codes), want)
    assert np.array_equal(ra.unpack_codes4(np.array([[0x21, 0x43, 0xf5]], np.uint8), 5), codes)


def test_packer_raises_on_a_code_out_of_range(ra):
    for K in KS:
        codes = np.zeros((3, 5), np.uint8)
        codes[2, 4] = K
        with pytest.raises(ra.PanicError):
            ra.pack_codes4(codes, n_centroids=K)
        with pytest.raises(ValueError):
            pack_ref(codes, K)
    with pytest.raises(ra.PanicError):
        ra.pack_codes4(np.zeros((1, 4), np.uint8), n_centroids=17)
    with pytest.raises(ra.PanicError):
        ra.pack_codes4(np.full((1, 4), -1, np.int32))
    with pytest.raises(ra.PanicError):
        ra.unpack_codes4(np.zeros((2, 3), np.uint8), 4)                # 4 codes are 2 bytes


def test_header_exports_library_and_rust_declare_the_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert DEFINITION in flat
    assert "IGNORED by every reader" in flat
    for text in (hdr, rust, open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()):
        assert '"adc_packed4_wgs"' in text
    assert "adc_packed4_wgs" not in open(os.path.join(ROOT, "tests", "conftest.py")).read()


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    head = (None, 0, None, 1, None, 10, 4, None)                      # .., d_packed, n_codes, packed_row_stride, d_allow
    lists = (None, 2, None, 1, 1)
    assert L.pqhip_adc_search_packed4_f32_dev(*head, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_packed4_f32_dev(*head, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_search_lists_packed4_f32_dev(*head, *lists, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_packed4_f32_dev(*head, *lists, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_search_lists_residual_packed4_f32_dev(*head, *lists, None, 1, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_residual_packed4_f32_dev(*head, *lists, None, 1, None, 5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_pack_codes4_dev(None, 0, None, 1, 10, 4, None, 2, z) == _lib.EINVAL
    assert L.pqhip_unpack_codes4_dev(None, 0, None, 10, 2, None, 0, None, 4, z) == _lib.EINVAL


def test_python_surface():
    from reductive_amd import Pq, qmatrix
    for name in ("adc_search_device", "adc_ip_search_device", "adc_search_lists_device", "adc_ip_search_lists_device",
                 "adc_search_lists_residual_device", "adc_ip_search_lists_residual_device"):
        assert inspect.signature(getattr(Pq, name)).parameters["packed4"].default is False, name
    assert hasattr(Pq, "pack_codes4_device") and hasattr(Pq, "unpack_codes4_device")
    for cls in (qmatrix.QuantizedMatrix, qmatrix.PartitionedMatrix, qmatrix.ResidualPartitionedMatrix):
        assert cls.packed4 is False
        assert callable(cls.pack4) and callable(cls.unpack4)
        for name in ("within", "similar_above"):
            assert "unpack4()" in getattr(cls, name).__doc__, (cls, name)
    for name in ("distances", "inner_products", "partition", "partition_residual"):
        assert "unpack4()" in getattr(qmatrix.QuantizedMatrix, name).__doc__, name


def test_more_than_16_centroids_raise_before_any_device_call(ra):
    """K = 32: every packed4=True call and both device converters raise PanicError on their first line -- the arguments
    are not even tensors, so nothing could have reached the device."""
    rng = np.random.default_rng(5)
    pq = ra.Pq(None, rng.standard_normal((4, 32, 2)).astype(np.float32))
    for call in (lambda: pq.adc_search_device(None, None, 5, packed4=True),
                 lambda: pq.adc_ip_search_device(None, None, 5, packed4=True),
                 lambda: pq.adc_search_lists_device(None, None, None, None, 5, packed4=True),
                 lambda: pq.adc_ip_search_lists_device(None, None, None, None, 5, packed4=True),
                 lambda: pq.adc_search_lists_residual_device(None, None, None, None, 0, 0, 5, packed4=True),
                 lambda: pq.adc_ip_search_lists_residual_device(None, None, None, None, 0, 5, packed4=True),
                 lambda: pq.pack_codes4_device(None),
                 lambda: pq.unpack_codes4_device(None)):
        with pytest.raises(ra.PanicError, match="16 centroids"):
            call()


def same(got, want):
    (gv, gi), (wv, wi) = got, want
    assert np.array_equal(gi, wi)
    assert np.asarray(gv, np.float32).tobytes() == np.asarray(wv, np.float32).tobytes()


@pytest.mark.parametrize("M,K", [(5, 3), (16, 16), (17, 2)])
def test_packed_reference_is_the_existing_reference(M, K):
    """The existing references fed unpack_ref(pack_ref(codes)) return what they return for codes: the scan values are
    the oracle's over either, and every search reference -- plain, masked, lists, residual -- is a function of those."""
    rng = np.random.default_rng(1000 * M + K)
    n, nq, k, n_lists = 300, 3, 10, 7
    codes = draw_codes(M + K, n, M, K)
    tables = rng.integers(-3, 4, (nq, M, K)).astype(np.float32)      # integer-valued: ties at the k-th place
    again = unpack_ref(pack_ref(codes, K), M)
    assert np.array_equal(again, codes)
    va, vb = orc.adc_scan(tables, codes), orc.adc_scan(tables, again)
    assert va.tobytes() == vb.tobytes()
    scales = rng.standard_normal(n).astype(np.float32)
    terms = rng.standard_normal(n).astype(np.float32)
    allow = rng.random(n) < 0.5
    cuts = np.sort(rng.integers(0, n + 1, n_lists - 1))
    list_off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    probes = np.stack([rng.permutation(n_lists)[:3] for _ in range(nq)]).astype(np.int64)
    probes[0, 1] = -1
    bias = rng.standard_normal(probes.shape).astype(np.float32)
    same(ref_search(vb, k), ref_search(va, k))
    same(ref_ip_search(scores(vb, scales), k), ref_ip_search(scores(va, scales), k))
    same(ref_masked_search(vb, allow, k), ref_masked_search(va, allow, k))
    same(ref_masked_search(scores(vb, scales), allow, k, ip=True), ref_masked_search(scores(va, scales), allow, k, ip=True))
    for ip in (False, True):
        same(ref_lists_search(vb, list_off, probes, k, ip=ip), ref_lists_search(va, list_off, probes, k, ip=ip))
        same(ref_masked_lists_search(vb, allow, list_off, probes, k, ip=ip),
             ref_masked_lists_search(va, allow, list_off, probes, k, ip=ip))
        kw = dict(scales=scales, ip=True) if ip else dict(terms=terms)
        same(ref_residual_search(vb, list_off, probes, bias, k, **kw), ref_residual_search(va, list_off, probes, bias, k, **kw))
        same(ref_masked_residual_search(vb, allow, list_off, probes, bias, k, **kw),
             ref_masked_residual_search(va, allow, list_off, probes, bias, k, **kw))
