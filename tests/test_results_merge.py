"""Merging search results, CPU side: the reference of tests/results_merge_ref.py applied to per-shard brute-force top-k
results of consecutive row ranges equals the brute-force top-k of the whole (both metrics, values from a small set with
-0, +-Inf and NaN, parts of size 0, 1 and less than k); header, EXPORTS, SIGNATURES, library and rust/pqhip_ffi.rs name the
entry point; the argument checks that a null codebook reaches; the wrapper's shape and dtype checks, which come before
any device call.  (Everything that needs a codebook handle: tests/test_gpu_results_merge.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from results_merge_ref import QNAN, SPECIAL_VALUES, bits, brute_topk, canonical, order_key, ref_merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_topk_merge_f32_dev"


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def test_order_key_and_canonical_values():
    f = np.array([-np.inf, -2.0, -0.25, -0.0, 0.0, 0.25, 2.0, np.inf, np.nan], np.float32)
    key = order_key(f)
    assert key[3] == key[4] == 0x80000000 and key[-1] == 0xFFFFFFFF
    assert np.all(np.diff(key[[0, 1, 2, 3, 5, 6, 7, 8]].astype(np.int64)) > 0)
    odd_nan = np.array([0xFFC12345, 0x7F800001], np.uint32).view(np.float32)
    assert np.all(order_key(odd_nan) == 0xFFFFFFFF)
    assert bits(canonical(odd_nan)).tolist() == [0x7FC00000] * 2 and bits(QNAN) == 0x7FC00000
    assert bits(canonical(np.array([-0.0, 0.0, -1.5], np.float32))).tolist() == [0, 0, 0xBFC00000]


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("splits", [[0, 40], [0, 0, 1, 4, 40], [0, 1, 2, 3, 40, 40], [0, 13, 26, 39, 40], [0, 7, 7, 8, 33, 40]])
@pytest.mark.parametrize("k_in", [1, 5, 12, 64])
def test_reference_merge_of_shards_is_the_search_of_the_whole(k_in, splits, largest):
    rng = np.random.default_rng(k_in * 100 + len(splits))
    n, nq = splits[-1], 9
    values = rng.choice(SPECIAL_VALUES, (nq, n)).astype(np.float32)
    values[0] = np.float32(0.5)                              # one query of ties only
    values[1, ::2] = np.float32(np.nan)
    P = len(splits) - 1
    val = np.empty((P, nq, k_in), np.float32)
    idx = np.empty((P, nq, k_in), np.int64)
    for p in range(P):
        val[p], idx[p] = brute_topk(values[:, splits[p]:splits[p + 1]], k_in, largest)
    sizes = np.diff(splits)
    garbage = rng.choice(SPECIAL_VALUES, val.shape).astype(np.float32)
    val = np.where(idx < 0, garbage, val)                    # an absent entry's value is not looked at
    for k in sorted({1, min(3, k_in), k_in}):
        want_v, want_i = brute_topk(values, k, largest)
        got_v, got_i, got_p = ref_merge(val, idx, k, largest, offsets=splits[:-1])
        assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_i, want_i)
        src = np.searchsorted(np.asarray(splits[1:]), np.maximum(got_i, 0), side="right")
        assert np.array_equal(got_p, np.where(got_i < 0, -1, src))
    # wider than everything there is: padded
    got_v, got_i, got_p = ref_merge(val, idx, P * k_in + 2, largest, offsets=splits[:-1])
    count = int(np.minimum(sizes, k_in).sum())
    assert np.all(got_i[:, count:] == -1) and np.all(got_p[:, count:] == -1) and np.all(got_i[:, :count] >= 0)
    assert np.all(got_v[:, count:] == (-np.inf if largest else np.inf))


def test_reference_ties_go_to_the_earlier_part_and_never_look_at_ids():
    val = np.array([[[1.0, 2.0, 0.0]], [[1.0, 1.0, np.nan]], [[-0.0, 1.0, 2.0]]], np.float32)
    idx = np.array([[[90, 80, -1]], [[5, 4, 3]], [[70, 1, 60]]], np.int64)
    v, i, p = ref_merge(val, idx, 9)
    assert i[0].tolist() == [70, 90, 5, 4, 1, 80, 60, 3, -1] and p[0].tolist() == [2, 0, 1, 1, 2, 0, 2, 1, -1]
    assert bits(v[0]).tolist() == bits(np.array([0, 1, 1, 1, 1, 2, 2, QNAN, np.inf], np.float32)).tolist()
    v, i, p = ref_merge(val, idx, 4, largest=True, offsets=[100, 200, 300])
    assert i[0].tolist() == [180, 360, 190, 205] and p[0].tolist() == [0, 2, 0, 1]


def test_header_exports_library_and_ffi_name_the_entry_point(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    assert NAME in declared and NAME in _lib.EXPORTS and NAME in _lib.SIGNATURES
    assert hasattr(L, NAME)
    assert re.search(r"pub fn %s\(" % NAME, ffi)
    fn = getattr(L, NAME)
    assert len(fn.argtypes) == 21 and fn.argtypes[10] is ctypes.c_int32 and fn.argtypes[-1] is ctypes.c_void_p
    assert '"topk_merge_wgs"' in hdr and '"topk_merge_wgs"' in ffi
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    # the three statements of the definition
    assert "the output is bit for bit that search on the whole matrix for every k <= k_in" in flat
    assert "For any parts the values are those of the union. Ties go to the earlier part." in flat
    assert "gives an unspecified order, but nothing is read or written out of bounds" in flat
    assert "The merge is stable and never compares ids." in flat
    assert "#define PQHIP_TOPK_MERGE_MAX_K 1024" in hdr and "#define PQHIP_TOPK_MERGE_MAX_PARTS 65536" in hdr
    # the new unit stays out of the units the host-only build links, and no existing unit refers to it
    csrc = os.path.join(ROOT, "reductive_amd", "csrc")
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")) and "results_merge" not in name:
            assert "topk_merge_f32" not in open(os.path.join(csrc, name)).read(), name


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    fn = L.pqhip_topk_merge_f32_dev
    assert fn(None, 0, p, 4, 4, p, 4, 4, 1, 1, 4, None, 0, 4, p, 4, p, 4, None, 0, z) == _lib.EINVAL
    assert fn(None, 0, None, 0, 0, None, 0, 0, 1, 0, 1, None, 0, 1, None, 0, None, 0, None, 0, z) == _lib.EINVAL
    assert fn(None, 7, p, 4, 4, p, 4, 4, 0, -1, 0, p, 2, 0, p, 4, p, 4, p, 4, z) == _lib.EINVAL
    assert fn(None, 0, p, 4, 4, p, 4, 4, 1 << 20, 1, 4096, None, 1, 4096, p, 4, p, 4, None, 0, z) == _lib.EINVAL


def test_wrapper_checks_shapes_before_any_device_call(ra):
    """CPU tensors throughout: a mismatch must be refused before the wrapper asks for a device, a handle or a stream"""
    import torch
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))
    vals = torch.zeros((3, 5, 7), dtype=torch.float32)
    ids = torch.zeros((3, 5, 7), dtype=torch.int64)
    merge = pq.merge_topk_device
    with pytest.raises(ra.PanicError, match="torch tensor"):
        merge(np.zeros((3, 5, 7), np.float32), ids, 4)
    with pytest.raises(ra.PanicError, match="torch tensor"):
        merge(vals, ids.numpy(), 4)
    with pytest.raises(ra.PanicError, match="torch tensor"):
        merge(vals, ids, 4, offsets=[0, 1, 2])
    with pytest.raises(ra.PanicError, match="float32 \\[P, nq, k_in\\]"):
        merge(vals.double(), ids, 4)
    with pytest.raises(ra.PanicError, match="float32 \\[P, nq, k_in\\]"):
        merge(vals[0], ids[0], 4)
    with pytest.raises(ra.PanicError, match="int64 of the shape of vals"):
        merge(vals, ids.int(), 4)
    with pytest.raises(ra.PanicError, match="int64 of the shape of vals"):
        merge(vals, ids[:, :, :6], 4)
    with pytest.raises(ra.PanicError, match="between 1 and 65536 parts"):
        merge(vals[:0], ids[:0], 4)
    with pytest.raises(ra.PanicError, match="between 1 and 1024 entries"):
        merge(vals[:, :, :0], ids[:, :, :0], 4)
    with pytest.raises(ra.PanicError, match="between 1 and 1024 entries"):
        merge(torch.zeros((1, 1, 1025)), torch.zeros((1, 1, 1025), dtype=torch.int64), 4)
    for k in (0, -1, 1025):
        with pytest.raises(ra.PanicError, match="k must be between 1 and 1024"):
            merge(vals, ids, k)
    with pytest.raises(ra.PanicError, match="one per part"):
        merge(vals, ids, 4, offsets=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ra.PanicError, match="one per part"):
        merge(vals, ids, 4, offsets=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        merge(vals, ids, 4, offsets=torch.zeros(3, dtype=torch.int64), want_parts=True)
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        merge(vals, ids, 40, largest=True)
    assert pq._handle is None                    # no codebook handle was created: nothing reached the library
