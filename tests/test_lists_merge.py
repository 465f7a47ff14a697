"""List merge, CPU side: the reference of tests/lists_merge_ref.py tied to ivf_layout (merging two list-ordered arrays is
the layout of the concatenated rows under the concatenated assignments); header, EXPORTS, library and rust/pqhip_ffi.rs
name the entry point and its option; the argument checks that a null codebook reaches; the wrapper's shape and dtype
checks, which come before any device call.  (Everything that needs a codebook handle: tests/test_gpu_lists_merge.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from lists_merge_ref import random_offsets, ref_merge, ref_valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_lists_merge_dev"


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.mark.parametrize("n_lists,n_a,n_b", [(1, 7, 5), (2, 40, 1), (24, 3001, 997), (300, 3001, 63), (24, 0, 50), (24, 50, 0),
                                             (5, 0, 0)])
def test_reference_is_the_layout_of_the_concatenation(n_lists, n_a, n_b):
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(n_lists * 1000 + n_a + n_b)
    live = rng.random(n_lists) < 0.6                       # some lists stay empty in a, in b or in both
    live[rng.integers(n_lists)] = True
    ids = np.flatnonzero(live)
    assign_a = rng.choice(ids, n_a)
    assign_b = rng.choice(np.flatnonzero(live | (rng.random(n_lists) < 0.3)), n_b)
    rows_a = rng.integers(0, 256, (n_a, 3)).astype(np.uint8)
    rows_b = rng.integers(0, 256, (n_b, 3)).astype(np.uint8)
    perm_a, off_a = ivf_layout(assign_a, n_lists)
    perm_b, off_b = ivf_layout(assign_b, n_lists)
    out, off = ref_merge(off_a, rows_a[perm_a], off_b, rows_b[perm_b])
    perm, list_off = ivf_layout(np.concatenate([assign_a, assign_b]), n_lists)
    assert np.array_equal(out, np.concatenate([rows_a, rows_b])[perm])
    assert np.array_equal(off, list_off)
    # the row numbers merge the same way: those of b renumbered from n_a
    ids_out, _ = ref_merge(off_a, perm_a, off_b, perm_b + n_a)
    assert np.array_equal(ids_out, perm)


def test_validity_rule_and_offset_shapes():
    assert ref_valid([0], 0) and ref_valid([0, 0, 3, 3, 7], 7)
    assert not ref_valid([0, 3, 6], 7)           # ends one short
    assert not ref_valid([1, 3, 7], 7)           # does not start at 0
    assert not ref_valid([0, 5, 3, 7], 7)        # decreases once
    assert not ref_valid([0, 3, 8], 7) and not ref_valid([0, -1, 7], 7)
    rng = np.random.default_rng(3)
    for shape in ("random", "edges", "heavy"):
        for n_lists in (1, 2, 24, 300):
            off = random_offsets(rng, 1000, n_lists, shape)
            assert off.shape == (n_lists + 1,) and ref_valid(off, 1000)
            if shape == "edges" and n_lists > 2:
                assert off[1] == 0 and off[-2] == 1000
            if shape == "heavy" and n_lists > 1:
                assert np.diff(off).max() >= 900


def test_header_exports_library_and_ffi_name_the_entry_point(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    assert NAME in declared and NAME in _lib.EXPORTS
    assert hasattr(L, NAME)
    assert re.search(r"pub fn %s\(" % NAME, ffi)
    fn = getattr(L, NAME)
    assert len(fn.argtypes) == 13 and fn.argtypes[7] is ctypes.c_int64 and fn.argtypes[-1] is ctypes.c_void_p
    assert '"lists_merge_wgs"' in hdr and '"lists_merge_wgs"' in ffi
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "valid iff off[0] == 0, it is non-decreasing and off[n_lists] == n" in flat
    assert "no byte of d_out is written" in flat
    m = re.search(r"#define PQHIP_LISTS_MERGE_MAX_LISTS (\d+)", hdr)
    assert m and int(m.group(1)) >= 16384
    assert "#define PQHIP_LISTS_MERGE_MAX_ROW_BYTES 4096" in hdr


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    assert L.pqhip_lists_merge_dev(None, 0, None, 0, None, 0, 0, 1, None, None, None, None, z) == _lib.EINVAL
    assert L.pqhip_lists_merge_dev(None, 0, p, 3, p, 4, 2, 15, p, p, p, p, z) == _lib.EINVAL
    assert L.pqhip_lists_merge_dev(None, 7, p, -1, p, 4, 2, 0, p, p, p, None, z) == _lib.EINVAL
    assert L.pqhip_lists_merge_dev(None, 0, p, 3, p, 4, 1 << 40, 8192, p, p, p, p, z) == _lib.EINVAL


def test_wrapper_checks_shapes_before_any_device_call(ra):
    """CPU tensors throughout: a mismatch must be refused before the wrapper asks for a device, a handle or a stream"""
    import torch
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))
    off = torch.zeros(4, dtype=torch.int64)
    u8 = torch.zeros((5, 15), dtype=torch.uint8)
    merge = pq.merge_lists_device
    with pytest.raises(ra.PanicError, match="one dtype"):
        merge(off, u8, off, torch.zeros((5, 15), dtype=torch.int8))
    with pytest.raises(ra.PanicError, match="one dtype"):
        merge(off, torch.zeros(5), off, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ra.PanicError, match="same number of columns"):
        merge(off, u8, off, torch.zeros((5, 16), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="same number of columns"):
        merge(off, u8, off, torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="same number of columns"):
        merge(off, torch.zeros((5, 3, 5), dtype=torch.uint8), off, torch.zeros((5, 3, 5), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="one length"):
        merge(off, u8, torch.zeros(5, dtype=torch.int64), u8)
    with pytest.raises(ra.PanicError, match="one length"):
        merge(off.int(), u8, off.int(), u8)
    with pytest.raises(ra.PanicError, match="one length"):
        merge(off[:0], u8, off[:0], u8)
    with pytest.raises(ra.PanicError, match="between 1 and 4096 bytes"):
        merge(off, torch.zeros((5, 513), dtype=torch.int64), off, torch.zeros((2, 513), dtype=torch.int64))
    with pytest.raises(ra.PanicError, match="at least one list"):
        merge(off[:1], u8, off[:1], u8)
    with pytest.raises(ra.PanicError, match="out must be"):
        merge(off, u8, off, u8, out=torch.zeros((9, 15), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="out must be"):
        merge(off, u8, off, u8, out=torch.zeros((10, 15), dtype=torch.int8))
    with pytest.raises(ra.PanicError, match="contiguous"):
        merge(off, torch.zeros((5, 30), dtype=torch.uint8)[:, ::2], off, u8)
    with pytest.raises(ra.PanicError, match="torch tensor"):
        merge(off, np.zeros((5, 15), np.uint8), off, u8)
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        merge(off, u8, off, u8)
    assert pq._handle is None                    # no codebook handle was created: nothing reached the library
