"""Row compaction, CPU side: the reference of tests/rows_compact_ref.py tied to ivf_layout (compacting a list-ordered array
under a position-order mask, ids renumbered by rank, is the layout of the kept rows under their assignments); header,
EXPORTS, library and rust/pqhip_ffi.rs name the entry point and its option; the header states the capacity rule and the
validity rule; the argument checks that a null codebook reaches; the wrapper's shape and dtype checks, which come before
any device call.  (Everything that needs a codebook handle: tests/test_gpu_rows_compact.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from rows_compact_ref import pack_words, ref_compact, unpack_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_rows_compact_dev"


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def test_words_round_trip_and_tail_bits():
    rng = np.random.default_rng(1)
    for n in (0, 1, 31, 32, 33, 70):
        bits = rng.random(n) < 0.5
        for tail in (0, 0xFFFFFFFF, 0xA5A5A5A5):
            words = pack_words(bits, tail)
            assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
            assert np.array_equal(unpack_words(words, n), bits)
    assert pack_words([True, False, True]).tolist() == [5] and pack_words([True] * 3, 0xFFFFFFFF).tolist() == [0xFFFFFFFF]
    assert pack_words([False] * 32 + [True]).tolist() == [0, 1]


@pytest.mark.parametrize("mask", ["random", "ones", "zeros"])
@pytest.mark.parametrize("n_lists,n", [(1, 7), (2, 41), (24, 3001), (300, 3001), (24, 0)])
def test_reference_is_the_layout_of_the_kept_rows(n_lists, n, mask):
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(n_lists * 1000 + n)
    live = rng.random(n_lists) < 0.6                       # some lists are empty from the start
    live[rng.integers(n_lists)] = True
    assign = rng.choice(np.flatnonzero(live), n)
    rows = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if mask == "random":
        flags = rng.random(n) < 0.6
        if n:
            gone = assign[rng.integers(n)]                 # one list is emptied by the mask
            flags[assign == gone] = False
            assert np.any(assign == gone) and not np.any(flags[assign == gone])
    else:
        flags = np.full(n, mask == "ones")
    perm, off = ivf_layout(assign, n_lists)
    keep_pos = flags[perm]                                 # the mask in position order
    out, off_out, src, c = ref_compact(keep_pos, rows[perm], off)
    kept = np.flatnonzero(flags)
    want_perm, want_off = ivf_layout(assign[kept], n_lists)
    assert c == kept.size and np.array_equal(out, rows[kept][want_perm])
    assert np.array_equal(off_out, want_off)
    assert np.array_equal(src, np.flatnonzero(keep_pos))
    # the row numbers compact the same way and are renumbered by their rank among the kept rows
    rank = np.cumsum(flags) - 1
    ids = ref_compact(keep_pos, perm)[0]
    assert np.array_equal(rank[ids], want_perm)
    if mask == "ones":
        assert np.array_equal(out, rows[perm]) and np.array_equal(off_out, off)
    if mask == "zeros":
        assert c == 0 and not off_out.any()


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
    assert len(fn.argtypes) == 14 and fn.argtypes[4] is ctypes.c_int64 and fn.argtypes[-1] is ctypes.c_void_p
    assert '"rows_compact_wgs"' in hdr and '"rows_compact_wgs"' in ffi
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    # the capacity rule and the validity rule
    assert "If c > out_capacity_rows, no byte of d_out or d_src_rows is written and no flag is raised" in flat
    assert "valid iff off[0] == 0, it is non-decreasing and off[n_lists] == n" in flat
    assert "If it is invalid, no byte of d_out or d_src_rows is written" in flat
    assert "bits of the last word at or beyond n are ignored" in flat
    assert "#define PQHIP_ROWS_COMPACT_MAX_ROW_BYTES 4096" in hdr


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    fn = L.pqhip_rows_compact_dev
    assert fn(None, 0, None, 0, 1, None, None, 0, None, 0, None, None, p, z) == _lib.EINVAL
    assert fn(None, 0, p, 3, 15, p, p, 3, p, 2, p, p, p, z) == _lib.EINVAL
    assert fn(None, 7, p, -1, 0, p, None, -1, None, -1, p, None, None, z) == _lib.EINVAL
    assert fn(None, 0, p, 3, 8192, p, p, 3, p, 1 << 40, p, p, p, z) == _lib.EINVAL


def test_wrapper_checks_shapes_before_any_device_call(ra):
    """CPU tensors throughout: a mismatch must be refused before the wrapper asks for a device, a handle or a stream"""
    import torch
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))
    words = torch.zeros(2, dtype=torch.int32)
    u8 = torch.zeros((37, 15), dtype=torch.uint8)
    off = torch.zeros(4, dtype=torch.int64)
    compact = pq.compact_rows_device
    with pytest.raises(ra.PanicError, match="torch tensor"):
        compact(words, np.zeros((37, 15), np.uint8))
    with pytest.raises(ra.PanicError, match="torch tensor"):
        compact(np.zeros(2, np.int32), u8)
    with pytest.raises(ra.PanicError, match="vector or a matrix"):
        compact(words, torch.zeros((37, 3, 5), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="between 1 and 4096 bytes"):
        compact(words, torch.zeros((37, 513), dtype=torch.int64))
    with pytest.raises(ra.PanicError, match="between 1 and 4096 bytes"):
        compact(words, torch.zeros((37, 0), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="ceil\\(n / 32\\) int32 words"):
        compact(words[:1], u8)
    with pytest.raises(ra.PanicError, match="ceil\\(n / 32\\) int32 words"):
        compact(words, torch.zeros((65, 15), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="ceil\\(n / 32\\) int32 words"):
        compact(words.long(), u8)
    with pytest.raises(ra.PanicError, match="ceil\\(n / 32\\) int32 words"):
        compact(words, None, n=65)
    with pytest.raises(ra.PanicError, match="plan-only"):
        compact(words, None)
    with pytest.raises(ra.PanicError, match="number of rows"):
        compact(words, u8, n=36)
    with pytest.raises(ra.PanicError, match="n_lists \\+ 1"):
        compact(words, u8, list_off=off.int())
    with pytest.raises(ra.PanicError, match="n_lists \\+ 1"):
        compact(words, u8, list_off=off[:0])
    with pytest.raises(ra.PanicError, match="capacity must not be negative"):
        compact(words, u8, capacity=-1)
    with pytest.raises(ra.PanicError, match="out must be"):
        compact(words, u8, out=torch.zeros((37, 16), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="out must be"):
        compact(words, u8, out=torch.zeros((37, 15), dtype=torch.int8))
    with pytest.raises(ra.PanicError, match="fewer rows than the capacity"):
        compact(words, u8, capacity=30, out=torch.zeros((29, 15), dtype=torch.uint8))
    with pytest.raises(ra.PanicError, match="contiguous"):
        compact(words, torch.zeros((37, 30), dtype=torch.uint8)[:, ::2])
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        compact(words, u8, list_off=off, want_src_rows=True)
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        compact(words, None, n=37)
    assert pq._handle is None                    # no codebook handle was created: nothing reached the library
