"""The row compaction on the GPU (include/pqhip.h: pqhip_rows_compact_dev, Pq.compact_rows_device).  Reference:
tests/rows_compact_ref.py (pinned against ivf_layout by test_rows_compact.py).  Every comparison is bit for bit, on the
bytes.  Covered: row widths 1 .. 4,096 bytes; n from 0 over the word (32) and the tile (1,024) to 70,001, and 300,001 rows
of 15 bytes for the forced grids; masks all set, all clear, alternating, first row only, last row only, whole words clear,
random at 0.1 / 0.5 / 0.9 and garbage in the tail bits of the last word (the full cross up to 32 MB an array; beyond that
three masks per shape); input and output 1 .. 15 bytes off any alignment with guard bytes around the output; one result
for every forced grid (option "rows_compact_wgs"); a capacity one short of the count (nothing written, the count right,
no flag) and exactly the count; the plan-only call; list offsets of 1 .. 16,384 lists; the three kinds of invalid
offsets (nothing written, the range flag, a valid call afterwards); the source rows; the statuses in their precedence."""
import ctypes

import numpy as np
import pytest

import synth
from lists_merge_ref import random_offsets
from rows_compact_ref import pack_words, ref_compact

pytestmark = pytest.mark.gpu

WIDTHS = (1, 4, 8, 15, 17, 600, 1200, 4096)
NS = (0, 1, 31, 32, 33, 1023, 1024, 1025, 3001, 70001)
LISTS = (1, 2, 24, 300, 16384)


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.fixture(scope="module")
def pq(ra):
    return ra.Pq(None, synth.normalish(4000, (2, 16, 4)))


def masks(rng, n, few=False):
    """(name, keep bits [n], tail bits of the last word)"""
    half = rng.random(n) < 0.5
    words_clear = half.copy()
    for w in rng.integers(0, n // 32 + 1, max(1, n // 64)):
        words_clear[32 * w:32 * w + 32] = False
    out = [("random-0.5", half, 0), ("words-clear", words_clear, 0), ("garbage-tail", rng.random(n) < 0.5, 0xFFFFFFFF)]
    if few:
        return out
    one = lambda i: np.arange(n) == i
    return out + [("ones", np.ones(n, bool), 0), ("zeros", np.zeros(n, bool), 0), ("zeros-garbage-tail", np.zeros(n, bool), 0xDEADBEEF),
                  ("alternating", np.arange(n) % 2 == 0, 0), ("first", one(0), 0), ("last", one(n - 1), 0),
                  ("random-0.1", rng.random(n) < 0.1, 0), ("random-0.9", rng.random(n) < 0.9, 0)]


def words_of(bits, tail=0):
    import torch
    return torch.from_numpy(pack_words(bits, tail).view(np.int32)).cuda()


def as_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def check_compact(pq, bits, tail, rows, rows_d, off=None, **kw):
    import torch
    want, want_off, want_src, c = ref_compact(bits, rows, off)
    off_d = None if off is None else torch.from_numpy(off).cuda()
    out, off_out, src, count = pq.compact_rows_device(words_of(bits, tail), rows_d, list_off=off_d, want_src_rows=True, check=True, **kw)
    assert count == c
    assert tuple(out.shape) == want.shape and out.dtype == rows_d.dtype
    assert as_bytes(out) == want.tobytes()
    assert src.dtype == torch.int64 and np.array_equal(src.cpu().numpy(), want_src)
    if off is None:
        assert off_out is None
    else:
        assert np.array_equal(off_out.cpu().numpy(), want_off)
    return out


@pytest.mark.parametrize("row_bytes", WIDTHS)
def test_widths_sizes_and_masks(ra, pq, row_bytes):
    import torch
    rng = np.random.default_rng(5100 + row_bytes)
    full = rng.integers(0, 256, (max(NS), row_bytes), dtype=np.uint8)
    full_d = torch.from_numpy(full).cuda()
    ra.launch_log(reset=True)               # the log keeps a bounded number of distinct names: start from an empty one
    for n in NS:
        for name, bits, tail in masks(rng, n, few=n * row_bytes > (32 << 20)):
            check_compact(pq, bits, tail, full[:n], full_d[:n])
    assert "k_rows_compact_move" in ra.launch_log(reset=True)


@pytest.mark.parametrize("dtype,cols", [(np.float32, None), (np.int64, None), (np.float16, 24), (np.float32, 24)])
def test_dtypes_and_vectors(pq, dtype, cols):
    """the tensors a matrix stores: norms, ids, attached vectors -- any dtype, [n] or [n, w]"""
    import torch
    rng = np.random.default_rng(5150)
    n = 3001
    width = np.dtype(dtype).itemsize * (cols or 1)
    rows = rng.integers(0, 256, (n, width), dtype=np.uint8).view(dtype).reshape((n,) if cols is None else (n, cols))
    out = check_compact(pq, rng.random(n) < 0.7, 0, rows, torch.from_numpy(rows).cuda())
    assert out.dim() == (1 if cols is None else 2)


@pytest.mark.parametrize("row_bytes", [1, 15, 17, 600])
def test_misaligned_pointers_and_guard_bytes(pq, row_bytes):
    import torch
    rng = np.random.default_rng(5200 + row_bytes)
    n, guard = 3001, 64
    rows = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    bits = rng.random(n) < 0.6
    want, _, _, c = ref_compact(bits, rows)
    words = words_of(bits)
    for s_in in range(1, 16):
        s_out = 7 * s_in % 16                               # every output shift 1 .. 15 over the loop
        ibuf = torch.full((s_in + rows.size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        iv = ibuf[s_in:s_in + rows.size].view(n, row_bytes)
        iv.copy_(torch.from_numpy(rows))
        obuf = torch.full((s_out + n * row_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        ov = obuf[s_out:s_out + n * row_bytes].view(n, row_bytes)
        assert iv.data_ptr() % 16 == s_in and ov.data_ptr() % 16 == s_out
        out, _, _, count = pq.compact_rows_device(words, iv, out=ov, check=True)
        assert count == c and out.data_ptr() == ov.data_ptr() and tuple(out.shape) == (c, row_bytes)
        got = obuf.cpu().numpy()
        assert got[s_out:s_out + want.size].tobytes() == want.tobytes()
        # the guard bytes before the output and from count * row_bytes on
        assert np.all(got[:s_out] == 0xA5) and np.all(got[s_out + want.size:] == 0xA5)
    assert sorted(7 * s % 16 for s in range(1, 16)) == list(range(1, 16))


def test_result_does_not_depend_on_the_grid(ra, pq):
    import torch
    rng = np.random.default_rng(5300)
    n, row_bytes, L = 300001, 15, 24
    rows = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    rows_d = torch.from_numpy(rows).cuda()
    off = random_offsets(rng, n, L)
    seen = set()
    try:
        for name, bits, tail in masks(rng, n, few=True):
            for wgs in (1, 2, 7, 0):
                ra.set_option("rows_compact_wgs", wgs)
                seen.add((name, as_bytes(check_compact(pq, bits, tail, rows, rows_d, off))))
    finally:
        ra.set_option("rows_compact_wgs", 0)
    assert len(seen) == 3                                   # one result per mask


def raw_call(ra, pq, words, n, row_bytes, src, dst, cap, off_in=None, n_lists=0, off_out=None, src_rows=None, count=None, slot=0):
    import torch
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()
    return ra.lib().pqhip_rows_compact_dev(pq._cb(), slot, p(words), n, row_bytes, p(src), p(dst), cap, p(off_in), n_lists,
                                          p(off_out), p(src_rows), p(count), z)


def test_capacity_rule_and_plan_only(ra, pq):
    import torch
    from reductive_amd import _lib
    rng = np.random.default_rng(5400)
    n, row_bytes, L = 3001, 15, 24
    rows = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    bits = rng.random(n) < 0.5
    off = random_offsets(rng, n, L)
    want, want_off, want_src, c = ref_compact(bits, rows, off)
    words, rows_d, off_d = words_of(bits), torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda()
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cap in (c - 1, 0, c, c + 5):
        out = torch.full((n, row_bytes), 0x5A, dtype=torch.uint8, device="cuda")
        src = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        off_out = torch.full((L + 1,), -7, dtype=torch.int64, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        assert raw_call(ra, pq, words, n, row_bytes, rows_d, out, cap, off_d, L, off_out, src, count) == _lib.OK
        assert ra.lib().pqhip_check_codes_dev(pq._cb(), 0, z) == _lib.OK          # too small a capacity raises no flag
        assert int(count) == c and np.array_equal(off_out.cpu().numpy(), want_off)
        if cap < c:
            assert bool((out == 0x5A).all()) and bool((src == -7).all())
        else:
            assert as_bytes(out[:c]) == want.tobytes() and bool((out[c:] == 0x5A).all())
            assert np.array_equal(src[:c].cpu().numpy(), want_src) and bool((src[c:] == -7).all())
    # the wrapper: nothing comes back when the rows do not fit, everything when they fit exactly
    buf = torch.full((c, row_bytes), 0x5A, dtype=torch.uint8, device="cuda")
    out, off_out, src, count = pq.compact_rows_device(words, rows_d, list_off=off_d, want_src_rows=True, capacity=c - 1, out=buf,
                                                      check=True)
    assert out is None and src is None and count == c and bool((buf == 0x5A).all())
    assert np.array_equal(off_out.cpu().numpy(), want_off)
    out, _, src, count = pq.compact_rows_device(words, rows_d, want_src_rows=True, capacity=c, check=True)
    assert count == c and as_bytes(out) == want.tobytes() and np.array_equal(src.cpu().numpy(), want_src)
    # the plan-only call: no rows, no output
    ra.launch_log(reset=True)
    out, off_out, src, count = pq.compact_rows_device(words, None, list_off=off_d, n=n, check=True)
    assert "k_rows_compact_move" not in ra.launch_log(reset=True)
    assert out is None and src is None and count == c and np.array_equal(off_out.cpu().numpy(), want_off)
    out, off_out, src, count = pq.compact_rows_device(words, None, want_src_rows=True, n=n, check=True)
    assert out is None and off_out is None and count == c and np.array_equal(src.cpu().numpy(), want_src)


@pytest.mark.parametrize("n_lists", LISTS)
def test_list_offsets(pq, n_lists):
    import torch
    rng = np.random.default_rng(5500 + n_lists)
    for n in (3001, 70001):
        rows = rng.integers(0, 256, (n, 15), dtype=np.uint8)
        rows_d = torch.from_numpy(rows).cuda()
        for shape in ("random", "edges", "heavy"):
            off = random_offsets(rng, n, n_lists, shape)
            bits = rng.random(n) < 0.5
            if n_lists > 2:                                 # one list is emptied by the mask
                l = int(np.argmax(np.diff(off) > 0))
                bits[off[l]:off[l + 1]] = False
            check_compact(pq, bits, 0, rows, rows_d, off)
        check_compact(pq, np.ones(n, bool), 0, rows, rows_d, off)
        check_compact(pq, np.zeros(n, bool), 0xFFFFFFFF, rows, rows_d, off)


def corrupt(off, kind):
    off = off.copy()
    if kind == "short":
        off[-1] -= 1
    elif kind == "first":
        off[0] = 1
    else:                                   # two adjacent interior entries swapped: the array decreases exactly once
        l = next(l for l in range(1, off.size - 2) if off[l] < off[l + 1])
        off[l], off[l + 1] = off[l + 1], off[l]
        assert np.sum(off[1:] < off[:-1]) == 1
    return off


@pytest.mark.parametrize("kind", ["short", "first", "swapped"])
def test_invalid_offsets_write_nothing_and_raise_the_flag(ra, pq, kind):
    """harmless by construction: the entries stay inside [0, n] and the mover never starts"""
    import torch
    rng = np.random.default_rng(5600)
    n, row_bytes, L = 30011, 15, 24
    rows = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    bits = rng.random(n) < 0.5
    off = random_offsets(rng, n, L)
    bad = corrupt(off, kind)
    assert bad.min() >= 0 and bad.max() <= n
    want, want_off, want_src, c = ref_compact(bits, rows, off)
    words, rows_d = words_of(bits), torch.from_numpy(rows).cuda()
    out = torch.full((n, row_bytes), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.compact_rows_device(words, rows_d, list_off=torch.from_numpy(bad).cuda(), out=out, check=True)
    assert bool((out == 0x5A).all())                             # no byte of the output was written
    src = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    from reductive_amd import _lib
    assert raw_call(ra, pq, words, n, row_bytes, rows_d, out, n, torch.from_numpy(bad).cuda(), L, None, src, count) == _lib.OK
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ra.lib().pqhip_check_codes_dev(pq._cb(), 0, z) == _lib.ECODE_RANGE
    assert bool((out == 0x5A).all()) and bool((src == -7).all())
    # a valid call on the same stream afterwards is correct, and the flag is down again
    got, off_out, _, count = pq.compact_rows_device(words, rows_d, list_off=torch.from_numpy(off).cuda(), out=out, check=True)
    assert count == c and as_bytes(got) == want.tobytes() and np.array_equal(off_out.cpu().numpy(), want_off)


def test_statuses_in_their_precedence(ra, pq):
    import torch
    from reductive_amd import _lib
    n, rb, L = 100, 15, 4
    words = torch.zeros(4, dtype=torch.int32, device="cuda")
    rows = torch.zeros((n, rb), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, rb), dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 10, 10, 50, 100], dtype=torch.int64, device="cuda")
    off_out = torch.zeros(L + 1, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    call = lambda **kw: raw_call(ra, pq, **{**dict(words=words, n=n, row_bytes=rb, src=rows, dst=out, cap=n, off_in=off, n_lists=L,
                                                  off_out=off_out, src_rows=None, count=count), **kw})
    assert call() == _lib.OK
    for kw in (dict(n=-1), dict(row_bytes=0), dict(cap=-1), dict(count=None), dict(n_lists=-1), dict(src=None), dict(dst=None),
               dict(off_in=None), dict(words=None)):
        assert call(**kw) == _lib.EINVAL, kw
        if "row_bytes" not in kw:                               # an invalid argument before the slot and the limits
            assert call(slot=7, row_bytes=4097, **kw) == _lib.EINVAL, kw
    assert call(slot=7) == _lib.ENODEV and call(slot=-1) == _lib.ENODEV
    assert call(slot=7, row_bytes=4097) == _lib.ENODEV          # the slot before the limits
    assert call(row_bytes=4097) == _lib.EUNSUPPORTED
    assert call(n_lists=(1 << 20) + 1) == _lib.EUNSUPPORTED
    assert call(n=(1 << 49) + 1) == _lib.EUNSUPPORTED
    # fine: no offsets at all, offsets in without offsets out, a null mask without rows
    assert call(off_in=None, off_out=None) == _lib.OK and call(off_out=None) == _lib.OK
    assert call(words=None, n=0, src=None, dst=None, off_in=None, off_out=None) == _lib.OK
    torch.cuda.synchronize()


def test_no_rows_launches_nothing(ra, pq):
    import torch
    words = torch.zeros(0, dtype=torch.int32, device="cuda")
    e = torch.zeros((0, 15), dtype=torch.uint8, device="cuda")
    for L in (0, 5):
        off = torch.zeros(L + 1, dtype=torch.int64, device="cuda")
        ra.launch_log(reset=True)
        out, off_out, src, count = pq.compact_rows_device(words, e, list_off=off, want_src_rows=True, check=True)
        assert ra.launch_log(reset=True) == ""
        assert count == 0 and tuple(out.shape) == (0, 15) and out.dtype == torch.uint8 and tuple(src.shape) == (0,)
        assert off_out.cpu().numpy().tolist() == [0] * (L + 1)
