"""The list layout on the GPU (include/pqhip.h: pqhip_lists_layout_dev, Pq.lists_layout_device).  Reference: ivf_layout in
numpy (tests/test_index_build.py pins the element-by-element reference against it).  Every comparison is exact, and the
entry point is called with guard elements around all four outputs.  Covered: n in {0, 1, 63, 64, 65, 1023, 1024, 1025,
5000, 70001} (the wave, the tile of 256 rows x 4 and the slice boundaries) x 1 .. 16,384 lists x int32 / int64 ids x the
patterns of tests/lists_layout_ref.py (uniform, one list, ascending, descending, runs of 64 and of 65, two ids
alternating, only the first and the last list); one result for every forced grid (option "lists_layout_wgs"); ids -1
and n_lists at the first, the last and a middle row (nothing written, the range flag, a valid call afterwards); the
statuses; the empty layout."""
import ctypes

import numpy as np
import pytest

import synth
from lists_layout_ref import PATTERNS, pattern

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000, 70001)
LISTS = (1, 2, 24, 300, 16384)
GUARD, SENT = 16, -0x5A5A5A5A5A5A5A5B


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
    return ra.Pq(None, synth.normalish(5000, (2, 16, 4)))


def guarded(n):
    import torch
    return torch.full((n + 2 * GUARD,), SENT, dtype=torch.int64, device="cuda")


def raw_layout(ra, pq, assign_t, n_lists, with_lists=True):
    """the C entry point with guard elements around every output -> (status, list_off, ids, positions, lists) buffers"""
    import torch
    n = assign_t.shape[0]
    off, ids, pos, lists = guarded(n_lists + 1), guarded(n), guarded(n), guarded(n)
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ra.lib().pqhip_lists_layout_dev(pq._cb(), 0, assign_t.data_ptr() if n else None, assign_t.element_size(), n, n_lists,
                                         off.data_ptr() + 8 * GUARD, ids.data_ptr() + 8 * GUARD if n else None,
                                         pos.data_ptr() + 8 * GUARD if n else None,
                                         lists.data_ptr() + 8 * GUARD if with_lists and n else None, z)
    return rc, off, ids, pos, lists


def inner(buf):
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENT) and np.all(got[-GUARD:] == SENT)          # the guard elements on both sides
    return got[GUARD:-GUARD]


def check_layout(ra, pq, a, n_lists, dtype, with_lists=True):
    import torch
    from reductive_amd import _lib
    from reductive_amd.qmatrix import ivf_layout
    perm, list_off = ivf_layout(a, n_lists)
    t = torch.from_numpy(a.astype(dtype)).cuda()
    rc, off, ids, pos, lists = raw_layout(ra, pq, t, n_lists, with_lists)
    assert rc == _lib.OK
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ra.lib().pqhip_check_codes_dev(pq._cb(), 0, z) == _lib.OK
    what = (a.size, n_lists, np.dtype(dtype).name)
    assert np.array_equal(inner(off), list_off), what
    assert np.array_equal(inner(ids), perm), what
    want_pos = np.empty(a.size, np.int64)
    want_pos[perm] = np.arange(a.size)
    assert np.array_equal(inner(pos), want_pos), what
    if with_lists:
        assert np.array_equal(inner(lists), a[perm]), what
    else:
        assert np.all(lists.cpu().numpy() == SENT)
    return inner(ids)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n_lists", LISTS)
def test_sizes_lists_widths_and_patterns(ra, pq, n_lists, dtype):
    rng = np.random.default_rng(5100 + n_lists)
    ra.launch_log(reset=True)
    for n in NS:
        for kind in PATTERNS:
            check_layout(ra, pq, pattern(kind, n, n_lists, rng), n_lists, dtype)
    log = ra.launch_log(reset=True)
    for k in ("k_layout_count", "k_layout_columns", "k_layout_offsets", "k_layout_place"):
        assert k in log


def test_wrapper_and_lists_null(ra, pq):
    import torch
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(5200)
    a = pattern("uniform", 5000, 300, rng)
    perm, list_off = ivf_layout(a, 300)
    for dt in (torch.int32, torch.int64):
        t = torch.from_numpy(a).cuda().to(dt)
        ids, off, pos = pq.lists_layout_device(t, 300, check=True)
        ids2, off2, pos2, lists = pq.lists_layout_device(t, 300, want_lists=True)
        for x in (ids, off, pos, lists):
            assert x.is_cuda and x.dtype == torch.int64 and x.is_contiguous()
        assert np.array_equal(ids.cpu().numpy(), perm) and np.array_equal(off.cpu().numpy(), list_off)
        assert torch.equal(ids, ids2) and torch.equal(off, off2) and torch.equal(pos, pos2)
        assert np.array_equal(pos.cpu().numpy()[perm], np.arange(5000)) and np.array_equal(lists.cpu().numpy(), a[perm])
    check_layout(ra, pq, a, 300, np.int64, with_lists=False)


@pytest.mark.parametrize("n", [5000, 70001])
def test_result_does_not_depend_on_the_grid(ra, pq, n):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(5300 + n)
    for n_lists, kind in ((24, "uniform"), (300, "one_list"), (16384, "uniform"), (2, "alternating"), (300, "runs65")):
        a = pattern(kind, n, n_lists, rng)
        seen = []
        try:
            for wgs in (1, 2, 7, cus, 0):
                ra.set_option("lists_layout_wgs", wgs)
                seen.append(check_layout(ra, pq, a, n_lists, np.int32).tobytes())
        finally:
            ra.set_option("lists_layout_wgs", 0)
        assert len(set(seen)) == 1


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("bad", ["minus_one", "n_lists"])
def test_invalid_ids_write_nothing_and_raise_the_flag(ra, pq, bad, where, dtype):
    import torch
    from reductive_amd import _lib
    rng = np.random.default_rng(5400)
    n, n_lists = 70001, 24
    good = pattern("uniform", n, n_lists, rng)
    a = good.copy()
    a[{"first": 0, "middle": 33333, "last": n - 1}[where]] = -1 if bad == "minus_one" else n_lists
    t = torch.from_numpy(a.astype(dtype)).cuda()
    rc, off, ids, pos, lists = raw_layout(ra, pq, t, n_lists)
    assert rc == _lib.OK                                              # the ids are device memory: the flag reports them
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ra.lib().pqhip_check_codes_dev(pq._cb(), 0, z) == _lib.ECODE_RANGE
    for buf in (ids, pos, lists):
        assert bool((buf == SENT).all())                              # no element was written
    inner(off)                                                        # (contents unspecified; the guards hold)
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.lists_layout_device(t, n_lists, check=True)
    # a valid call on the same stream afterwards is correct, and the flag is down again
    check_layout(ra, pq, good, n_lists, dtype)


def test_statuses_and_the_empty_layout(ra, pq):
    import torch
    from reductive_amd import _lib
    lay = ra.lib().pqhip_lists_layout_dev
    cb = pq._cb()
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.zeros(100, dtype=torch.int64, device="cuda")
    o = torch.zeros(100, dtype=torch.int64, device="cuda")
    p = o.data_ptr()
    assert lay(cb, 0, a.data_ptr(), 2, 100, 5, p, p, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, a.data_ptr(), 8, -1, 5, p, p, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, a.data_ptr(), 8, 100, 0, p, p, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, None, 8, 100, 5, p, p, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, a.data_ptr(), 8, 100, 5, None, p, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, a.data_ptr(), 8, 100, 5, p, None, p, None, z) == _lib.EINVAL
    assert lay(cb, 0, a.data_ptr(), 8, 100, 5, p, p, None, None, z) == _lib.EINVAL
    assert lay(cb, 7, a.data_ptr(), 8, 100, 5, p, p, p, None, z) == _lib.ENODEV
    assert lay(cb, 0, a.data_ptr(), 8, 100, 16385, p, p, p, None, z) == _lib.EUNSUPPORTED
    assert lay(cb, 0, a.data_ptr(), 8, (1 << 49) + 1, 5, p, p, p, None, z) == _lib.EUNSUPPORTED
    assert lay(cb, 7, a.data_ptr(), 2, 100, 16385, p, p, p, None, z) == _lib.EINVAL          # the precedence
    assert lay(cb, 7, a.data_ptr(), 8, 100, 16385, p, p, p, None, z) == _lib.ENODEV
    for n_lists in (1, 300):
        ra.launch_log(reset=True)
        ids, off, pos, lists = pq.lists_layout_device(a[:0], n_lists, want_lists=True, check=True)
        assert ra.launch_log(reset=True) == ""
        assert off.cpu().numpy().tolist() == [0] * (n_lists + 1)
        assert tuple(ids.shape) == tuple(pos.shape) == tuple(lists.shape) == (0,)
