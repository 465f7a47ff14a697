"""The list merge on the GPU (include/pqhip.h: pqhip_lists_merge_dev, Pq.merge_lists_device).  Reference:
tests/lists_merge_ref.py (pinned against ivf_layout by test_lists_merge.py).  Every comparison is bit for bit, on the bytes.
Covered: row widths 1 .. 4,096 bytes through uint8 / float32 / int64 vectors and [n, M] matrices; 1 .. 16,384 lists;
n_a = 30,011 with n_b in {0, 1, 63, 1025, 9973} and n_a = 0 (the full cross of widths <= 60, lists and n_b; at 4,096
bytes, 123 MB a case, one case per number of lists and per n_b); lists empty in a, in b, in both, at both ends, one list
with 90 % of the rows, list sizes around the wave and the pass; all three pointers one byte (and 3 / 5 / 9 bytes) off any
alignment with guard bytes around the output; one result for every forced grid (option "lists_merge_wgs"); invalid
offsets inside [0, n] (nothing written, the range flag, a valid call afterwards); d_off_out null and given; the empty
merge; the statuses."""
import ctypes

import numpy as np
import pytest

import synth
from lists_merge_ref import random_offsets, ref_merge

pytestmark = pytest.mark.gpu

N_A = 30011
N_BS = (0, 1, 63, 1025, 9973)
LISTS = (1, 2, 24, 300, 16384)
# row_bytes -> (numpy dtype, columns or None for a vector)
WIDTHS = {1: (np.uint8, None), 3: (np.uint8, 3), 4: (np.float32, None), 8: (np.int64, None), 15: (np.uint8, 15),
          16: (np.uint8, 16), 17: (np.uint8, 17), 60: (np.uint8, 60), 4096: (np.float32, 1024)}


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


def draw_rows(rng, n, row_bytes):
    """n rows of random bytes, seen as the width's dtype (every bit pattern, NaNs included: rows are only copied)"""
    dt, cols = WIDTHS[row_bytes]
    raw = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
    return raw.view(dt).reshape((n,) if cols is None else (n, cols))


def as_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def check_merge(pq, off_a, a, off_b, b, **kw):
    import torch
    want, want_off = ref_merge(off_a, a, off_b, b)
    out, off = pq.merge_lists_device(torch.from_numpy(off_a).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(off_b).cuda(),
                                     torch.from_numpy(b).cuda(), **kw)
    assert tuple(out.shape) == want.shape and out.dtype == torch.from_numpy(a).dtype
    assert as_bytes(out) == want.tobytes(), (a.shape, b.shape, off_a.size - 1)
    assert np.array_equal(off.cpu().numpy(), want_off)
    return out


@pytest.mark.parametrize("row_bytes", sorted(WIDTHS))
def test_widths_lists_and_batch_sizes(ra, pq, row_bytes):
    rng = np.random.default_rng(4100 + row_bytes)
    a = draw_rows(rng, N_A, row_bytes)
    b_all = draw_rows(rng, max(N_BS), row_bytes)
    cases = [(L, nb) for L in LISTS for nb in N_BS] if row_bytes <= 60 else list(zip(LISTS, N_BS))
    ra.launch_log(reset=True)               # the log keeps a bounded number of distinct names: start from an empty one
    for L, nb in cases:
        check_merge(pq, random_offsets(rng, N_A, L), a, random_offsets(rng, nb, L), b_all[:nb])
    for L, nb in ((1, 1), (24, 1025), (16384, 9973)) if row_bytes <= 60 else ((24, 63),):       # n_a = 0 with n_b > 0
        check_merge(pq, np.zeros(L + 1, np.int64), a[:0], random_offsets(rng, nb, L), b_all[:nb])
    assert "k_lists_merge_move" in ra.launch_log(reset=True)


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    return off


@pytest.mark.parametrize("row_bytes", [4, 15])
def test_list_shapes(pq, row_bytes):
    rng = np.random.default_rng(4200 + row_bytes)
    edge = [63, 64, 65, 1023, 1024, 1025]
    # sizes around the wave (64) and the pass (1,024 chunks) on either side, against each other, empty and tiny lists
    sa = edge + [0, 0, 7, 0] + edge[::-1] + [0]
    sb = edge[::-1] + [0, 5, 0, 0] + [0] * 6 + [0]
    for x, y in ((sa, sb), (sb, sa), ([0] + sa + [0], [0] + sb + [0])):
        assert any(p == 0 and q > 0 for p, q in zip(x, y)) and any(p > 0 and q == 0 for p, q in zip(x, y))
        assert any(p == 0 and q == 0 for p, q in zip(x, y))
        check_merge(pq, offsets_of(x), draw_rows(rng, sum(x), row_bytes), offsets_of(y), draw_rows(rng, sum(y), row_bytes))
    a = draw_rows(rng, N_A, row_bytes)
    b = draw_rows(rng, 9973, row_bytes)
    for L in (24, 300):
        for shape_a, shape_b in (("edges", "edges"), ("heavy", "random"), ("random", "heavy"), ("heavy", "heavy"), ("edges", "heavy")):
            off_a, off_b = random_offsets(rng, N_A, L, shape_a), random_offsets(rng, 9973, L, shape_b)
            if shape_a == "edges":
                assert off_a[1] == 0 and off_a[-2] == N_A               # first and last list empty
            if shape_a == "heavy":
                assert np.diff(off_a).max() >= (N_A * 9) // 10          # a list far longer than any slice
            check_merge(pq, off_a, a, off_b, b)


@pytest.mark.parametrize("row_bytes", [15, 16])
@pytest.mark.parametrize("shifts", [(1, 1, 1), (3, 5, 9)])
def test_misaligned_pointers_and_guard_bytes(pq, row_bytes, shifts):
    import torch
    rng = np.random.default_rng(4300 + row_bytes + shifts[2])
    L, nb, guard = 300, 1025, 64
    a, b = draw_rows(rng, N_A, row_bytes), draw_rows(rng, nb, row_bytes)
    off_a, off_b = random_offsets(rng, N_A, L), random_offsets(rng, nb, L)
    want, want_off = ref_merge(off_a, a, off_b, b)

    def shifted(rows, shift):
        buf = torch.full((shift + rows.size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[shift:shift + rows.size].view(rows.shape)
        view.copy_(torch.from_numpy(rows))
        assert view.data_ptr() % 16 == shift
        return buf, view

    _, ad = shifted(a, shifts[0])
    _, bd = shifted(b, shifts[1])
    obuf, od = shifted(np.full_like(want, 0xA5), shifts[2])
    out, off = pq.merge_lists_device(torch.from_numpy(off_a).cuda(), ad, torch.from_numpy(off_b).cuda(), bd, out=od)
    assert out.data_ptr() == od.data_ptr()
    got = obuf.cpu().numpy()
    assert got[shifts[2]:shifts[2] + want.size].tobytes() == want.tobytes()
    assert np.all(got[:shifts[2]] == 0xA5) and np.all(got[shifts[2] + want.size:] == 0xA5)      # the guard bytes on both sides
    assert np.array_equal(off.cpu().numpy(), want_off)


def test_result_does_not_depend_on_the_grid(ra, pq):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(4400)
    for row_bytes, L in ((15, 300), (4, 16384), (17, 24)):
        a, b = draw_rows(rng, N_A, row_bytes), draw_rows(rng, 9973, row_bytes)
        off_a, off_b = random_offsets(rng, N_A, L, "heavy"), random_offsets(rng, 9973, L)
        try:
            for wgs in (1, 2, 7, cus, 0):
                ra.set_option("lists_merge_wgs", wgs)
                check_merge(pq, off_a, a, off_b, b)
        finally:
            ra.set_option("lists_merge_wgs", 0)


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
@pytest.mark.parametrize("which", ["a", "b"])
def test_invalid_offsets_write_nothing_and_raise_the_flag(ra, pq, kind, which):
    import torch
    rng = np.random.default_rng(4500)
    row_bytes, L, nb = 15, 24, 1025
    a, b = draw_rows(rng, N_A, row_bytes), draw_rows(rng, nb, row_bytes)
    off_a, off_b = random_offsets(rng, N_A, L), random_offsets(rng, nb, L)
    n = N_A if which == "a" else nb
    bad = corrupt(off_a if which == "a" else off_b, kind)
    assert bad.min() >= 0 and bad.max() <= n                     # still inside [0, n]: only the plan's rule catches it
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((N_A + nb, row_bytes), 0x5A, dtype=torch.uint8, device="cuda")
    oa = torch.from_numpy(bad if which == "a" else off_a).cuda()
    ob = torch.from_numpy(bad if which == "b" else off_b).cuda()
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.merge_lists_device(oa, ad, ob, bd, out=out, check=True)
    assert bool((out == 0x5A).all())                             # no byte of the output was written
    # a valid call on the same stream afterwards is correct, and the flag is down again
    want, want_off = ref_merge(off_a, a, off_b, b)
    got, off = pq.merge_lists_device(torch.from_numpy(off_a).cuda(), ad, torch.from_numpy(off_b).cuda(), bd, out=out, check=True)
    assert as_bytes(got) == want.tobytes() and np.array_equal(off.cpu().numpy(), want_off)


def test_c_entry_point_offsets_out_null_and_given_and_statuses(ra, pq):
    import torch
    from reductive_amd import _lib
    L_ = ra.lib()
    rng = np.random.default_rng(4600)
    row_bytes, L, nb = 15, 24, 1025
    a, b = draw_rows(rng, N_A, row_bytes), draw_rows(rng, nb, row_bytes)
    off_a, off_b = random_offsets(rng, N_A, L), random_offsets(rng, nb, L)
    want, want_off = ref_merge(off_a, a, off_b, b)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    oa, ob = torch.from_numpy(off_a).cuda(), torch.from_numpy(off_b).cuda()
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cb = pq._cb()
    merge = L_.pqhip_lists_merge_dev
    for with_off in (False, True):
        out = torch.zeros((N_A + nb, row_bytes), dtype=torch.uint8, device="cuda")
        off = torch.full((L + 3,), -7, dtype=torch.int64, device="cuda")
        rc = merge(cb, 0, oa.data_ptr(), N_A, ob.data_ptr(), nb, L, row_bytes, ad.data_ptr(), bd.data_ptr(), out.data_ptr(),
                   off.data_ptr() + 8 if with_off else None, z)
        assert rc == _lib.OK
        assert L_.pqhip_check_codes_dev(cb, 0, z) == _lib.OK
        assert as_bytes(out) == want.tobytes()
        o = off.cpu().numpy()
        if with_off:
            assert o[0] == -7 and o[-1] == -7 and np.array_equal(o[1:-1], want_off)
        else:
            assert np.all(o == -7)
    p = (oa.data_ptr(), N_A, ob.data_ptr(), nb, L)
    io = (ad.data_ptr(), bd.data_ptr(), out.data_ptr(), None, z)
    assert merge(cb, 0, *p, 0, *io) == _lib.EINVAL
    assert merge(cb, 0, oa.data_ptr(), -1, ob.data_ptr(), nb, L, 15, *io) == _lib.EINVAL
    assert merge(cb, 0, oa.data_ptr(), N_A, ob.data_ptr(), nb, -1, 15, *io) == _lib.EINVAL
    assert merge(cb, 0, oa.data_ptr(), N_A, ob.data_ptr(), nb, 0, 15, *io) == _lib.EINVAL        # rows without lists
    assert merge(cb, 7, *p, 15, *io) == _lib.ENODEV
    assert merge(cb, 0, *p, 4097, *io) == _lib.EUNSUPPORTED
    assert merge(cb, 0, oa.data_ptr(), N_A, ob.data_ptr(), nb, (1 << 20) + 1, 15, *io) == _lib.EUNSUPPORTED
    assert merge(cb, 0, None, N_A, ob.data_ptr(), nb, L, 15, *io) == _lib.EINVAL
    assert merge(cb, 0, *p, 15, None, bd.data_ptr(), out.data_ptr(), None, z) == _lib.EINVAL
    assert merge(cb, 0, *p, 15, ad.data_ptr(), None, out.data_ptr(), None, z) == _lib.EINVAL
    assert merge(cb, 0, *p, 15, ad.data_ptr(), bd.data_ptr(), None, None, z) == _lib.EINVAL
    # a null input is fine where it has no rows
    out.zero_()
    zero = torch.zeros(L + 1, dtype=torch.int64, device="cuda")
    assert merge(cb, 0, oa.data_ptr(), N_A, zero.data_ptr(), 0, L, 15, ad.data_ptr(), None, out.data_ptr(), None, z) == _lib.OK
    assert as_bytes(out[:N_A]) == a.tobytes()


def test_empty_merge_launches_nothing(ra, pq):
    import torch
    for L in (0, 5):
        off = torch.zeros(L + 1, dtype=torch.int64, device="cuda")
        e = torch.zeros((0, 15), dtype=torch.uint8, device="cuda")
        ra.launch_log(reset=True)
        out, off_out = pq.merge_lists_device(off, e, off, e, check=True)
        assert ra.launch_log(reset=True) == ""
        assert tuple(out.shape) == (0, 15) and out.dtype == torch.uint8
        assert off_out.cpu().numpy().tolist() == [0] * (L + 1)
