"""The merge of search results on the GPU (include/pqhip.h: pqhip_topk_merge_f32_dev, Pq.merge_topk_device).  Reference:
tests/results_merge_ref.py (pinned against brute force by test_results_merge.py).  Every comparison is bit for bit.
Values come from SPECIAL_VALUES (multiples of 0.25 in [-2, 2], -0, +-Inf, NaN), so ties and special values are the rule.
Covered: 1 .. 17 parts (across the eight merge waves); (k_in, k) over a lane-count boundary, k > P k_in and k < k_in; 1, 3
and 67 queries; both metrics; parts with different fill counts, all-padding parts and rows among them; a NaN entry next
to padding; offsets present and absent; the parts output; strided views with garbage in the gaps; output rows wider than
k; forced grids; no query at all; the statuses in their precedence."""
import ctypes

import numpy as np
import pytest

import synth
from results_merge_ref import QNAN, SPECIAL_VALUES, bits, order_key, ref_merge

pytestmark = pytest.mark.gpu

PARTS = (1, 2, 3, 8, 9, 17)
WIDTHS = ((1, 1), (5, 3), (64, 64), (65, 65), (100, 100), (1024, 1024), (7, 100), (1024, 1))
QUERIES = (1, 3, 67)


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
    return ra.Pq(None, synth.normalish(4100, (2, 16, 4)))


def results(rng, P, nq, k_in, largest):
    """P sorted result rows per query with random fill counts (some parts all padding, some full), garbage values and
    index -1 in the padding, ids that repeat across parts"""
    val = rng.choice(SPECIAL_VALUES, (P, nq, k_in)).astype(np.float32)
    key = order_key(-val if largest else val).reshape(val.shape)
    val = np.take_along_axis(val, np.argsort(key, axis=2, kind="stable"), axis=2)
    count = rng.integers(0, k_in + 1, (P, nq))
    count[rng.random((P, nq)) < 0.2] = k_in
    count[rng.random((P, nq)) < 0.15] = 0
    if P > 1:
        count[rng.integers(P)] = 0                                  # one part returns nothing for any query
    idx = rng.integers(0, 1000, (P, nq, k_in)).astype(np.int64)
    absent = np.arange(k_in)[None, None, :] >= count[:, :, None]
    idx[absent] = -1
    val[absent] = rng.choice(SPECIAL_VALUES, int(absent.sum())).astype(np.float32)
    return val, idx


def assert_merge(got, want, parts=True):
    assert got[0].dtype.is_floating_point and tuple(got[0].shape) == want[0].shape
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0]))
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    if parts:
        assert np.array_equal(got[2].cpu().numpy(), want[2])


@pytest.mark.parametrize("k_in,k", WIDTHS)
@pytest.mark.parametrize("P", PARTS)
def test_merge_is_the_reference(pq, P, k_in, k):
    import torch
    rng = np.random.default_rng(P * 10000 + k_in * 7 + k)
    offsets = np.cumsum(rng.integers(0, 5000, P)).astype(np.int64) * 1000
    off_d = torch.from_numpy(offsets).cuda()
    for nq in QUERIES:
        for largest in (False, True):
            val, idx = results(rng, P, nq, k_in, largest)
            vd, xd = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
            got = pq.merge_topk_device(vd, xd, k, largest=largest, offsets=off_d, want_parts=True)
            assert got[2].dtype == torch.int32 and got[1].dtype == torch.int64
            want = ref_merge(val, idx, k, largest, offsets)
            assert_merge(got, want)
            got = pq.merge_topk_device(vd, xd, k, largest=largest)
            assert len(got) == 2
            plain = np.where(want[1] < 0, -1, want[1] - offsets[np.maximum(want[2], 0)])     # (the reference adds them last)
            assert_merge(got, (want[0], plain), parts=False)


def test_nan_entry_next_to_padding_and_ties_by_part(pq):
    import torch
    inf = np.float32(np.inf)
    val = np.array([[[1.0, np.nan, 0.0, -inf]], [[-0.0, 1.0, np.nan, np.nan]], [[inf, inf, inf, inf]], [[1.0, inf, np.nan, 5.0]]], np.float32)
    idx = np.array([[[7, 8, -1, -1]], [[9, 7, 6, 5]], [[-1, -1, -1, -1]], [[3, 2, 1, -1]]], np.int64)
    want = ref_merge(val, idx, 12)
    assert want[1][0].tolist() == [9, 7, 7, 3, 2, 8, 6, 5, 1, -1, -1, -1]
    assert want[2][0].tolist() == [1, 0, 1, 3, 3, 0, 1, 1, 3, -1, -1, -1]
    assert bits(want[0][0]).tolist() == bits(np.array([0, 1, 1, 1, inf, QNAN, QNAN, QNAN, QNAN, inf, inf, inf], np.float32)).tolist()
    vd, xd = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
    for k in (1, 5, 6, 9, 12, 200):
        assert_merge(pq.merge_topk_device(vd, xd, k, want_parts=True), ref_merge(val, idx, k))
    # scores: every NaN is still last, padding is -Inf
    val = -val
    got = pq.merge_topk_device(torch.from_numpy(val).cuda(), xd, 12, largest=True, want_parts=True)
    want = ref_merge(val, idx, 12, True)
    assert want[1][0].tolist() == [9, 7, 7, 3, 2, 8, 6, 5, 1, -1, -1, -1] and np.all(want[0][0, 9:] == -inf)
    assert_merge(got, want)


@pytest.mark.parametrize("P,k_in,k", [(3, 5, 4), (9, 100, 100), (2, 1024, 1000)])
def test_strided_views_are_respected_and_gaps_are_not_read(pq, P, k_in, k):
    import torch
    rng = np.random.default_rng(P + k)
    nq = 5
    for largest in (False, True):
        val, idx = results(rng, P, nq, k_in, largest)
        want = ref_merge(val, idx, k, largest)
        # gaps hold what would win every comparison: present ids with the best value there is
        big_v = torch.full((2 * P + 1, nq + 3, k_in + 9), float("inf") if largest else float("-inf"), dtype=torch.float32, device="cuda")
        big_i = torch.full((2 * P, nq + 2, k_in + 4), 424242, dtype=torch.int64, device="cuda")
        vv = big_v[1::2, 2:2 + nq, 6:6 + k_in]
        iv = big_i[0::2, 1:1 + nq, 3:3 + k_in]
        vv.copy_(torch.from_numpy(val))
        iv.copy_(torch.from_numpy(idx))
        assert not vv.is_contiguous() and not iv.is_contiguous() and vv.stride(2) == 1
        assert_merge(pq.merge_topk_device(vv, iv, k, largest=largest, want_parts=True), want)
        # a column stride other than one goes through a copy
        wide = torch.zeros((P, nq, 2 * k_in), dtype=torch.float32, device="cuda")
        wide[:, :, ::2] = torch.from_numpy(val).cuda()
        assert_merge(pq.merge_topk_device(wide[:, :, ::2], iv, k, largest=largest, want_parts=True), want)


def raw_call(ra, pq, vd, xd, off, largest, k, ov, oi, op, slot=0, k_in=None, v_rs=None):
    import torch
    P, nq, kk = vd.shape
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return ra.lib().pqhip_topk_merge_f32_dev(
        pq._cb(), slot, ptr(vd), vd.stride(0), vd.stride(1) if v_rs is None else v_rs, ptr(xd), xd.stride(0), xd.stride(1), P, nq,
        kk if k_in is None else k_in, ptr(off), largest, k, ptr(ov), 0 if ov is None else ov.stride(0), ptr(oi),
        0 if oi is None else oi.stride(0), ptr(op), 0 if op is None else op.stride(0),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_output_rows_wider_than_k_keep_their_tail(ra, pq):
    import torch
    rng = np.random.default_rng(77)
    P, nq, k_in, k = 5, 9, 70, 66
    val, idx = results(rng, P, nq, k_in, False)
    vd, xd = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
    ov = torch.full((nq, k + 3), 123.5, dtype=torch.float32, device="cuda")
    oi = torch.full((nq, k + 5), -77, dtype=torch.int64, device="cuda")
    op = torch.full((nq, k + 1), -55, dtype=torch.int32, device="cuda")
    assert raw_call(ra, pq, vd, xd, None, 0, k, ov, oi, op) == 0
    torch.cuda.synchronize()
    want = ref_merge(val, idx, k)
    assert_merge((ov[:, :k], oi[:, :k], op[:, :k]), want)
    assert bool((ov[:, k:] == 123.5).all()) and bool((oi[:, k:] == -77).all()) and bool((op[:, k:] == -55).all())


def test_result_does_not_depend_on_the_grid(ra, pq):
    import torch
    rng = np.random.default_rng(78)
    P, nq, k_in, k = 9, 67, 130, 129
    val, idx = results(rng, P, nq, k_in, True)
    vd, xd = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
    want = ref_merge(val, idx, k, True)
    try:
        for wgs in (1, 2, 5, 66, 1 << 30):
            ra.set_option("topk_merge_wgs", wgs)
            assert_merge(pq.merge_topk_device(vd, xd, k, largest=True, want_parts=True), want)
    finally:
        ra.set_option("topk_merge_wgs", 0)


def test_no_query_and_statuses_in_their_precedence(ra, pq):
    import torch
    from reductive_amd import _lib
    val, idx, part = pq.merge_topk_device(torch.empty((3, 0, 5), device="cuda"), torch.empty((3, 0, 5), dtype=torch.int64, device="cuda"),
                                          4, want_parts=True)
    assert tuple(val.shape) == tuple(idx.shape) == tuple(part.shape) == (0, 4)
    vd = torch.zeros((2, 3, 8), dtype=torch.float32, device="cuda")
    xd = torch.zeros((2, 3, 8), dtype=torch.int64, device="cuda")
    ov = torch.zeros((3, 8), dtype=torch.float32, device="cuda")
    oi = torch.zeros((3, 8), dtype=torch.int64, device="cuda")
    op = torch.zeros((3, 8), dtype=torch.int32, device="cuda")
    assert raw_call(ra, pq, vd, xd, None, 0, 8, ov, oi, op) == _lib.OK
    assert raw_call(ra, pq, vd, xd, None, 2, 8, ov, oi, op, slot=99) == _lib.EINVAL          # EINVAL before the slot
    assert raw_call(ra, pq, vd, xd, None, 0, 0, ov, oi, op) == _lib.EINVAL
    assert raw_call(ra, pq, vd, xd, None, 0, 1025, ov, oi, op, slot=99) == _lib.ENODEV       # the slot before the limits
    assert raw_call(ra, pq, vd, xd, None, 0, 1025, None, oi, op) == _lib.EUNSUPPORTED        # the limits before the pointers
    assert raw_call(ra, pq, vd, xd, None, 0, 8, ov, oi, op, k_in=1025) == _lib.EUNSUPPORTED
    assert raw_call(ra, pq, vd, xd, None, 0, 8, None, oi, op, v_rs=4) == _lib.EINVAL         # the pointers before the strides
    assert raw_call(ra, pq, vd, xd, None, 0, 8, ov, None, op) == _lib.EINVAL
    assert raw_call(ra, pq, vd, xd, None, 0, 8, ov, oi, op, v_rs=7) == _lib.ESHAPE
    assert raw_call(ra, pq, vd, xd, None, 0, 9, ov, oi, None) == _lib.ESHAPE                 # output rows narrower than k
    assert raw_call(ra, pq, vd, xd, None, 0, 8, ov, oi, op[:, :4].contiguous()) == _lib.ESHAPE
    # no query: nothing is launched and no pointer is looked at
    empty = torch.empty((2, 0, 8), dtype=torch.float32, device="cuda")
    assert raw_call(ra, pq, empty, empty.long(), None, 1, 8, None, None, None) == _lib.OK
    torch.cuda.synchronize()
