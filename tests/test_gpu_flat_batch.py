"""GPU tests of the exact searches for query batches (Pq.flat_search_batch_device, Pq.flat_range_batch_device and
`screen=True` on the resident matrices): matrix-core screen, exact resolve.  Every result must equal the plain exhaustive
call's bit for bit -- values, ids and lims -- whatever the screen returned."""
import functools

import numpy as np
import pytest

import flat_search_ref as fr
import synth
from test_gpu_adc_search_lists import ra  # noqa: F401
from test_gpu_rerank import make_data, make_pq

pytestmark = pytest.mark.gpu


def same(got, want):
    """tuples of tensors equal bit for bit (floats compared as their bits)"""
    import torch
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape)
        if g.dtype == torch.float32:
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w)


@functools.lru_cache(maxsize=None)
def world(half):
    """4,100 x 300 rows with duplicates, ties and special values, 70 queries; on the device once"""
    import torch
    q, x = make_data(9100, 4100, 300, 70, half)
    x[17] = x[5]
    x[140] = x[5]
    x[4000:4010] = x[5]                                # ten more copies: ties across the k-th place
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1].astype(x.dtype)
    x[9] = 0
    return torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), x


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
@pytest.mark.parametrize("k", [1, 10, 128, 1024])
def test_gpu_flat_search_batch_equals_the_plain_search(ra, k, ip, half):
    pq = make_pq(ra)
    qd, xd, _ = world(half)
    stats = {}
    got = pq.flat_search_batch_device(qd, xd, k, ip=ip, stats=stats, check=True)
    same(got, pq.flat_search_device(qd, xd, k, ip=ip))
    if k <= 10:                                        # 4,100 rows: a larger k passes the fallback limit of 256 per query
        assert stats["fallback_queries"] == 0 and stats["candidates"] <= 70 * 4100 / 16, stats   # the screen route was taken
        assert stats["x_exp"] > 0                      # from the largest FINITE element
    one = pq.flat_search_batch_device(qd[3], xd, k, ip=ip)
    same(one, pq.flat_search_device(qd[3], xd, k, ip=ip))


@pytest.mark.parametrize("ip", [False, True])
def test_gpu_flat_search_batch_small_matrices_masks_and_fallbacks(ra, ip):
    import torch
    pq = make_pq(ra)
    qd, xd, x = world(False)
    # k > n and n around a tile
    for n in (1, 31, 33, 1023, 1025):
        for k in (1, 40):
            same(pq.flat_search_batch_device(qd[:33], xd[:n], k, ip=ip), pq.flat_search_device(qd[:33], xd[:n], k, ip=ip))
    # a mask, and a mask so thin that the sample holds fewer than k rows: those queries take the plain call
    rng = np.random.default_rng(9101)
    allow = rng.random(4100) < 0.6
    thin = np.zeros(4100, bool)
    thin[[5, 17, 140, 2001]] = True
    for flags, k, fell in ((allow, 10, 0), (thin, 3, 70), (thin, 10, 70)):
        wd = torch.from_numpy(fr.mask_words(flags)).cuda()
        stats = {}
        got = pq.flat_search_batch_device(qd, xd, k, ip=ip, allow=wd, stats=stats)
        same(got, pq.flat_search_device(qd, xd, k, ip=ip, allow=wd))
        assert stats["fallback_queries"] == fell, stats
    # unaligned rows and a caller's x_exp that is far off: still the same result
    big = torch.zeros((4100, 301), device="cuda")
    big[:, :300] = xd
    for x_exp in (0, 14, -30):
        same(pq.flat_search_batch_device(qd, big[:, :300], 10, ip=ip, x_exp=x_exp), pq.flat_search_device(qd, xd, 10, ip=ip))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_gpu_flat_range_batch_equals_the_plain_range(ra, ip, half):
    import torch
    pq = make_pq(ra)
    qd, xd, _ = world(half)
    val, _ = pq.flat_search_device(qd, xd, 64, ip=ip)
    thr = val[:, 63].clone()                           # 64 rows per query and their ties
    thr[5] = float("nan")
    thr[6] = float("inf")
    thr[7] = float("-inf")
    thr[8] = val[8, 0]
    same(pq.flat_range_batch_device(qd, xd, thr, ip=ip, check=True), pq.flat_range_device(qd, xd, thr, ip=ip))
    same(pq.flat_range_batch_device(qd[2], xd, float(thr[2]), ip=ip), pq.flat_range_device(qd[2], xd, float(thr[2]), ip=ip))
    wd = torch.from_numpy(fr.mask_words(np.random.default_rng(9102).random(4100) < 0.5)).cuda()
    same(pq.flat_range_batch_device(qd, xd, thr, ip=ip, allow=wd), pq.flat_range_device(qd, xd, thr, ip=ip, allow=wd))


def test_gpu_screen_route_of_the_resident_matrices(ra):
    """screen=True equals screen=False on FlatMatrix and on a quantized class with attached vectors"""
    import torch
    from reductive_amd import qmatrix
    rng = np.random.default_rng(9103)
    n, d = 2200, 24
    x = synth.normalish(9104, (n, d)).astype(np.float32)
    x[1500] = x[7]
    q = torch.from_numpy((x[rng.choice(n, 40, replace=False)] * np.float32(1.01)).astype(np.float32)).cuda()
    flags = rng.random(n) < 0.4
    fm = ra.FlatMatrix(x)
    fh = ra.FlatMatrix(x.astype(np.float16))
    pq = ra.train_pq(4, 4, 2, 1, x, rng=np.random.default_rng(9105))
    codes = pq.quantize_batch_device(torch.from_numpy(x).cuda())
    qm = qmatrix.QuantizedMatrix(pq, codes.cpu().numpy()).attach_vectors(x)
    r_l2 = float(fm.nearest(q, 30)[0][:, -1].median())
    r_ip = float(fm.most_similar(q, 30)[0][:, -1].median())
    for m in (fm, fh):
        for allow in (None, flags):
            same(m.nearest(q, 10, allow=allow, screen=True), m.nearest(q, 10, allow=allow))
            same(m.most_similar(q, 10, allow=allow, screen=True), m.most_similar(q, 10, allow=allow))
            same(m.within(q, r_l2, allow=allow, screen=True), m.within(q, r_l2, allow=allow))
            same(m.similar_above(q, r_ip, allow=allow, sort=True, screen=True), m.similar_above(q, r_ip, allow=allow, sort=True))
    for allow in (None, flags):
        same(qm.exact_nearest(q, 10, allow=allow, screen=True), qm.exact_nearest(q, 10, allow=allow))
        same(qm.exact_most_similar(q, 10, allow=allow, screen=True), qm.exact_most_similar(q, 10, allow=allow))
        same(qm.exact_within(q, r_l2, allow=allow, screen=True), qm.exact_within(q, r_l2, allow=allow))
        same(qm.exact_similar_above(q, r_ip, allow=allow, screen=True), qm.exact_similar_above(q, r_ip, allow=allow))
    same(qm.exact_nearest(q, 10, screen=True), fm.nearest(q, 10))
