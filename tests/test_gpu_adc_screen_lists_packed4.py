"""GPU tests of the one-hot screen over 4-bit packed codes in probed lists (include/pqhip.h:
pqhip_adc_screen_lists_packed4_f32_dev) through Pq.adc_screen_lists_device(packed4=True), and of the batch list search built
on it (Pq.adc_search_lists_batch_device(packed4=True), screen="onehot" on a packed PartitionedMatrix).  The screen equals
the u8 list screen on the unpacked codes bit for bit and holds every row of the exact f64 range answer, for every grid,
unit size, chunk, split and capacity; the batch search equals the plain packed list search bit for bit."""
import functools

import numpy as np
import pytest

import synth
from adc_lists_ref import probed_positions
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
LENS = [0, 1, 31, 33, 1000, 700, 235]          # empty, one row, both sides of a tile, a long list, tiles at every bit offset of the mask
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N, LONG = int(OFF[-1]), 4
FORMS = [(False, False), (True, False), (True, True)]
# a pad nibble, K < 16, PB no multiple of 4; PB 17 and 24: the instantiation of 8 row dwords; M > 64: one block of 32 slots
SHAPES = [(1, 16), (7, 11), (8, 16), (17, 16), (33, 16), (48, 16), (66, 3)]
EACH_KERNEL = [(7, 11), (48, 16), (66, 3)]             # the three instantiations of the count pass: <4, 2>, <8, 2>, <13, 1>
OPTIONS = ("adc_screen_lists_wgs", "adc_screen_lists_unit_rows", "adc_screen_lists_chunk_queries")


def skewed(rng, n, M, K, nq, ip):
    """codes [n, M] u8 that favour the first centroids, and tables [nq, M, K] whose entries there are small"""
    codes = np.where(rng.random((n, M)) < 0.5, rng.integers(0, min(K, 4), (n, M)), rng.integers(0, K, (n, M))).astype(np.uint8)
    t = (rng.random((nq, M, K)) + 0.5).astype(np.float32)
    t[:, :, : min(K, 4)] *= np.float32(0.1)
    return codes, (-t if ip else t), t.astype(np.float64)[:, np.arange(M), codes.astype(np.int64)].sum(axis=2) * (-1 if ip else 1)


def packed_rows(pq, cd):
    """the packed rows of the u8 codes `cd` at an odd byte stride"""
    import torch
    PB = (cd.shape[1] + 1) // 2
    buf = torch.zeros((cd.shape[0], PB + 1 + PB % 2), dtype=torch.uint8, device="cuda")
    pq.pack_codes4_device(cd, out=buf[:, :PB], check=True)
    return buf[:, :PB]


@functools.lru_cache(maxsize=None)
def world(ra, M, K, ip, nq=70, n_probe=3):
    """skewed codes, tables with a few small entries, every query probing the long list (so its second group of 64 is
    padded) and n_probe - 1 others in a rotated order, one -1 pad, thresholds at the 21st best allowed probed row, scales
    and a mask; in the packed rows every nibble of an unprobed or disallowed row is 15"""
    import torch
    rng = np.random.default_rng(9300 + M)
    codes, t, v64 = skewed(rng, N, M, K, nq, ip)                          # v64 [nq, N]: the exact values
    scales = (rng.random(N) + 0.5).astype(np.float32)
    allow = rng.random(N) < 0.7
    others = [l for l in range(len(LENS)) if l != LONG]
    probes = np.stack([np.roll(np.concatenate([[LONG], rng.permutation(others)[: n_probe - 1]]), q % n_probe) for q in range(nq)])
    probes[3, -1] = -1                                                    # query 3 has the long list in slot 0
    thr, probed = np.zeros(nq, np.float32), np.zeros(N, bool)
    for q in range(nq):
        pos = probed_positions(OFF, probes[q], N)
        probed[pos] = True
        thr[q] = np.sort(v64[q, pos[allow[pos]]])[-21 if ip else 20]
    pq = make_pq(ra, M, K)
    cd = torch.from_numpy(codes).cuda()
    pk = packed_rows(pq, cd)
    pk[torch.from_numpy(~(probed & allow)).cuda()] = 0xFF                  # K < 16: reading one of them raises the range flag
    return dict(pq=pq, t=t, v64=v64, scales=scales, allow=allow, thr=thr, probes=probes, cd=cd, pk=pk, td=torch.from_numpy(t).cuda(),
                sd=torch.from_numpy(scales).cuda(), wd=dev_words(allow), od=torch.from_numpy(OFF).cuda(), pd=torch.from_numpy(probes).cuda())


def screen(w, codes, ip, scaled, s=slice(None), packed4=True, **kw):
    return w["pq"].adc_screen_lists_device(codes, w["td"][s], w["od"], w["pd"][s], w["thr"][s], ip=ip,
                                           scales=w["sd"] if scaled else None, allow=w["wd"], packed4=packed4, **kw)


@pytest.mark.parametrize("ip,scaled", FORMS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_gpu_packed_list_screen_equals_the_u8_list_screen_and_holds_the_exact_answer(ra, M, K, ip, scaled):
    import torch
    w = world(ra, M, K, ip)
    lims, idx = got = screen(w, w["pk"], ip, scaled, check=True)          # check=True: no poisoned row was read
    same(got, screen(w, w["cd"], ip, scaled, packed4=False))
    lh, ih = lims.cpu().numpy(), idx.cpu().numpy()
    for q in range(w["thr"].size):
        pos = probed_positions(OFF, w["probes"][q], N)
        S = pos[w["allow"][pos]]
        v = w["v64"][q, S] * (w["scales"].astype(np.float64)[S] if scaled else 1.0)
        want = S[(v >= w["thr"][q]) if ip else (v <= w["thr"][q])]
        assert want.size > 0 and np.isin(want, ih[lh[q]:lh[q + 1]]).all(), q
    total = int(lims[-1])
    for cap in (0, total // 2):                                           # counts always, a valid prefix when short
        l2, i2, t2, _ = w["pq"]._adc_screen_lists(w["pk"], w["td"], w["od"], w["pd"], w["thr"], ip, w["sd"] if scaled else None, w["wd"],
                                                  cap, None, False, True)
        assert t2 == total and torch.equal(l2, lims) and torch.equal(i2, idx[:cap])


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, True)])
@pytest.mark.parametrize("M,K", EACH_KERNEL)
def test_gpu_packed_list_screen_one_result_for_every_grid_unit_chunk_and_split(ra, M, K, ip, scaled):
    import torch
    w = world(ra, M, K, ip)
    want = screen(w, w["pk"], ip, scaled)
    try:
        for values in ((1, 64, 1), (3, 64, 7), (1, 0, 0), (3, 0, 7)):     # one workgroup keeps the image from unit to unit
            for name, v in zip(OPTIONS, values):
                ra.set_option(name, v)
            same(screen(w, w["pk"], ip, scaled), want)
    finally:
        for name in OPTIONS:
            ra.set_option(name, 0)
    a, b = screen(w, w["pk"], ip, scaled, slice(0, 40)), screen(w, w["pk"], ip, scaled, slice(40, 70))
    same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), want)


@pytest.mark.parametrize("ip,scaled", [(False, False), (True, True)])
@pytest.mark.parametrize("M", [15, 48])                                   # the packed fill walk behind <4, 2> and <8, 2>
def test_gpu_packed_list_screen_pairs_beyond_the_hit_word_budget(ra, M, ip, scaled):
    """one list of 4,000 of 4,099 rows, probed by every query: 8 budgeted words per query against a pair's 125, so the
    fill pass forms most pairs again from the packed rows -- the u8 list screen's result on the unpacked codes"""
    import torch
    K, nq, n = 16, 33, 4099
    pq, rng = make_pq(ra, M, K), np.random.default_rng(5)
    codes, t, v = skewed(rng, n, M, K, nq, ip)
    sc = (rng.random(n) + 0.5).astype(np.float32)
    v = v * (sc if scaled else 1.0)
    thr = np.sort(v[:, :4000], axis=1)[:, -60 if ip else 60].astype(np.float32)
    off = torch.from_numpy(np.concatenate([[0, 4000], 4000 + np.cumsum([2] * 36 + [1] * 27)]).astype(np.int64)).cuda()
    cd, td, pr = torch.from_numpy(codes).cuda(), torch.from_numpy(t).cuda(), torch.zeros((nq, 1), dtype=torch.int64, device="cuda")
    kw = dict(ip=ip, scales=torch.from_numpy(sc).cuda() if scaled else None, allow=dev_words(rng.random(n) < 0.7))
    got = pq.adc_screen_lists_device(packed_rows(pq, cd), td, off, pr, thr, check=True, packed4=True, **kw)
    same(got, pq.adc_screen_lists_device(cd, td, off, pr, thr, **kw))
    assert int(got[0][-1]) >= 20 * nq


def test_gpu_packed_list_screen_nibbles_past_K_and_the_pad_nibble(ra):
    """the poisoned rows of world() are the disallowed and the unprobed ones: check=True shows that none raises the flag"""
    M, K = 7, 11
    w = world(ra, M, K, False)
    want = screen(w, w["pk"], False, False, check=True)
    live = int(np.flatnonzero(w["allow"][: OFF[LONG + 1]])[-1])           # an allowed row of the long list, which every query probes
    pad = w["pk"].clone()
    pad[live, -1] |= 0xF0                                                 # the pad nibble: nobody's code
    same(screen(w, pad, False, False, check=True), want)
    bad = w["pk"].clone()
    bad[live, 1] = (bad[live, 1] & 0x0F) | (K << 4)                       # code 3 of that row
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        screen(w, bad, False, False, check=True)
    lims, idx = (a.cpu().numpy() for a in screen(w, bad, False, False))
    least = w["t"][:, 3].argmin(axis=1)                                   # an image entry of 0 is that of the subquantizer's least entry
    for c in np.unique(least):
        as0 = bad.clone()
        as0[live, 1] = (as0[live, 1] & 0x0F) | (int(c) << 4)
        l0, i0 = (a.cpu().numpy() for a in screen(w, as0, False, False))
        for q in np.flatnonzero(least == c):
            assert np.array_equal(idx[lims[q]:lims[q + 1]], i0[l0[q]:l0[q + 1]]), q


@functools.lru_cache(maxsize=None)
def batch_world(ra, ip):
    """6,000 rows in 24 lists of 250 that differ in how good their rows are; integer-valued tables (many ties); four rows
    of lists 1 and 10 each are the same best row of every query, the two lists probed in either slot order; one doubled
    probe"""
    import torch
    rng = np.random.default_rng(41)
    M, K, n, nq = 16, 16, 6000, 40
    t = rng.integers(4, 40, (nq, M, K)).astype(np.float32)
    t[:, :, 1:3] = rng.integers(1, 3, (nq, M, 2)).astype(np.float32)
    t[:, :, 0] = 0
    codes = rng.integers(1, K, (n, M)).astype(np.uint8)
    near = rng.random((n, M)) < np.repeat(np.linspace(0.9, 0.1, 24), 250)[:, None]
    codes[near] = rng.integers(1, 3, int(near.sum())).astype(np.uint8)
    codes[300:304], codes[2600:2604] = 0, 0                               # value 0 in lists 1 and 10: ties across probe slots
    probes = np.zeros((nq, 12), np.int64)
    for q in range(nq):
        rest = rng.permutation(np.setdiff1d(np.arange(24), [q % 3, 1, 10]))[:11]
        pair = [10] if q % 3 == 1 else ([1, 10] if q % 2 else [10, 1])
        probes[q] = np.concatenate([[q % 3], pair, rest])[:12]
    probes[5, 7] = probes[5, 3]                                           # a doubled probe: the query falls back
    pq = make_pq(ra, M, K)
    cd = torch.from_numpy(codes).cuda()
    return dict(pq=pq, pk=packed_rows(pq, cd), td=torch.from_numpy(-t if ip else t).cuda(),
                sd=torch.from_numpy((rng.integers(1, 3, n)).astype(np.float32)).cuda(), wd=dev_words(rng.random(n) < 0.8),
                od=torch.arange(0, n + 1, 250, device="cuda"), pd=torch.from_numpy(probes).cuda())


@pytest.mark.parametrize("k,masked", [(1, False), (10, True), (10, False)])
@pytest.mark.parametrize("ip,scaled", FORMS)
def test_gpu_packed_list_batch_search_equals_the_plain_packed_list_search(ra, ip, scaled, k, masked):
    w = batch_world(ra, ip)
    pq = w["pq"]
    kw = {"scales": w["sd"] if scaled else None} if ip else {}
    plain = pq.adc_ip_search_lists_device if ip else pq.adc_search_lists_device
    wd, stats = (w["wd"] if masked else None), {}
    got = pq.adc_search_lists_batch_device(w["pk"], w["td"], w["od"], w["pd"], k, ip=ip, allow=wd, stats=stats, check=True, packed4=True, **kw)
    same(got, plain(w["pk"], w["td"], w["od"], w["pd"], k, allow=wd, packed4=True, **kw))
    assert stats["fallback_queries"] == 1 and stats["candidates"] > 0, stats   # the doubled probe alone


def test_gpu_onehot_route_of_the_packed_partitioned_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    M, K, n = 16, 16, 6000
    pq, rng = make_pq(ra, M, K), np.random.default_rng(9)
    x = synth.normalish(73, (n, 4 * M))
    qm = qmatrix.QuantizedMatrix(pq, rng.integers(0, K, (n, M)).astype(np.uint8), norms=(rng.random(n) + 0.5).astype(np.float32))
    pm = qmatrix.PartitionedMatrix(qm.attach_vectors(x), x[:12].copy(), rng.integers(0, 12, n))
    pm.vectors = qm.vectors                                               # as QuantizedMatrix.partition hands them on
    pm = pm.pack4()
    q = torch.from_numpy(x[:40] * np.float32(1.01)).cuda()
    for a in (None, rng.random(n) < 0.7):
        same(pm.nearest(q, 2, 5, allow=a, screen="onehot"), pm.nearest(q, 2, 5, allow=a))
        for use_norms in (True, False):
            same(pm.most_similar(q, 2, 5, use_norms=use_norms, allow=a, screen="onehot"), pm.most_similar(q, 2, 5, use_norms=use_norms, allow=a))
        same(pm.nearest(q, 3, 5, refine=20, allow=a, screen="onehot"), pm.nearest(q, 3, 5, refine=20, allow=a))
        same(pm.most_similar(q, 3, 5, refine=20, allow=a, screen="onehot"), pm.most_similar(q, 3, 5, refine=20, allow=a))
