"""GPU tests of the one-hot screen over 4-bit packed codes (include/pqhip.h: pqhip_adc_screen_packed4_f32_dev) through
Pq.adc_screen_device(packed4=True), and of the batch search built on it (Pq.adc_search_batch_device(packed4=True),
screen="onehot" on a packed QuantizedMatrix).  The screen equals the u8 screen on the unpacked codes bit for bit -- and so
holds that screen's contract against the f32-chain reference and the device's range calls -- for every grid, grouping and
capacity; the batch search equals the plain packed search bit for bit."""
import numpy as np
import pytest

import adc_screen_ref as asr
import synth
from test_gpu_adc_range import dev_words, make_pq, ra  # noqa: F401
from test_gpu_adc_screen import N, check_screen, world
from test_gpu_flat_batch import same

pytestmark = pytest.mark.gpu
FORMS = [(False, False), (True, False), (True, True)]
SHAPES = [(1, 16, 1), (7, 16, 33), (16, 16, 73), (48, 16, 33), (15, 9, 5)]   # 73: a pass of 64 and a ragged one of 32 slots


def packed_rows(pq, cd):
    """the packed rows of the u8 codes `cd`, ceil(M / 2) + 1 bytes apart"""
    import torch
    PB = (cd.shape[1] + 1) // 2
    buf = torch.zeros((cd.shape[0], PB + 1), dtype=torch.uint8, device="cuda")
    pq.pack_codes4_device(cd, out=buf[:, :PB], check=True)
    return buf[:, :PB]


@pytest.mark.parametrize("ip,scaled", FORMS)
@pytest.mark.parametrize("M,K,nq", SHAPES)
def test_gpu_packed_screen_equals_the_u8_screen(ra, M, K, nq, ip, scaled):
    import torch
    pq, w = make_pq(ra, M, K), world(M, K, nq, ip)
    pk, thr = packed_rows(pq, w["cd"]), w["thr"]
    kw = dict(ip=ip, scales=w["sd"] if scaled else None, allow=w["wd"])
    want = pq.adc_screen_device(w["cd"], w["td"], thr, check=True, **kw)
    results = []
    try:
        for wgs in (1, 3):
            ra.set_option("adc_screen_wgs", wgs)
            results.append(pq.adc_screen_device(pk, w["td"], thr, check=True, packed4=True, **kw))
    finally:
        ra.set_option("adc_screen_wgs", 0)
    for got in results:                                                   # the u8 screen, whatever the grid
        same(got, want)
    check_screen(pq, w, ip, scaled, thr, results[0])
    lims, idx = want
    if nq > 1:                                                            # the grouping into passes and calls
        h = nq // 2
        a, b = (pq.adc_screen_device(pk, w["td"][s], thr[s], packed4=True, **kw) for s in (slice(0, h), slice(h, nq)))
        same((torch.cat([a[0], b[0][1:] + a[0][-1]]), torch.cat([a[1], b[1]])), (lims, idx))
    total = int(lims[-1])
    for cap in (0, total // 2):                                           # counts always, a valid prefix when short
        l2, i2, t2, _ = pq._adc_screen(pk, w["td"], thr, ip, kw["scales"], w["wd"], cap, None, False, "pqhip_adc_screen_packed4_f32_dev", True)
        assert t2 == total and torch.equal(l2, lims) and torch.equal(i2, idx[:cap])


def test_gpu_packed_screen_nibbles_past_K_and_the_pad_nibble(ra):
    M, K, nq = 15, 9, 5
    pq, w = make_pq(ra, M, K), world(M, K, nq, False)
    pk = packed_rows(pq, w["cd"])
    want = pq.adc_screen_device(pk, w["td"], w["thr"], allow=w["wd"], check=True, packed4=True)
    pad = pk.clone()
    pad[:, -1] |= 0xF0                                                    # the pad nibble of every row: nobody's code
    same(pq.adc_screen_device(pad, w["td"], w["thr"], allow=w["wd"], check=True, packed4=True), want)
    bad, row = pk.clone(), int(np.flatnonzero(w["allow"])[-1])
    bad[row, 1] = (bad[row, 1] & 0x0F) | (K << 4)                         # code 3 of an allowed row
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.adc_screen_device(bad, w["td"], w["thr"], allow=w["wd"], check=True, packed4=True)
    bad, row = pk.clone(), int(np.flatnonzero(~w["allow"])[-1])
    bad[row, 1] = (bad[row, 1] & 0x0F) | (K << 4)                         # a disallowed row is not loaded
    same(pq.adc_screen_device(bad, w["td"], w["thr"], allow=w["wd"], check=True, packed4=True), want)


@pytest.mark.parametrize("ip,scaled", FORMS)
def test_gpu_packed_batch_search_equals_the_plain_packed_search(ra, ip, scaled):
    from reductive_amd import pq as rules
    M, K, nq = 16, 16, 40
    pq, w = make_pq(ra, M, K), world(M, K, nq, ip)
    pk = packed_rows(pq, w["cd"])
    kw = {"scales": w["sd"] if scaled else None} if ip else {}
    plain = pq.adc_ip_search_device if ip else pq.adc_search_device
    thin = np.zeros(N, bool)
    thin[[5, 17, 140, 2001]] = True
    for k, wd, fell in ((1, None, None), (1, w["wd"], 0), (100, None, None), (1024, w["wd"], None), (3, dev_words(thin), nq)):
        stats = {}
        got = pq.adc_search_batch_device(pk, w["td"], k, ip=ip, allow=wd, stats=stats, check=True, packed4=True, **kw)
        same(got, plain(pk, w["td"], k, allow=wd, packed4=True, **kw))
        assert fell is None or stats["fallback_queries"] == fell, stats
    # the input meant for the screen route stays under the fallback share on the CPU model as well
    _, _, took_plain, _ = asr.ref_adc_search_batch(w["t"][:8], w["codes"], 1, rules.flat_batch_sample, rules.flat_batch_falls_back, ip,
                                                   w["scales"] if scaled else None)
    assert not took_plain.any()


def test_gpu_onehot_route_of_the_packed_matrix(ra):
    import torch
    from reductive_amd import qmatrix
    M, K = 16, 16
    pq, w = make_pq(ra, M, K), world(M, K, 40, False)
    x = synth.normalish(73, (N, 4 * M))
    qm = qmatrix.QuantizedMatrix(pq, w["codes"].astype(np.uint8), norms=w["scales"]).attach_vectors(x).pack4()
    q = torch.from_numpy(x[:40] * np.float32(1.01)).cuda()
    for allow in (None, w["allow"]):
        same(qm.nearest(q, 1, allow=allow, screen="onehot"), qm.nearest(q, 1, allow=allow))
        for use_norms in (True, False):
            same(qm.most_similar(q, 2, use_norms=use_norms, allow=allow, screen="onehot"),
                 qm.most_similar(q, 2, use_norms=use_norms, allow=allow))
        same(qm.nearest(q, 3, refine=20, allow=allow, screen="onehot"), qm.nearest(q, 3, refine=20, allow=allow))
        same(qm.most_similar(q, 3, refine=20, allow=allow, screen="onehot"), qm.most_similar(q, 3, refine=20, allow=allow))
