"""The list range searches at every width of the row fetch (include/pqhip.h: pqhip_adc_*range_lists*_f32_dev).
test_gpu_adc_range.py runs its list cases at M = 15, four code dwords per row; here one case per wider bucket of
lists_nv_bucket -- 8, 13 and 25 dwords -- for the four policies, against tests/adc_range_ref.py as there, with the row
sums from the oracle's scan."""
import numpy as np
import pytest

import synth
from adc_range_ref import ref_range_lists, ref_range_residual
from test_gpu_adc_range import check_codes, dev_words, draw_tables, lists_setup, make_pq, ra, same, scaled  # noqa: F401 (ra: fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(30, 32), (48, 16), (100, 8)])
def test_gpu_range_lists_code_widths(ra, M, K):
    """the list range kernels at 8, 13 and 25 code dwords per row (test_gpu_range_lists runs M = 15: 4 dwords), the four
    policies, unmasked and masked, for one and two workgroups per query; the row sums come from the oracle's scan"""
    import torch
    from oracle import pq_oracle as orc
    from reductive_amd import _lib
    nq, n, n_lists, n_probe = 5, 4000, 16, 3
    pq = make_pq(ra, M, K)
    t = draw_tables(8890 + M, nq, M, K)
    codes = synth.codes_u8(8891 + M, (n, M), K)
    cd = torch.from_numpy(codes).cuda()
    off = lists_setup(8892, n, n_lists)
    rng = np.random.default_rng(8893 + M)
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    pr[0, 0] = 11                                              # the long list
    bias = rng.standard_normal(pr.shape).astype(np.float32)
    terms = rng.standard_normal(n).astype(np.float32)
    sc = (synth.uniform01(8894, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    allow = rng.random(n) < 0.5
    s = orc.adc_scan(t.cpu().numpy(), codes)
    od, pd, bd = torch.from_numpy(off).cuda(), torch.from_numpy(pr).cuda(), torch.from_numpy(bias).cuda()
    td, scd, wd = torch.from_numpy(terms).cuda(), torch.from_numpy(sc).cuda(), dev_words(allow)
    inf = np.full(nq, np.inf, np.float32)
    cases = [("l2", False, lambda thr, w: pq.adc_range_lists_device(cd, t, od, pd, thr, allow=w),
              lambda thr, al: ref_range_lists(s, off, pr, thr, allow=al)),
             ("ip", True, lambda thr, w: pq.adc_ip_range_lists_device(cd, t, od, pd, thr, scales=scd, allow=w),
              lambda thr, al: ref_range_lists(scaled(s, sc), off, pr, thr, ip=True, allow=al)),
             ("residual l2", False, lambda thr, w: pq.adc_range_lists_residual_device(cd, t, od, pd, bd, td, thr, allow=w),
              lambda thr, al: ref_range_residual(s, off, pr, bias, thr, terms=terms, allow=al)),
             ("residual ip", True, lambda thr, w: pq.adc_ip_range_lists_residual_device(cd, t, od, pd, bd, thr, scales=scd, allow=w),
              lambda thr, al: ref_range_residual(s, off, pr, bias, thr, scales=sc, ip=True, allow=al))]
    ra.launch_log(reset=True)
    assert check_codes(pq) == _lib.OK
    try:
        for G in (1, 2):
            ra.set_option("adc_range_wgs_per_query", G)
            for name, ip, run, ref in cases:
                wl, wv, wi = ref(-inf if ip else inf, None)    # every probed row: a threshold on a row's own value
                thr = np.array([wv[wl[q] + rng.integers(wl[q + 1] - wl[q])] for q in range(nq)], np.float32)
                assert np.isfinite(thr).all()
                for al, w in ((None, None), (allow, wd)):
                    want = ref(thr, al)
                    assert 0 < want[0][-1] < wl[-1]
                    same(run(thr, w), want, "%s, M %d, G %d, masked %s" % (name, M, G, al is not None))
                    assert check_codes(pq) == _lib.OK
    finally:
        ra.set_option("adc_range_wgs_per_query", 0)
    log = ra.launch_log(reset=True)
    for k in ("k_adc_range_lists_u8", "k_adc_ip_range_lists_u8", "k_adc_range_lists_residual_u8", "k_adc_ip_range_lists_residual_u8"):
        assert k in log, (k, log)
