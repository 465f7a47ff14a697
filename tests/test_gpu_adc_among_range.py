"""ADC range search among given rows on the GPU (pqhip_adc_among_range_f32_dev, pqhip_adc_ip_among_range_f32_dev): the
kernel against the sequential-f32 numpy model (candidate rules and row values of tests/adc_among_ref.py, the predicate in
the order named), then the batch routes against the plain range calls of the same process; all bit for bit."""
import ctypes

import numpy as np
import pytest

import synth
from adc_among_ref import among_values, candidates
from oracle import pq_oracle as orc

OPTION = "adc_among_range_wgs_per_query"
N, NQ, PER_QUERY = 3000, 3, 2500
# one M per row width the launcher instantiates (4, 8, 13, 25 dwords), odd ones at codes_row_stride == M; K < 256: the
# codes of rows that are not named can be poisoned too
SHAPES = [(15, 256), (17, 256), (53, 256), (100, 256), (3, 16)]


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_among_range(s, ids, lims, thr, ip, extra=None, row_list=None, bias=None):
    """CSR of the qualifying places of every query in the order named -> (lims, val, idx, flagged)"""
    n, n_lists = s.shape[1], 0 if bias is None else bias.shape[1]
    vals, idxs, flagged = [], [], False
    for q in range(s.shape[0]):
        mine = ids if lims is None else ids[int(lims[q]):int(lims[q + 1])]
        flagged |= candidates(ids, lims, q, n, row_list, n_lists)[1]
        rows = mine[(mine >= 0) & (mine < n)]
        if row_list is not None:
            rows = rows[(row_list[rows] >= 0) & (row_list[rows] < n_lists)]
        v = among_values(s[q], rows, ip, extra, row_list, None if bias is None else bias[q])
        with np.errstate(invalid="ignore"):
            hit = v >= thr[q] if ip else v <= thr[q]
        vals.append(v[hit])
        idxs.append(rows[hit])
    out_lims = np.concatenate([[0], np.cumsum([v.size for v in vals])]).astype(np.int64)
    return out_lims, np.concatenate(vals).astype(np.float32), np.concatenate(idxs).astype(np.int64), flagged


def same(got, want):
    for g, w in zip(got, want):
        g, w = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (g, w))
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def draw_ids(rng, bad):
    """NQ x PER_QUERY unsorted ids with -1 and one duplicate; bad: also an id >= n and one < -1"""
    parts = []
    for q in range(NQ):
        p = rng.permutation(N)[:PER_QUERY].astype(np.int64)
        p[[7, 1500]] = -1
        p[900] = p[100]
        if bad and q == 1:
            p[[3, 2000]] = N, -7
        parts.append(p)
    return np.concatenate(parts), np.arange(NQ + 1, dtype=np.int64) * PER_QUERY


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("M,K", SHAPES)
def test_gpu_among_range_matches_the_model(ra, M, K, ip, residual):
    """shared list and per-query lims, 1 and 3 workgroups per query (2,500 places: two full trips and a partial one, with
    3 workgroups slices of 834 places that end off a 64-place boundary); thresholds mid-range, +-Inf and NaN, a NaN table
    entry that a named row reaches; rows that are not named are poisoned and must not raise the flag"""
    rng = np.random.default_rng(9700 + M + 2 * ip + residual)
    n_lists = 7
    pq = ra.Pq(None, synth.normalish(9701 + M, (M, K, 1)))
    codes = synth.codes_u8(9702 + M, (N, M), K)
    t = rng.standard_normal((NQ, M, K)).astype(np.float32)
    ids, lims = draw_ids(np.random.default_rng(9790 + M), bad=False)
    t[0, 0, codes[ids[5], 0]] = np.nan
    with np.errstate(invalid="ignore"):
        s = orc.adc_scan(t, codes)
    extra = ((rng.random(N) * 3 - 0.5) if ip else rng.standard_normal(N)).astype(np.float32) if (ip or residual) else None
    row_list = rng.integers(0, n_lists, N).astype(np.int64) if residual else None
    bias = rng.standard_normal((NQ, n_lists)).astype(np.float32) if residual else None
    off = np.ones(N, bool)                                             # poison: whatever belongs to a row that no query names
    off[ids[ids >= 0]] = False
    p_codes, p_extra, p_list = codes.copy(), None if extra is None else extra.copy(), None if row_list is None else row_list.copy()
    if K < 256:
        p_codes[off] = K
    if extra is not None:
        p_extra[off] = np.nan
    if residual:
        p_list[off] = -5
    v0 = among_values(s[0], ids[:PER_QUERY][ids[:PER_QUERY] >= 0], ip, extra, row_list, None if bias is None else bias[0])
    mid = np.nanquantile(v0, 0.8 if ip else 0.2)
    thr = np.array([mid, -np.inf if ip else np.inf, np.nan], np.float32)
    # the bias as a transposed view: the wrapper's contiguous copy must outlive both of its calls
    kw = dict(row_list=dev(p_list), list_bias=dev(bias.T.copy()).T) if residual else {}
    if extra is not None:
        kw["scales" if ip else "row_terms"] = dev(p_extra)
    call = pq.adc_ip_among_range_device if ip else pq.adc_among_range_device
    cd, td, thd = dev(p_codes), dev(t), dev(thr)
    bad_ids, _ = draw_ids(np.random.default_rng(9790 + M), bad=True)       # the same rows named
    try:
        for G in (1, 3):
            ra.set_option(OPTION, G)
            for use_lims in (False, True):
                ld = dev(lims) if use_lims else None
                want = ref_among_range(s, ids, lims if use_lims else None, thr, ip, extra, row_list, bias)
                places = PER_QUERY if use_lims else ids.size
                assert not want[3] and 0.1 < want[0][1] / places < 0.3 and want[0][3] == want[0][2]
                same(call(cd, td, dev(ids), thd, lims=ld, check=True, **kw), want[:3])
                want = ref_among_range(s, bad_ids, lims if use_lims else None, thr, ip, extra, row_list, bias)
                assert want[3]
                same(call(cd, td, dev(bad_ids), thd, lims=ld, **kw), want[:3])
                with pytest.raises(ra.PanicError, match="index out of bounds"):
                    call(cd, td, dev(bad_ids), thd, lims=ld, check=True, **kw)
    finally:
        ra.set_option(OPTION, 0)


@pytest.mark.gpu
def test_gpu_among_range_capacity_and_a_range_beyond_the_bitmap(ra):
    """capacity = half of the total: the prefix is written, the guard after it is untouched, lims holds the true counts.
    One of 32 queries names 7,000 of the 8,000 ids: its trips beyond its bitmap take the fill pass's path without a mask."""
    import torch
    from reductive_amd import _lib
    M, K, nq = 15, 256, 32
    rng = np.random.default_rng(9750)
    pq = ra.Pq(None, synth.normalish(9751, (M, K, 1)))
    codes = synth.codes_u8(9752, (N, M), K)
    t = rng.standard_normal((nq, M, K)).astype(np.float32)
    s = orc.adc_scan(t, codes)
    ids = rng.integers(0, N, 8000).astype(np.int64)
    lims = np.concatenate([[0], np.cumsum([50, 7000] + [32] * 29 + [22])]).astype(np.int64)
    thr = np.quantile(s, 0.3, axis=1).astype(np.float32)
    want = ref_among_range(s, ids, lims, thr, False)
    total, guard = int(want[0][-1]), 32
    assert lims[-1] == ids.size and total > 2000 and want[0][2] - want[0][1] > 1500
    cd, td, idd, ld, thd = dev(codes), dev(t), dev(ids), dev(lims), dev(thr)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        for G, cap in ((1, total), (3, total // 2)):
            ra.set_option(OPTION, G)
            out_lims = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
            val = torch.full((cap + guard,), 7.5, dtype=torch.float32, device="cuda")
            idx = torch.full((cap + guard,), -9, dtype=torch.int64, device="cuda")
            rc = _lib.lib().pqhip_adc_among_range_f32_dev(pq._cb(), 0, td.data_ptr(), nq, cd.data_ptr(), 1, N, M, ld.data_ptr(),
                                                          idd.data_ptr(), ids.size, None, 0, None, 0, None, thd.data_ptr(),
                                                          out_lims.data_ptr(), val.data_ptr(), idx.data_ptr(), cap, stream)
            assert rc == _lib.OK
            same((out_lims, val[:cap], idx[:cap]), (want[0], want[1][:cap], want[2][:cap]))
            assert (val[cap:] == 7.5).all() and (idx[cap:] == -9).all()
    finally:
        ra.set_option(OPTION, 0)


@pytest.fixture(scope="module")
def index(ra):
    """20,000 rows in 16 lists, 40 queries: more than one screen group of 32 queries"""
    import torch
    M, K, n, nq, n_lists = 15, 256, 20000, 40, 16
    rng = np.random.default_rng(9760)
    pq = ra.Pq(None, synth.normalish(9761, (M, K, 2)))
    codes = dev(synth.codes_u8(9762, (n, M), K))
    q = dev(rng.standard_normal((nq, 2 * M)).astype(np.float32))
    sizes = rng.multinomial(n, np.ones(n_lists) / n_lists)
    list_off = dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    probes = np.stack([rng.permutation(n_lists)[:4] for _ in range(nq)]).astype(np.int64)
    probes[1, 2] = probes[1, 0]                                            # a list named twice
    probes[2, 1:] = -1                                                     # padding
    scales = dev((rng.random(n) + 0.5).astype(np.float32))
    allow = pq.pack_row_mask_device(dev(rng.random(n) < 0.5))
    tables = {False: pq.adc_tables_device(q), True: pq.adc_ip_tables_device(q)}
    thr = {ip: torch.quantile(pq.adc_scan_device(codes, tables[ip]) * (scales if ip else 1.0), 0.99 if ip else 0.01, dim=1)
           for ip in (False, True)}                                       # about 1 % of the rows qualify
    return dict(pq=pq, codes=codes, n=n, list_off=list_off, probes=dev(probes), scales=scales, allow=allow, tables=tables, thr=thr)


@pytest.mark.gpu
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_gpu_range_batch_routes_equal_the_plain_range_calls(ra, index, ip):
    import torch
    X = index
    pq, codes, t, thr = X["pq"], X["codes"], X["tables"][ip], X["thr"][ip]
    kw = {"scales": X["scales"]} if ip else {}
    plain = pq.adc_ip_range_device if ip else pq.adc_range_device
    among = pq.adc_ip_among_range_device if ip else pq.adc_among_range_device
    want = plain(codes, t, thr, **kw)
    assert int(want[0][-1]) > 40 * 100
    same(among(codes, t, torch.arange(X["n"], device="cuda"), thr, **kw), want)
    for allow in (None, X["allow"]):
        want = plain(codes, t, thr, allow=allow, **kw)
        for bits in (8, 16):
            same(pq.adc_range_batch_device(codes, t, thr, ip=ip, allow=allow, image_bits=bits, check=True, **kw), want)
    plain_lists = pq.adc_ip_range_lists_device if ip else pq.adc_range_lists_device
    want = plain_lists(codes, t, X["list_off"], X["probes"], thr, **kw)
    assert want[0][2] > want[0][1] and want[0][3] > want[0][2]
    same(pq.adc_range_lists_batch_device(codes, t, X["list_off"], X["probes"], thr, ip=ip, check=True, **kw), want)


@pytest.mark.gpu
def test_gpu_matrix_range_routes(ra):
    """within(screen=) equals within(); within_among over the rows of a wider radius equals within() filtered to them"""
    import torch
    from reductive_amd import qmatrix
    M, K, n, nq = 15, 256, 6000, 5
    rng = np.random.default_rng(9770)
    pq = ra.Pq(None, synth.normalish(9771, (M, K, 2)))
    x = rng.standard_normal((n, 2 * M)).astype(np.float32)
    qm = qmatrix.QuantizedMatrix(pq, pq.quantize_batch(x))
    q = dev(x[:nq] + 0.1 * rng.standard_normal((nq, 2 * M)).astype(np.float32))
    r = float(torch.quantile(qm.distances(q), 0.02))
    want = qm.within(q, r)
    assert int(want[0][-1]) > nq
    for screen in (True, "u16"):
        same(qm.within(q, r, screen=screen), want)
    pm = qm.partition(8, n_iterations=2, vectors=x, rng=np.random.default_rng(9772))
    want = pm.within(q, r, 3)
    assert int(want[0][-1]) > nq
    same(pm.within(q, r, 3, screen=True), want)
    rm = qm.partition_residual(8, n_iterations=2, pq_iterations=2, vectors=x, rng=np.random.default_rng(9773))
    for m, r_m in ((pm, r), (rm, float(rm.nearest(q, 40, 3)[0][:, -1].min()))):
        want, wide = m.within(q, r_m, 3), m.within(q, 2 * r_m, 3)
        assert int(wide[0][-1]) > int(want[0][-1]) > nq
        same(m.within_among(q, wide[::2], r_m), want)
    t_hi, t_lo = (float(qm.most_similar(q, k)[0][:, -1].max()) for k in (40, 400))
    want = qm.similar_above(q, t_hi)
    assert int(want[0][-1]) >= 40
    same(qm.similar_above_among(q, qm.similar_above(q, t_lo)[::2], t_hi), want)
