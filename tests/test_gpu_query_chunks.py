"""Every query loop of the search drivers past its first chunk, on the GPU.  The calls are the ones
tests/query_chunks.py declares (test_query_chunks.py proves that each needs three launches with a shorter last chunk):
route S reaches the scratch bound with few queries (the grid option forced to its cap, long lists), route Y the 65,535 of
gridDim.y with 131,075 queries.  Route Y, and re-ranking on both routes, repeat PERIOD = 7 patterns of (query, probe row,
bias row, threshold, candidate row): query i uses pattern i mod 7, tiled on the device, and the reference is computed for
the patterns only.  The period divides no chunk, and the reference rows are pairwise different, so a row read from or
written to the place of another chunk cannot compare equal.

References: adc_lists_ref, adc_residual_ref, adc_masked_ref, adc_among_ref, adc_range_ref, flat_lists_ref, rerank_ref,
never another entry point of the library; row values of the ADC calls from the oracle's scan.  Indices exactly, values bit
for bit (a NaN as the canonical NaN), sentinels around the strided outputs intact (the raw-call helpers of the other GPU
tests), the range flag clear, and the launch log equal to the model's: every kernel x3."""
import zlib

import numpy as np
import pytest

import flat_lists_ref as flr
import query_chunks as qc
import rerank_ref as rr
from adc_among_ref import ref_among
from adc_ip_ref import assert_same, scores
from adc_range_ref import ref_range_lists, ref_range_residual
from oracle import pq_oracle as orc
from test_gpu_adc_among import among_raw
from test_gpu_adc_packed4 import dev_packed, flag, make_pq, mask_words, to_dev
from test_gpu_adc_range import call_raw as range_raw
from test_gpu_adc_range import fn_name as range_name
from test_gpu_adc_search_grid import call as search_call
from test_gpu_adc_search_grid import draw_tables, lists_name, lists_reference
from test_gpu_adc_search_lists import ra  # noqa: F401
from test_gpu_flat_lists import lists_raw as flat_lists_raw
from test_gpu_rerank import rerank_raw

ONE_ROW, TWO_ROWS, EMPTY = 1, 5, (2, 6)          # the lists of one row, of two rows and of none


def seed_of(c):
    return zlib.crc32(("%s %s %s" % (c.driver, c.item, c.route)).encode())


def pattern(c):
    """[nq]: the pattern of every query"""
    return np.arange(c.nq) % c.period


def tile_dev(a, c):
    """pattern rows [period, ...] -> device [nq, ...], tiled on the device"""
    import torch
    d = to_dev(a)
    if c.period == c.nq:
        return d
    return d[torch.arange(c.nq, device="cuda") % c.period].contiguous()


def widen(t, width, fill):
    """device [nq, w] -> the same rows as the first w columns of a [nq, width] tensor: a row stride of its own"""
    import torch
    wide = torch.full((t.shape[0], width), fill, dtype=t.dtype, device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


def tile_csr(lims, arrays, c):
    """CSR over the patterns -> (lims [nq + 1], arrays) over the queries"""
    P = c.period
    full, rest = divmod(c.nq, P)
    lens = np.diff(lims)[pattern(c)]
    out_lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = []
    for a in arrays:
        a = np.asarray(a)
        out.append(np.concatenate([np.tile(a[:lims[P]], full), a[:lims[rest]]]))
        assert out[-1].size == out_lims[-1]
    return out_lims, out


def assert_distinct(rows, what):
    """the reference rows of the patterns, as bytes, are pairwise different"""
    assert len(set(rows)) == len(rows), "%s: %d reference rows, %d different" % (what, len(rows), len(set(rows)))


def topk_rows(v, i):
    return [np.asarray(v[p], np.float32).tobytes() + np.asarray(i[p], np.int64).tobytes() for p in range(v.shape[0])]


def csr_rows(lims, v, i):
    return [np.asarray(v[lims[p]:lims[p + 1]], np.float32).tobytes() + np.asarray(i[lims[p]:lims[p + 1]], np.int64).tobytes()
            for p in range(lims.size - 1)]


def draw_lists(rng, n):
    """9 uneven lists: list 1 holds one row, list 5 two, lists 2 and 6 none"""
    cuts = np.sort(rng.choice(np.arange(1, n - 3), 4, replace=False))
    a, b, cc, d, e = np.diff(np.concatenate([[0], cuts, [n - 3]]))
    sizes = np.array([a, 1, 0, b, cc, 2, 0, d, e], np.int64)
    assert sizes.size == qc.N_LISTS and sizes.sum() == n and all(sizes[l] == 0 for l in EMPTY)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def draw_probes(rng, period):
    """[period, 3], pairwise different rows of two distinct lists and one -1, never the two empty lists together;
    pattern 0 reaches one row and pattern 1 two, so that k = 3 also returns padding"""
    rows = [(ONE_ROW, -1, EMPTY[0]), (TWO_ROWS, EMPTY[1], -1)]
    while len(rows) < period:
        r = tuple(int(x) for x in np.insert(rng.permutation(qc.N_LISTS)[:qc.N_PROBE - 1], rng.integers(0, qc.N_PROBE), -1))
        if r not in rows and not set(EMPTY) <= set(r):
            rows.append(r)
    return np.array(rows, np.int64)


def draw_bias(rng, pr):
    """a bias row per pattern; NaN where a probe is skipped (never read into a result)"""
    bias = rng.standard_normal(pr.shape).astype(np.float32)
    bias[(pr < 0) | np.isin(pr, EMPTY)] = np.nan
    return bias


def draw_allow(rng, off):
    """about half of the rows, the rows of the two short lists among them"""
    allow = rng.random(int(off[-1])) < 0.5
    allow[off[ONE_ROW]] = True
    allow[off[TWO_ROWS]:off[TWO_ROWS + 1]] = True
    return allow


class forced:
    """the driver's grid option for the calls of one item"""

    def __init__(self, ra, c):
        self.ra, self.option, self.G = ra, qc.OPTIONS[c.driver], c.G

    def __enter__(self):
        self.ra.set_option(self.option, self.G)

    def __exit__(self, *exc):
        self.ra.set_option(self.option, 0)


def logged(ra, pq, run):
    """(what run() returns, the launch log of its calls, the range flag after them)"""
    pq._cb()                                  # the handle is created on first use, with launches of its own
    ra.launch_log(reset=True)
    got = run()
    return got, ra.launch_log(reset=True), flag(pq)


# ---- ADC list searches: adc_search_lists_run -----------------------------------------------------------------------
def lists_data(c):
    """everything the item needs that no GPU computes: inputs per pattern and the reference rows"""
    rng = np.random.default_rng(seed_of(c))
    family = "p4" if c.item == "packed4" else "u8"
    K = qc.K_P4 if family == "p4" else qc.K_U8
    ip = c.item in ("ip_scaled", "packed4")
    residual, masked = c.item == "residual", c.item == "masked"
    t = draw_tables(rng, c.period, qc.M, K)
    codes = rng.integers(0, K, (c.n, qc.M)).astype(np.uint8)
    off = draw_lists(rng, c.n)
    pr = draw_probes(rng, c.period)
    bias = draw_bias(rng, pr)
    x = rng.standard_normal(c.n).astype(np.float32)              # scales (IP) or row terms (residual distance)
    allow = draw_allow(rng, off) if masked else None
    s = orc.adc_scan(t, codes)
    values = s if residual else (scores(s, x) if ip else s)
    want = lists_reference(values, allow, off, pr, bias, c.k, ip, residual, None if ip else x, x if ip else None)
    assert_distinct(topk_rows(*want), c)
    assert (want[1][0] >= 0).sum() == 1 and (want[1][1] >= 0).sum() == 2          # padding also at k = 3
    return dict(family=family, K=K, ip=ip, residual=residual, t=t, codes=codes, off=off, pr=pr, bias=bias, x=x, allow=allow,
                want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("item,route", qc.case_ids("lists"))
def test_gpu_lists_search_query_chunks(ra, item, route):
    c = qc.case("lists", item, route)
    d = lists_data(c)
    ip, residual = d["ip"], d["residual"]
    pq = make_pq(ra, qc.M, d["K"])
    td = tile_dev(d["t"], c)
    cd = dev_packed(ra, d["codes"], d["K"]) if d["family"] == "p4" else to_dev(d["codes"])
    lo = to_dev(d["off"])
    prd = widen(tile_dev(d["pr"], c), qc.P_RS, 0)
    assert prd.stride(0) == qc.P_RS
    kw = dict(lists=(lo, prd))
    if residual:
        kw["bias"] = widen(tile_dev(d["bias"], c), qc.B_RS, float("nan"))
        assert kw["bias"].stride(0) == qc.B_RS
    if ip or residual:
        kw.update(extra=to_dev(d["x"]), has_extra=True)
    words = None if d["allow"] is None else mask_words(d["allow"])
    want_v, want_i = d["want"][0][pattern(c)], d["want"][1][pattern(c)]
    with forced(ra, c):
        got, log, f = logged(ra, pq, lambda: search_call(lists_name(ip, residual), d["family"], pq, td, cd, words, c.k, **kw))
        assert log == qc.log(c, ip=ip), log
        assert_same(got[0], got[1], want_v, want_i)
        assert f == 0
        if item == "l2":                      # and through the Python entry point
            got, log, f = logged(ra, pq, lambda: pq.adc_search_lists_device(cd, td, lo, prd, c.k, check=True))
            assert log == qc.log(c), log
            assert_same(got[0].cpu().numpy(), got[1].cpu().numpy(), want_v, want_i)
            assert f == 0


# ---- exact search in probed lists: pqhip_flat_search_lists_f32_dev -------------------------------------------------
def flat_lists_data(c):
    rng = np.random.default_rng(seed_of(c))
    ip, half, masked = c.item == "ip_f16", c.item in ("ip_f16", "masked"), c.item == "masked"
    q = rng.standard_normal((c.period, qc.D)).astype(np.float32)
    x = rng.standard_normal((c.n, qc.D)).astype(np.float16 if half else np.float32)
    off = draw_lists(rng, c.n)
    pr = draw_probes(rng, c.period)
    allow = draw_allow(rng, off) if masked else None
    want_v, want_i, flagged = flr.ref_flat_search_lists(q, x, off, pr, c.k, ip=ip, allow=allow)
    assert not flagged
    assert_distinct(topk_rows(want_v, want_i), c)
    return dict(ip=ip, q=q, x=x, off=off, pr=pr, allow=allow, want=(want_v, want_i))


@pytest.mark.gpu
@pytest.mark.parametrize("item,route", qc.case_ids("flat_lists"))
def test_gpu_flat_lists_query_chunks(ra, item, route):
    import torch
    c = qc.case("flat_lists", item, route)
    d = flat_lists_data(c)
    pq = make_pq(ra, qc.M, qc.K_U8)           # any quantizer: the call borrows its slot, scratch and flag
    qd = widen(tile_dev(d["q"], c), qc.D + 3, float("nan"))
    xd, od, pd = to_dev(d["x"]), to_dev(d["off"]), tile_dev(d["pr"], c)
    wd = None if d["allow"] is None else torch.from_numpy(flr.mask_words(d["allow"])).cuda()
    with forced(ra, c):
        got, log, f = logged(ra, pq, lambda: flat_lists_raw(pq, qd, xd, od, pd, c.k, d["ip"], words=wd))
    assert log == qc.log(c, ip=d["ip"]), log
    flr.assert_same(got[0], got[1], d["want"][0][pattern(c)], d["want"][1][pattern(c)])
    assert f == 0


# ---- ADC search among given rows: adc_among ------------------------------------------------------------------------
def among_data(c):
    rng = np.random.default_rng(seed_of(c))
    shared, residual = c.item == "shared", c.item == "residual"
    ip = shared
    t = draw_tables(rng, c.period, qc.M, qc.K_U8)
    codes = rng.integers(0, qc.K_U8, (c.n, qc.M)).astype(np.uint8)
    off = draw_lists(rng, c.n)
    row_list = np.repeat(np.arange(qc.N_LISTS, dtype=np.int64), np.diff(off))
    x = rng.standard_normal(c.n).astype(np.float32)              # scales (shared: IP) or row terms (residual distance)
    bias = rng.standard_normal((c.period, qc.N_LISTS)).astype(np.float32)
    if shared:
        ids = rng.choice(c.n, qc.AMONG_MAX_IDS - 3, replace=False).astype(np.int64)
        ids[5] = -1
        lims = None
    else:
        lens = rng.integers(3, qc.AMONG_MAX_IDS + 1, c.period)
        lens[:5] = (1, 2, 0, qc.AMONG_MAX_IDS, 3)                # uneven, one empty; k = 3 also returns padding
        parts = []
        for n_ids in lens.tolist():
            rows = rng.choice(c.n, n_ids, replace=False).astype(np.int64)
            if n_ids > 3:
                rows[rng.integers(0, n_ids)] = -1
            parts.append(rows)
        ids = np.concatenate(parts)
        lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s = orc.adc_scan(t, codes)
    want_v, want_i, flagged = ref_among(s, ids, c.k, lims=lims, ip=ip, extra=x if (ip or residual) else None,
                                        row_list=row_list if residual else None, bias=bias if residual else None)
    assert not flagged
    assert_distinct(topk_rows(want_v, want_i), c)
    return dict(ip=ip, residual=residual, t=t, codes=codes, row_list=row_list, x=x, bias=bias, ids=ids, lims=lims,
                want=(want_v, want_i))


@pytest.mark.gpu
@pytest.mark.parametrize("item,route", qc.case_ids("among"))
def test_gpu_among_query_chunks(ra, item, route):
    c = qc.case("among", item, route)
    d = among_data(c)
    ip, residual = d["ip"], d["residual"]
    pq = make_pq(ra, qc.M, qc.K_U8)
    td, cd = tile_dev(d["t"], c), to_dev(d["codes"])
    kw = {}
    if d["lims"] is None:
        ids = d["ids"]
    else:
        lims, (ids,) = tile_csr(d["lims"], [d["ids"]], c)
        assert np.diff(lims).max() <= qc.AMONG_MAX_IDS
        kw["lims"] = to_dev(lims)
    if residual:
        kw.update(row_list=to_dev(d["row_list"]), bias=widen(tile_dev(d["bias"], c), qc.AMONG_B_RS, float("nan")))
        assert kw["bias"].stride(0) == qc.AMONG_B_RS
    if ip or residual:
        kw["extra"] = to_dev(d["x"])
    idd = to_dev(ids)
    with forced(ra, c):
        got, log, f = logged(ra, pq, lambda: among_raw(pq, ip, cd, td, idd, c.k, **kw))
    assert log == qc.log(c, ip=ip), log
    assert_same(got[0], got[1], d["want"][0][pattern(c)], d["want"][1][pattern(c)])
    assert f == 0


# ---- ADC range search over probed lists: adc_range_lists -----------------------------------------------------------
def range_data(c):
    rng = np.random.default_rng(seed_of(c))
    residual = c.item == "residual_ip_scaled"
    ip = residual
    t = rng.standard_normal((c.period, qc.M, qc.K_U8)).astype(np.float32)
    codes = rng.integers(0, qc.K_U8, (c.n, qc.M)).astype(np.uint8)
    off = draw_lists(rng, c.n)
    pr = draw_probes(rng, c.period)
    bias = draw_bias(rng, pr)
    x = (rng.random(c.n) * 3 - 0.5).astype(np.float32)           # scales, some negative
    s = orc.adc_scan(t, codes)

    def ref(thr):
        if residual:
            return ref_range_residual(s, off, pr, bias, thr, scales=x, ip=True)
        return ref_range_lists(s, off, pr, thr)

    every = ref(np.full(c.period, -np.inf if ip else np.inf, np.float32))
    probed = np.diff(every[0])
    # the median of the values the pattern reaches: some of its rows qualify, not all
    thr = np.array([np.median(every[1][every[0][p]:every[0][p + 1]]) for p in range(c.period)]).astype(np.float32)
    want = ref(thr)
    hits = np.diff(want[0])
    assert (hits >= 1).all() and (hits[probed >= 2] < probed[probed >= 2]).all() and probed[0] == 1 and probed[1] == 2
    assert_distinct(csr_rows(*want), c)
    assert len(set(thr.tolist())) == c.period
    return dict(ip=ip, residual=residual, t=t, codes=codes, off=off, pr=pr, bias=bias, x=x, thr=thr, want=want)


def assert_csr(got, want, what):
    for g, w, part in zip(got, want, ("lims", "values", "indices")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, part)


@pytest.mark.gpu
@pytest.mark.parametrize("item,route", qc.case_ids("range_lists"))
def test_gpu_range_lists_query_chunks(ra, item, route):
    """lims carries the running total from chunk to chunk; also a pure count call and a capacity one short of the total"""
    c = qc.case("range_lists", item, route)
    d = range_data(c)
    ip, residual = d["ip"], d["residual"]
    pq = make_pq(ra, qc.M, qc.K_U8)
    td, cd, lo = tile_dev(d["t"], c), to_dev(d["codes"]), to_dev(d["off"])
    prd = widen(tile_dev(d["pr"], c), qc.P_RS, 0)
    thr = d["thr"][pattern(c)]
    kw = dict(lists=(lo, prd))
    if residual:
        kw.update(bias=widen(tile_dev(d["bias"], c), qc.B_RS, float("nan")), extra=to_dev(d["x"]), has_extra=True)
    lims, (val, idx) = tile_csr(d["want"][0], d["want"][1:], c)
    want = (lims, val.astype(np.float32), idx.astype(np.int64))
    total = int(lims[-1])
    assert c.nq <= total <= c.nq * c.n
    name = range_name(ip, lists=True, residual=residual)
    with forced(ra, c):
        got, log, f = logged(ra, pq, lambda: range_raw(pq, name, cd, td, thr, total, **kw))
        assert log == qc.log(c, ip=ip), log
        assert_csr(got, want, "capacity = total")
        assert f == 0
        if item == "l2":
            got, log, f = logged(ra, pq, lambda: range_raw(pq, name, cd, td, thr, 0, null_out=True, **kw))
            assert log == qc.log(c, ip=ip, count_only=True), log
            assert got[0].tobytes() == lims.tobytes() and got[1].size == 0 and f == 0
            got, log, f = logged(ra, pq, lambda: range_raw(pq, name, cd, td, thr, total - 1, **kw))      # canaries: in range_raw
            assert log == qc.log(c, ip=ip), log
            assert_csr(got, (lims, want[1][:total - 1], want[2][:total - 1]), "capacity = total - 1")
            assert f == 0


# ---- exact re-ranking: pqhip_rerank_f32_dev ------------------------------------------------------------------------
def rerank_data(c):
    rng = np.random.default_rng(seed_of(c))
    ip, half = c.item == "ip_f16", c.item == "ip_f16"
    q = rng.standard_normal((c.period, qc.D)).astype(np.float32)
    x = rng.standard_normal((c.n, qc.D)).astype(np.float16 if half else np.float32)
    cand = np.stack([rng.permutation(c.n)[:c.n_cand] for _ in range(c.period)]).astype(np.int64)
    if c.n_cand > 2:
        cand[rng.random(cand.shape) < 0.1] = -1
        cand[0, 2:] = -1                                         # two candidates: padding at k = 5
    else:
        cand[0, 1] = -1                                          # one candidate of two
    want_v, want_i, flagged = rr.ref_rerank(q, x, cand, c.k, ip=ip)
    assert not flagged and (want_i >= 0).sum(1).min() < c.k
    assert_distinct(topk_rows(want_v, want_i), c)
    return dict(ip=ip, q=q, x=x, cand=cand, want=(want_v, want_i))


@pytest.mark.gpu
@pytest.mark.parametrize("item,route", qc.case_ids("rerank"))
def test_gpu_rerank_query_chunks(ra, item, route):
    c = qc.case("rerank", item, route)
    d = rerank_data(c)
    pq = make_pq(ra, qc.M, qc.K_U8)
    qd = widen(tile_dev(d["q"], c), qc.D + 3, float("nan"))
    xd = to_dev(d["x"])
    cd = tile_dev(d["cand"], c)
    if c.n_cand < 4:
        cd = widen(cd, 4, 0)
    with forced(ra, c):
        got, log, f = logged(ra, pq, lambda: rerank_raw(pq, qd, xd, cd, c.k, d["ip"]))
    assert log == qc.log(c), log
    rr.assert_same(got[0], got[1], d["want"][0][pattern(c)], d["want"][1][pattern(c)])
    assert f == 0


# ---- no row to search: search_padding_only -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("item", qc.ITEMS["padding"])
def test_gpu_padding_only_query_chunks(ra, item):
    """n = 0 rows: every query gets -1 and +Inf (L2) resp. -Inf (IP), in three launches of the merge kernel alone"""
    import torch
    c = qc.case("padding", item, "Y")
    pq = make_pq(ra, qc.M, qc.K_U8)
    k = c.k
    lo = to_dev(np.zeros(qc.N_LISTS + 1, np.int64))
    prd = torch.zeros((c.nq, c.n_probe), dtype=torch.int64, device="cuda")
    if item == "flat_lists":
        qd = torch.zeros((c.nq, qc.D), dtype=torch.float32, device="cuda")
        xd = to_dev(np.zeros((1, qc.D), np.float32))
    else:
        td = torch.zeros((c.nq, qc.M, qc.K_U8), dtype=torch.float32, device="cuda")
        cd = torch.zeros((1, qc.M), dtype=torch.uint8, device="cuda")[:0]       # no row, and an address all the same
        idd = to_dev(np.arange(5, dtype=np.int64))

    def run(ip):
        if item == "lists":
            return search_call(lists_name(ip, False), "u8", pq, td, cd, None, k, lists=(lo, prd), has_extra=ip)
        if item == "exhaustive":
            return search_call("adc_ip_search" if ip else "adc_search", "u8", pq, td, cd, None, k, has_extra=ip)
        if item == "among":
            return among_raw(pq, ip, cd, td, idd, k, n=0)
        return flat_lists_raw(pq, qd, xd, lo, prd, k, ip, n_rows=0)

    for ip in (False, True):
        got, log, f = logged(ra, pq, lambda: run(ip))
        assert log == qc.log(c, ip=ip), log
        assert got[0].shape == (c.nq, k) and (got[1] == -1).all()
        assert (np.isneginf(got[0]) if ip else np.isposinf(got[0])).all()
        assert f == 0
