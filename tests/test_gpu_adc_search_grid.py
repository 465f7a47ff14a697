"""Every instantiation of the ADC top-k producers against the independent numpy references, and the selection in its
steady state.  The calls are the ones tests/adc_search_cells.py declares (its CPU test proves that they cover every
cell); row values come from the oracle's scan of the tables the test draws, the results from ref_search,
adc_ip_ref, adc_lists_ref, adc_residual_ref and adc_masked_ref -- never from another entry point of the library.  A
packed call is checked against the same references on the unpacked codes, which is its definition.  Indices exactly,
values bit for bit (a NaN as the canonical NaN), sentinels around the strided outputs intact, the range flag 0, and the
launch log equal to the planner's names and pass counts."""
import numpy as np
import pytest

import adc_search_cells as cells
from adc_ip_ref import assert_same, ref_ip_search, scores
from adc_lists_ref import ref_lists_search
from adc_masked_ref import ref_masked_lists_search, ref_masked_residual_search, ref_masked_search
from adc_residual_ref import ref_residual_search
from oracle import pq_oracle as orc
from test_gpu_adc_packed4 import SENT_I, SENT_V, dev_packed, flag, make_pq, mask_words, stream_ptr, to_dev
from test_gpu_adc_search import ref_search


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def call(name, family, pq, tables, codes, allow, k, code_bytes=1, lists=None, bias=None, extra=None, has_extra=False, pad=3):
    """One search through the C ABI: the _masked entry point (d_allow NULL: the unmasked call itself) or the _packed4
    one, row strides k + pad, sentinels around the outputs -> (value, idx) numpy [nq, k]."""
    import torch
    from reductive_amd import _lib
    nq = tables.shape[0]
    n, W = codes.shape
    rs = k + pad
    vbuf = torch.full((nq * rs + 2 * pad,), float(SENT_V), dtype=torch.float32, device="cuda")
    ibuf = torch.full((nq * rs + 2 * pad,), SENT_I, dtype=torch.int64, device="cuda")
    args = [pq._cb(), 0, tables.data_ptr(), nq, codes.data_ptr()]
    if family != "p4":
        args.append(code_bytes)
    args += [n, codes.stride(0) if n > 1 else W, None if allow is None else allow.data_ptr()]
    if lists is not None:
        lo, pr = lists
        args += [lo.data_ptr(), lo.shape[0] - 1, pr.data_ptr(), pr.shape[1], pr.stride(0) if nq > 1 else pr.shape[1]]
        if bias is not None:
            args += [bias.data_ptr(), bias.stride(0) if nq > 1 else pr.shape[1]]
    if has_extra:
        args.append(None if extra is None else extra.data_ptr())
    args += [k, vbuf.data_ptr() + 4 * pad, rs, ibuf.data_ptr() + 8 * pad, rs, stream_ptr()]
    full = "pqhip_%s_%s_f32_dev" % (name, "packed4" if family == "p4" else "masked")
    rc = getattr(_lib.lib(), full)(*args)
    assert rc == _lib.OK, (full, rc)
    vb, ib = vbuf.cpu().numpy(), ibuf.cpu().numpy()
    body = np.zeros(vb.size, bool)
    for q in range(nq):
        body[pad + q * rs: pad + q * rs + k] = True
    assert (vb[~body] == SENT_V).all() and (ib[~body] == SENT_I).all(), "write outside the outputs"
    return vb[body].reshape(nq, k), ib[body].reshape(nq, k)


def checked(ra, pq, want, k, planned, name, family, *args, **kw):
    """the call, its launch log against the planner's, the range flag, the result against the first k of `want`"""
    pq._cb()                                  # the handle is created on first use, with launches of its own
    ra.launch_log(reset=True)
    got_v, got_i = call(name, family, pq, *args, k, **kw)
    log = ra.launch_log(reset=True)
    assert flag(pq) == 0, (name, k)
    assert planned is not None and log == cells.log_text(planned.log), (name, k, log, planned)
    assert_same(got_v, got_i, want[0][:, :k], want[1][:, :k])


def draw_tables(rng, nq, M, K):
    """the first half of the queries normal f32 (the sequential f32 chain over m matters), the rest integer-valued in
    -3 .. 3 with NaN, +-Inf and -0 planted (ties at the k-th place); rarely enough that most row sums stay finite"""
    t = rng.standard_normal((nq, M, K)).astype(np.float32)
    h = nq // 2
    if nq > 1:
        t[h:] = rng.integers(-3, 4, (nq - h, M, K)).astype(np.float32)
        p = min(0.03, 0.1 / M)
        for s in (np.nan, np.inf, -np.inf, -0.0):
            t[h:][rng.random(t[h:].shape) < p] = s
    return t


def draw_codes(rng, n, M, K):
    codes = rng.integers(0, K, (n, M)).astype(np.uint8)
    if K == 256:
        codes[0, 0], codes[n - 1, M - 1] = 255, 128         # codes >= 128 are present
    return codes


def layouts(ra, family, codes, K):
    """Two device layouts of the same rows.  u8: a tight allocation of exactly n M bytes (the last rows take
    adc_fetch_row's byte-load path), and a view into a wider matrix -- row stride M + 3, base 1 byte into the
    allocation, every surrounding byte 255, so that with K < 256 a byte from outside a row raises the flag or changes a
    value.  Packed: exactly n PB bytes, and the same 1 byte into an allocation with the pad nibble of an odd M 0xF."""
    import torch
    n, M = codes.shape
    if family == "p4":
        raw = ra.pack_codes4(codes, n_centroids=K)
        if M % 2:
            raw[:, -1] |= 0xf0
        return [dev_packed(ra, codes, K), dev_packed(ra, codes, K, offset=1, raw=raw)]
    buf = torch.full((1 + n * (M + 3),), 255, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(n, M + 3)[:, :M]
    view.copy_(torch.from_numpy(codes))
    return [to_dev(codes), view]


def draw_masks(rng, n):
    """allow ~ 0.6, and the same with one whole 1,024-row trip cleared"""
    a = rng.random(n) < 0.6
    b = rng.random(n) < 0.6
    b[1024:2048] = False
    return [a, b]


def item_seed(*key):
    return abs(hash(tuple(int(x) for x in key))) % (1 << 31)


# ---- exhaustive searches: every (NV, NQ, L) ------------------------------------------------------------------------
EXHAUSTIVE = [(f, ip, m, M) for f, lists, ip, m, r, M in cells.grid_items() if not lists]


@pytest.mark.gpu
@pytest.mark.parametrize("family,ip,masked,M", EXHAUSTIVE)
def test_gpu_exhaustive_cells(ra, family, ip, masked, M):
    rng = np.random.default_rng(item_seed(1, family == "p4", ip, masked, M))
    name = "adc_ip_search" if ip else "adc_search"
    n, nq = cells.GRID_N, cells.GRID_NQ
    option = "adc_packed4_wgs" if family == "p4" else "adc_search_wgs"

    def reference(values, allow, k):
        if allow is not None:
            return ref_masked_search(values, allow, k, ip=ip)
        return ref_ip_search(values, k) if ip else ref_search(values, k)

    try:
        ra.set_option(option, cells.GRID_WGS)
        for K in cells.codebook_sizes(family, M):
            pq = make_pq(ra, M, K)
            codes = draw_codes(rng, n, M, K)
            t = draw_tables(rng, nq, M, K)
            td = to_dev(t)
            sc = rng.standard_normal(n).astype(np.float32)
            values = scores(orc.adc_scan(t, codes), sc) if ip else orc.adc_scan(t, codes)
            masks = draw_masks(rng, n) if masked else [None]
            kw = dict(extra=to_dev(sc), has_extra=True) if ip else {}
            plans = {k: cells.plan(cells.Call(family, False, ip, masked, False, M, K, k, nq, 1, 0, 0)) for k in cells.GRID_KS}
            for dev in layouts(ra, family, codes, K):
                for allow in masks:
                    words = None if allow is None else mask_words(allow)
                    want = reference(values, allow, cells.MAX_K)
                    for k in cells.GRID_KS:
                        checked(ra, pq, want, k, plans[k], name, family, td, dev, words, **kw)
            if K != 256:
                # the full scan: every row's value comes back (n < k), then the padding; IP without scales
                fn, fk = cells.FULL_SCAN
                sub = np.ascontiguousarray(codes[:fn])
                fv = orc.adc_scan(t, sub)
                allow = None if not masked else masks[0][:fn]
                want = reference(fv, allow, fk)
                assert (want[1][:, fn:] == -1).all() and (want[1][:, :fn if allow is None else int(allow.sum())] >= 0).all()
                checked(ra, pq, want, fk, plans[fk], name, family, td, layouts(ra, family, sub, K)[0],
                        None if allow is None else mask_words(allow), has_extra=ip)
    finally:
        ra.set_option(option, 0)


# ---- list searches: every (NV, L), plain and residual, with and without a mask -------------------------------------
LISTS = [(f, ip, m, r, M) for f, lists, ip, m, r, M in cells.grid_items() if lists]


def draw_lists(rng, n, nq):
    """9 lists, one of them empty, all probed by every query in a shuffled order with one -1 among the probes"""
    cuts = np.sort(rng.choice(np.arange(1, n), 7, replace=False))
    off = np.concatenate([[0], cuts[:4], [cuts[3]], cuts[4:], [n]]).astype(np.int64)      # list 4 is empty
    assert off.size == 10 and (np.diff(off) == 0).sum() == 1
    pr = np.stack([np.insert(rng.permutation(9), rng.integers(0, 10), -1) for _ in range(nq)]).astype(np.int64)
    assert pr.shape[1] == cells.LISTS_N_PROBE
    return off, pr


def lists_reference(values_or_s, allow, off, pr, bias, k, ip, residual, terms, scales):
    if residual:
        if allow is not None:
            return ref_masked_residual_search(values_or_s, allow, off, pr, bias, k, terms=terms, scales=scales, ip=ip)
        return ref_residual_search(values_or_s, off, pr, bias, k, terms=terms, scales=scales, ip=ip)
    if allow is not None:
        return ref_masked_lists_search(values_or_s, allow, off, pr, k, ip=ip)
    return ref_lists_search(values_or_s, off, pr, k, ip=ip)


def lists_name(ip, residual):
    return "adc_%ssearch_lists%s" % ("ip_" if ip else "", "_residual" if residual else "")


@pytest.mark.gpu
@pytest.mark.parametrize("family,ip,masked,residual,M", LISTS)
def test_gpu_lists_cells(ra, family, ip, masked, residual, M):
    rng = np.random.default_rng(item_seed(2, family == "p4", ip, masked, residual, M))
    n, nq = cells.GRID_N, cells.GRID_NQ
    name = lists_name(ip, residual)
    try:
        ra.set_option("adc_lists_wgs_per_query", cells.LISTS_G)
        for K in cells.codebook_sizes(family, M):
            pq = make_pq(ra, M, K)
            codes = draw_codes(rng, n, M, K)
            t = draw_tables(rng, nq, M, K)
            td = to_dev(t)
            off, pr = draw_lists(rng, n, nq)
            bias = rng.standard_normal(pr.shape).astype(np.float32)
            bias[(pr < 0) | (pr == 4)] = np.nan                                  # a skipped probe's bias is never read
            x = rng.standard_normal(n).astype(np.float32)                       # scales (IP) or row terms (residual distance)
            s = orc.adc_scan(t, codes)
            values = s if residual else (scores(s, x) if ip else s)
            masks = draw_masks(rng, n) if masked else [None]
            kw = dict(lists=(to_dev(off), to_dev(pr)))
            if residual:
                kw["bias"] = to_dev(bias)
            if ip or residual:
                kw.update(extra=to_dev(x), has_extra=True)
            plans = {k: cells.plan(cells.Call(family, True, ip, masked, residual, M, K, k, nq, 1, cells.LISTS_N_PROBE, cells.LISTS_G))
                     for k in cells.GRID_KS}
            for dev in layouts(ra, family, codes, K):
                for allow in masks:
                    words = None if allow is None else mask_words(allow)
                    want = lists_reference(values, allow, off, pr, bias, cells.MAX_K, ip, residual,
                                           None if ip else x, x if ip else None)
                    for k in cells.GRID_KS:
                        checked(ra, pq, want, k, plans[k], name, family, td, dev, words, **kw)
    finally:
        ra.set_option("adc_lists_wgs_per_query", 0)


# ---- the generic producer: any code width, table in LDS or through L2 ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ip", (False, True))
def test_gpu_generic_cells(ra, ip):
    rng = np.random.default_rng(item_seed(3, ip))
    n, nq = cells.GRID_N, 2
    name = "adc_ip_search" if ip else "adc_search"
    try:
        ra.set_option("adc_search_wgs", cells.GRID_WGS)
        for code_bytes, M, K in cells.GENERIC_SHAPES:
            pq = make_pq(ra, M, K)
            codes = rng.integers(0, K, (n, M)).astype(np.uint8 if code_bytes == 1 else np.int32)
            t = draw_tables(rng, nq, M, K)
            sc = rng.standard_normal(n).astype(np.float32)
            values = scores(orc.adc_scan(t, codes), sc) if ip else orc.adc_scan(t, codes)
            want = ref_ip_search(values, cells.MAX_K) if ip else ref_search(values, cells.MAX_K)
            kw = dict(extra=to_dev(sc), has_extra=True) if ip else {}
            td, cd = to_dev(t), to_dev(codes)
            for k in cells.UPPER_KS:
                planned = cells.plan(cells.Call("u8", False, ip, False, False, M, K, k, nq, code_bytes, 0, 0))
                assert [c.family for c in planned.cells][0] == ("any_u8" if code_bytes == 1 else "any_u32")
                checked(ra, pq, want, k, planned, name, "u8", td, cd, None, code_bytes=code_bytes, **kw)
    finally:
        ra.set_option("adc_search_wgs", 0)


# ---- the selection in its steady state -----------------------------------------------------------------------------
# Independent of the row width: M = 3, K = 16 serves every producer.  One forced workgroup hands each wave 5 * 64 L rows
# of a list of 64 L entries, so the list fills, the threshold becomes a real row and most rows are rejected against it.
STEADY_M, STEADY_K, STEADY_NQ = 3, 16, 8
ORDERS = ("random", "ascending", "descending", "four rows", "late k-th")
LATE_WAVE, LATE_LANE = 5, 17
_STEADY = {}


def steady_rows(L):
    return cells.SEARCH_WAVES * 5 * 64 * L


def steady_value(s, ip, residual, bias_q, terms):
    """the value of every row for every query; the residual bias is one number per query (the same on every probe slot),
    so a row's value does not depend on where it is stored"""
    with np.errstate(invalid="ignore", over="ignore"):
        if not residual:
            return s
        if ip:
            return (bias_q[:, None] + s).astype(np.float32)
        return ((bias_q[:, None] + terms[None]).astype(np.float32) - (s + s).astype(np.float32)).astype(np.float32) + np.float32(0)


def steady_data(L, order, ip, residual):
    """codes, tables, row terms, bias per query and the values [8, n], the rows in the order asked for: ascending /
    descending in the order key of query 0 (the key of -score for the similarity searches)"""
    key = (L, order, ip, residual)
    if key not in _STEADY:
        rng = np.random.default_rng(item_seed(4, L, ORDERS.index(order), ip, residual))
        n = steady_rows(L)
        t = rng.standard_normal((STEADY_NQ, STEADY_M, STEADY_K)).astype(np.float32)
        codes = rng.integers(0, STEADY_K, (n, STEADY_M)).astype(np.uint8)
        terms = rng.standard_normal(n).astype(np.float32)
        bias_q = rng.standard_normal(STEADY_NQ).astype(np.float32)
        if order == "four rows":
            pick = rng.integers(0, 4, n)
            codes, terms = np.ascontiguousarray(codes[:4][pick]), np.ascontiguousarray(terms[:4][pick])
        elif order == "late k-th":
            # One wave supplies the whole result and its k-th row (k = 64 L) comes last.  A wave's k-th entry matters to
            # the result only when the k - 1 rows before it are the same wave's, so only this order sees a threshold that
            # is one entry too strict.  Every value is a function of the code alone (constant row terms); the 64 L + 1
            # smallest distinct rows go to wave LATE_WAVE of workgroup 0: all but the k-th in its first L trips, which
            # fill the list, then a trip of larger rows, then the k-th, which must still enter.
            terms[:] = np.float32(0.25)
            every = np.stack(np.meshgrid(*[np.arange(STEADY_K)] * STEADY_M, indexing="ij"), -1).reshape(-1, STEADY_M).astype(np.uint8)
            v0 = steady_value(orc.adc_scan(t, every), ip, residual, bias_q, np.full(every.shape[0], 0.25, np.float32))[0].astype(np.float64)
            o = np.argsort(-v0 if ip else v0, kind="stable")
            m, k = 64 * L + 1, 64 * L
            assert (np.diff((-v0 if ip else v0)[o][:m + 1]) > 0).all()
            special, pool = every[o[:m]], every[o[m:]]
            codes = np.ascontiguousarray(pool[rng.integers(0, pool.shape[0], n)])
            for trip in range(L):
                lanes = rng.permutation(64)
                for j in range(64):
                    e = trip * 64 + j
                    codes[trip * 1024 + LATE_WAVE * 64 + lanes[j]] = special[e if e < k - 1 else e + 1]
            codes[(L + 1) * 1024 + LATE_WAVE * 64 + LATE_LANE] = special[k - 1]
        elif order != "random":
            v0 = steady_value(orc.adc_scan(t, codes), ip, residual, bias_q, terms)[0].astype(np.float64)
            v0 = -v0 if ip else v0
            perm = np.argsort(v0 if order == "ascending" else -v0, kind="stable")
            codes, terms = np.ascontiguousarray(codes[perm]), np.ascontiguousarray(terms[perm])
        values = steady_value(orc.adc_scan(t, codes), ip, residual, bias_q, terms)
        _STEADY[key] = (codes, t, terms, bias_q, values)
    return _STEADY[key]


def least_wave_share(n, per, allow):
    """the fewest allowed rows any wave of any workgroup sees when the rows (or the places of the probed concatenation)
    are cut into ranges of `per` and a wave takes 64 of every 1,024"""
    live = np.ones(n, bool) if allow is None else allow
    least = n
    for b in range(0, n, per):
        r = np.arange(b, min(b + per, n))
        wave = ((r - b) % 1024) // 64
        least = min(least, int(np.bincount(wave[live[r]], minlength=cells.SEARCH_WAVES).min()))
    return least


def steady_mask(seed, n, L):
    """allow ~ 0.7; the rows of the "late k-th" order that carry the result are allowed"""
    allow = np.random.default_rng(seed).random(n) < 0.7
    for trip in range(L + 2):
        allow[trip * 1024 + LATE_WAVE * 64: trip * 1024 + LATE_WAVE * 64 + 64] = True
    return allow


def edge_ks(L):
    return (1 if L == 1 else 32 * L + 1, 64 * L)


STEADY_EXHAUSTIVE = [(f, ip, m, L) for f in ("u8", "p4") for ip in (False, True) for m in (False, True) for L in cells.LIST_REGS]


@pytest.mark.gpu
@pytest.mark.parametrize("family,ip,masked,L", STEADY_EXHAUSTIVE)
def test_gpu_steady_state_exhaustive(ra, family, ip, masked, L):
    name = "adc_ip_search" if ip else "adc_search"
    option = "adc_packed4_wgs" if family == "p4" else "adc_search_wgs"
    n = steady_rows(L)
    pq = make_pq(ra, STEADY_M, STEADY_K)
    allow = steady_mask(item_seed(5, L), n, L) if masked else None
    words = None if allow is None else mask_words(allow)
    try:
        for order in ORDERS:
            codes, t, terms, bias_q, values = steady_data(L, order, ip, False)
            dev = layouts(ra, family, codes, STEADY_K)[0]
            for nq in [c for c in cells.QUERIES_PER_PASS if c * L <= 16]:
                td = to_dev(t[:nq])
                v = values[:nq]
                if allow is not None:
                    want = ref_masked_search(v, allow, 64 * L, ip=ip)
                else:
                    want = ref_ip_search(v, 64 * L) if ip else ref_search(v, 64 * L)
                for wgs in (1, 2):
                    # a forced grid keeps the rows per workgroup a multiple of 1,024
                    per = -(-(-(-n // wgs)) // 1024) * 1024
                    if order in ("random", "descending"):
                        assert least_wave_share(n, per, allow) > 64 * L
                    ra.set_option(option, wgs)
                    for k in edge_ks(L):
                        planned = cells.plan(cells.Call(family, False, ip, masked, False, STEADY_M, STEADY_K, k, nq, 1, 0, 0))
                        assert [c for c in planned.cells if c.family == family][0].nq == nq
                        checked(ra, pq, want, k, planned, name, family, td, dev, words, has_extra=ip)
    finally:
        ra.set_option(option, 0)


STEADY_LISTS = [(f, ip, m, r, L) for f in ("u8", "p4") for ip in (False, True) for m in (False, True) for r in (False, True)
                for L in cells.LIST_REGS]


@pytest.mark.gpu
@pytest.mark.parametrize("family,ip,masked,residual,L", STEADY_LISTS)
def test_gpu_steady_state_lists(ra, family, ip, masked, residual, L):
    """7 lists, all probed in list order (the walk is then the row order), G forced to 1 and to 2"""
    name = lists_name(ip, residual)
    n = steady_rows(L)
    pq = make_pq(ra, STEADY_M, STEADY_K)
    rng = np.random.default_rng(item_seed(6, L))
    allow = steady_mask(item_seed(8, L), n, L) if masked else None
    words = None if allow is None else mask_words(allow)
    off = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), 6, replace=False)), [n]]).astype(np.int64)
    pr = np.arange(7, dtype=np.int64)[None]
    try:
        for order in ORDERS:
            codes, t, terms, bias_q, values = steady_data(L, order, ip, residual)
            dev = layouts(ra, family, codes, STEADY_K)[0]
            kw = dict(lists=(to_dev(off), to_dev(pr)))
            if residual:
                kw["bias"] = to_dev(np.full((1, 7), bias_q[0], np.float32))
            if ip or residual:
                kw.update(extra=None if ip else to_dev(terms), has_extra=True)
            # plain: the values are the row sums; residual: the reference forms them from the row sums, bias and terms
            want = lists_reference(orc.adc_scan(t[:1], codes) if residual else values[:1], allow, off, pr,
                                   np.full((1, 7), bias_q[0], np.float32), 64 * L, ip, residual, None if ip else terms, None)
            for G in (1, 2):
                if order in ("random", "descending"):
                    assert least_wave_share(n, -(-n // G), allow) > 64 * L
                ra.set_option("adc_lists_wgs_per_query", G)
                for k in edge_ks(L):
                    planned = cells.plan(cells.Call(family, True, ip, masked, residual, STEADY_M, STEADY_K, k, 1, 1, 7, G))
                    checked(ra, pq, want, k, planned, name, family, to_dev(t[:1]), dev, words, **kw)
    finally:
        ra.set_option("adc_lists_wgs_per_query", 0)


# ---- the u8 searches do not depend on the grid ---------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_u8_search_grid_independence(ra):
    import torch
    rng = np.random.default_rng(item_seed(7))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, K, n, nq = 15, 256, 9001, 9
    pq = make_pq(ra, M, K)
    codes = draw_codes(rng, n, M, K)
    t = draw_tables(rng, nq, M, K)
    sc = rng.standard_normal(n).astype(np.float32)
    allow = rng.random(n) < 0.5
    s = orc.adc_scan(t, codes)
    td, cd, scd, words = to_dev(t), to_dev(codes), to_dev(sc), mask_words(allow)
    wants = {(False, False): ref_search(s, cells.MAX_K), (True, False): ref_ip_search(scores(s, sc), cells.MAX_K),
             (False, True): ref_masked_search(s, allow, cells.MAX_K), (True, True): ref_masked_search(scores(s, sc), allow, cells.MAX_K, ip=True)}
    try:
        for wgs in (1, 2, 7, cus, 0):
            ra.set_option("adc_search_wgs", wgs)
            for k in (10, 100, 1024):
                for (ip, masked), want in wants.items():
                    planned = cells.plan(cells.Call("u8", False, ip, masked, False, M, K, k, nq, 1, 0, 0))
                    kw = dict(extra=scd, has_extra=True) if ip else {}
                    checked(ra, pq, want, k, planned, "adc_ip_search" if ip else "adc_search", "u8", td, cd, words if masked else None, **kw)
    finally:
        ra.set_option("adc_search_wgs", 0)
