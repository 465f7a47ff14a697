"""The host policy of the ADC top-k searches restated as a pure planner (numpy-free arithmetic, no library): from a call
(family, M, K, k, nq, code bytes, ...) it returns the kernel instantiations ("cells") the call runs, with the number of
launches of each, and the launch log the library must report.  It mirrors pqhip_adc.hip (search_list_regs,
search_nv_bucket, lists_nv_bucket, search_lds, adc_search_run, adc_search, launch_search_any, adc_search_lists_run),
pqhip_adc_packed4.hip (the packed buckets and routes) and the launchers' names (adc_search_u8_launch.hip.h,
pqhip_adc_packed4.hip, pqhip_adc_packed4_lists.hip).  test_adc_search_cells.py pins the mirrored value lists to the
sources and proves that all_grid_calls(), the calls of test_gpu_adc_search_grid.py, cover every declared cell.

A cell is Cell(family, ip, masked, residual, nv, nq, L, tab_lds):
  family   "u8" / "u8_lists" / "p4" / "p4_lists" (producers), "any_u8" / "any_u32" (generic producer), "merge"
  nv       code dwords fetched per row (0: generic and merge);  nq  queries per pass (0: merge);  L  list registers
  tab_lds  generic producer only: the table in LDS (True) or read through L2 (False); None elsewhere
The packed producers take the mask at run time (one instantiation serves both), so `masked` of a p4 cell says how the
instantiation was called, and both ways are declared."""
import collections
import itertools

Cell = collections.namedtuple("Cell", "family ip masked residual nv nq L tab_lds")
# lists: a list search (n_probe probes, G workgroups per query); code_bytes: 1 or 4 (u8 family), ignored for p4
Call = collections.namedtuple("Call", "family lists ip masked residual M K k nq code_bytes n_probe G")
Plan = collections.namedtuple("Plan", "cells log")            # cells: {Cell: launches}; log: [(kernel name, launches)]

LDS_BYTES = 160 * 1024
MAX_K = 1024                  # kSearchMaxK
ADC_MAX_VALUE_WORDS = 25      # kAdcMaxValueWords
PACKED4_MAX_VALUE_WORDS = 13  # kPacked4MaxValueWords
SEARCH_QUEUE = 32             # kSearchQueue
SEARCH_WAVES = 16             # kSearchWaves
LIST_REGS = (1, 2, 4, 8, 16)                                  # dispatch_list_regs
QUERIES_PER_PASS = (8, 4, 1)                                  # dispatch_queries_per_pass
NV_U8 = (1, 2, 4, 8, 13, ADC_MAX_VALUE_WORDS)                 # search_nv_bucket, launch_search_u8
NV_U8_LISTS = (4, 8, 13, ADC_MAX_VALUE_WORDS)                 # lists_nv_bucket, launch_lists_u8
NV_P4 = (1, 2, 4, 8, PACKED4_MAX_VALUE_WORDS)                 # packed4_nv_bucket, launch_search_packed4
NV_P4_LISTS = (2, 8, PACKED4_MAX_VALUE_WORDS)                 # packed4_lists_nv_bucket, launch_lists_packed4
LISTS_SCRATCH_BYTES = 512 << 20                               # kListsScratchBytes


def _bucket(nv, buckets):
    for b in buckets:
        if nv <= b:
            return b
    return 0


def search_nv_bucket(nv):
    return _bucket(nv, NV_U8)


def lists_nv_bucket(nv):
    return _bucket(nv, NV_U8_LISTS)


def packed4_nv_bucket(nv):
    return _bucket(nv, NV_P4)


def packed4_lists_nv_bucket(nv):
    return _bucket(nv, NV_P4_LISTS)


def u8_words(M):
    return (M + 3) // 4


def packed4_words(M):
    """ceil(ceil(M / 2) / 4): the dwords of a packed row"""
    return ((M + 1) // 2 + 3) // 4


def search_list_regs(k):
    lk = 64
    while lk < k:
        lk <<= 1
    return lk // 64


def search_lds(table_bytes, nq, L):
    """a producer's dynamic LDS: max(table image + queues, combine lists)"""
    queues = SEARCH_WAVES * nq * SEARCH_QUEUE * 2 * 4
    comb = SEARCH_WAVES * nq * 64 * L * 2 * 4
    return max(table_bytes + queues, comb)


def passes(nq, L, table_bytes, multi_query):
    """adc_search_run: [(queries per pass, passes)] in launch order -- 8 / 4 / 1 with NQ L <= 16 and the 160 KB bound"""
    def fits(c):
        return multi_query and c * L <= 16 and search_lds(table_bytes * c, c, L) <= LDS_BYTES
    first = 1
    for c in (8, 4):
        if fits(c) and nq >= c:
            first = c
            break
    out, q = [], 0
    for nqp in QUERIES_PER_PASS:
        if nqp > first or (nqp == 4 and not fits(4)):
            continue
        cnt = (nq - q) // nqp
        if cnt:
            out.append((nqp, cnt))
            q += cnt * nqp
    assert q == nq
    return out


def _mq(nqp):
    return "" if nqp == 1 else "_mq<%d queries>" % nqp


def _log(entries):
    """the library's launch log: a name once, in order of first launch, with its count"""
    out = collections.OrderedDict()
    for name, cnt in entries:
        out[name] = out.get(name, 0) + cnt
    return list(out.items())


def log_text(log):
    """what pqhip_launch_log returns for these launches"""
    return " + ".join(name + (" x%d" % cnt if cnt > 1 else "") for name, cnt in log)


def plan(call):
    """Plan of a call with n > 0 rows (and n_lists > 0), or None when the library answers PQHIP_EUNSUPPORTED."""
    c = call
    assert c.family in ("u8", "p4") and c.k >= 1 and c.nq >= 1
    if c.k > MAX_K:
        return None
    L = search_list_regs(c.k)
    ipn = "ip_" if c.ip else ""
    merge = Cell("merge", c.ip, False, False, 0, 0, L, None)
    merge_name = "k_adc_%ssearch_merge" % ipn
    if c.family == "p4":
        if c.K > 16 or c.M > 100:
            return None
        table = c.M * 16 * 4
        nvb = (packed4_lists_nv_bucket if c.lists else packed4_nv_bucket)(packed4_words(c.M))
    else:
        table = c.M * c.K * 4
        nvb = (lists_nv_bucket if c.lists else search_nv_bucket)(u8_words(c.M))
    if c.lists:
        if c.family == "u8" and (c.code_bytes != 1 or nvb == 0 or search_lds(table, 1, L) > LDS_BYTES):
            return None
        plan_q = (c.n_probe * 2 + 1) * 8
        lists_q = c.G * 64 * L * 12
        chunk = max(1, min(c.nq, 65535, LISTS_SCRATCH_BYTES // (plan_q + lists_q)))
        launches = -(-c.nq // chunk)
        res = "residual_" if c.residual else ""
        if c.family == "p4":
            name = "k_adc_%ssearch_lists_%sp4" % (ipn, res)
        else:
            name = "k_adc_%ssearch_lists_%s%su8" % (ipn, res, "masked_" if c.masked else "")
        cells = {Cell(c.family + "_lists", c.ip, c.masked, c.residual, nvb, 1, L, None): launches, merge: launches}
        return Plan(cells, _log([("k_adc_lists_plan", launches), (name, launches), (merge_name, launches)]))
    assert not c.residual
    cells, entries = {}, []
    if c.family == "p4":
        fast = True
    else:
        if c.code_bytes not in (1, 4):
            return None
        fast = c.code_bytes == 1 and nvb != 0 and search_lds(table, 1, L) <= LDS_BYTES
        if c.masked and not fast:
            return None
    if fast:
        for nqp, cnt in passes(c.nq, L, table, True):
            cells[Cell(c.family, c.ip, c.masked, False, nvb, nqp, L, None)] = cnt
            if c.family == "p4":
                name = "k_adc_%ssearch_p4%s" % (ipn, _mq(nqp))
            else:
                name = "k_adc_%ssearch_%su8%s" % (ipn, "masked_" if c.masked else "", _mq(nqp))
            entries += [(name, cnt), (merge_name, cnt)]
    else:
        tab_lds = search_lds(table, 1, L) <= LDS_BYTES        # launch_search_any, diagnostics off
        cells[Cell("any_u8" if c.code_bytes == 1 else "any_u32", c.ip, False, False, 0, 1, L, tab_lds)] = c.nq
        entries += [("k_adc_%ssearch_%s" % (ipn, "wide" if tab_lds else "any"), c.nq), (merge_name, c.nq)]
    cells[merge] = sum(cnt for name, cnt in entries if name == merge_name)
    return Plan(cells, _log(entries))


# ---- every instantiation the launchers name ------------------------------------------------------------------------
NQ_L_PAIRS = tuple((nq, L) for nq in QUERIES_PER_PASS for L in LIST_REGS if nq * L <= 16)
B2 = (False, True)


def declared_cells():
    cells = set()
    for ip, masked, nv, (nq, L) in itertools.product(B2, B2, NV_U8, NQ_L_PAIRS):
        cells.add(Cell("u8", ip, masked, False, nv, nq, L, None))
    for ip, res, masked, nv, L in itertools.product(B2, B2, B2, NV_U8_LISTS, LIST_REGS):
        cells.add(Cell("u8_lists", ip, masked, res, nv, 1, L, None))
    for ip, masked, nv, (nq, L) in itertools.product(B2, B2, NV_P4, NQ_L_PAIRS):
        cells.add(Cell("p4", ip, masked, False, nv, nq, L, None))
    for ip, res, masked, nv, L in itertools.product(B2, B2, B2, NV_P4_LISTS, LIST_REGS):
        cells.add(Cell("p4_lists", ip, masked, res, nv, 1, L, None))
    for ip, fam, L, tab in itertools.product(B2, ("any_u8", "any_u32"), LIST_REGS, B2):
        cells.add(Cell(fam, ip, False, False, 0, 1, L, tab))
    for ip, L in itertools.product(B2, LIST_REGS):
        cells.add(Cell("merge", ip, False, False, 0, 0, L, None))
    return cells


# ---- the calls of test_gpu_adc_search_grid.py ----------------------------------------------------------------------
U8_MS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 52, 53, 100)           # first and last M of every bucket of NV_U8
P4_MS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 100)                 # first and last M of every bucket of NV_P4
GRID_KS = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)      # both edges of every L
UPPER_KS = (64, 128, 256, 512, 1024)
GRID_NQ = 13
GRID_N = 2077
GRID_WGS = 2
FULL_SCAN = (700, 1024)                                        # (n, k): every row comes back, then the padding
LISTS_N_PROBE = 10                                             # 9 lists, all probed, and one -1
LISTS_G = 2
# (code bytes, M, K): the generic producer with its table in LDS and through L2
GENERIC_SHAPES = ((1, 101, 4), (1, 160, 256), (4, 15, 1024), (4, 15, 4096))


def small_k(M):
    """a codebook size with M K <= 4,096 that is no power of two, at most 77 (8 tables fit LDS up to M = 53)"""
    K = min(77, 4096 // M)
    return K - 1 if K & (K - 1) == 0 else K


def codebook_sizes(family, M):
    return (13,) if family == "p4" else (small_k(M), 256)


def grid_calls(family, lists, ip, masked, residual, M):
    """the calls of one test item: every K of the width, every k"""
    out = []
    for K in codebook_sizes(family, M):
        for k in GRID_KS:
            out.append(Call(family, lists, ip, masked, residual, M, K, k, GRID_NQ, 1,
                            LISTS_N_PROBE if lists else 0, LISTS_G if lists else 0))
    return out


def generic_calls(ip):
    return [Call("u8", False, ip, False, False, M, K, k, 2, cb, 0, 0) for cb, M, K in GENERIC_SHAPES for k in UPPER_KS]


def grid_items():
    """(family, lists, ip, masked, residual, M) of every parametrised item of the grid tests"""
    out = []
    for family, ms in (("u8", U8_MS), ("p4", P4_MS)):
        for ip, masked, M in itertools.product(B2, B2, ms):
            out.append((family, False, ip, masked, False, M))
        for ip, residual, masked, M in itertools.product(B2, B2, B2, ms):
            out.append((family, True, ip, masked, residual, M))
    return out


def all_grid_calls():
    calls = []
    for item in grid_items():
        calls += grid_calls(*item)
    for ip in B2:
        calls += generic_calls(ip)
    return calls
