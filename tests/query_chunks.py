"""The query loops of the search drivers restated as arithmetic (no GPU, no torch, no library): every search that gives
each query its own workgroups launches per chunk of queries, a chunk bounded by the 65,535 of gridDim.y and by a scratch
budget, and offsets the caller's pointers by the first query of the chunk.  Five drivers have the loop:
  "lists"        adc_search_lists_run (pqhip_adc.hip): every ADC list search, u8 and packed4
  "flat_lists"   pqhip_flat_search_lists_f32_dev (pqhip_flat_search_lists.hip)
  "among"        adc_among (pqhip_adc_among.hip)
  "range_lists"  adc_range_lists (pqhip_adc_range.hip)
  "rerank"       pqhip_rerank_f32_dev (pqhip_rerank.hip)
and search_padding_only (pqhip_adc.hip) has it for calls with no row to search ("padding").
chunk() gives the chunk of a call, CASES the calls of test_gpu_query_chunks.py with the launches each needs and log()
the launch log the library must report for them.  The constants are read from the sources; test_query_chunks.py pins the
chunk expressions to the sources and proves that every case enters the third iteration with a shorter last chunk."""
import collections
import os
import re

import adc_search_cells as cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reductive_amd", "csrc")
DRIVER_FILES = {"lists": "pqhip_adc.hip", "flat_lists": "pqhip_flat_search_lists.hip", "among": "pqhip_adc_among.hip",
                "range_lists": "pqhip_adc_range.hip", "rerank": "pqhip_rerank.hip"}
OPTIONS = {"lists": "adc_lists_wgs_per_query", "flat_lists": "flat_lists_wgs_per_query", "among": "adc_among_wgs_per_query",
           "range_lists": "adc_range_wgs_per_query", "rerank": "rerank_wgs_per_query"}


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(name, text):
    """the value of `constexpr <type> name = <integer expression>;`: literals (a u suffix allowed), << and *"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9u<*\s]+);" % name, text)
    assert m, name
    return int(eval(re.sub(r"(\d)u", r"\1", m.group(1)), {"__builtins__": {}}))


def grid_cap(driver):
    """the bound on the forced number of workgroups per query, where the driver reads its option"""
    caps = re.findall(r"forced > 0 \? std::min<int64_t>\(forced, (\d+)\)", src(DRIVER_FILES[driver]))
    assert len(caps) == 1, (driver, caps)         # (the exhaustive range call bounds its option by an expression)
    return int(caps[0])


LISTS_SCRATCH_BYTES = constant("kListsScratchBytes", src("adc_search_launch.h"))
RERANK_SCRATCH_BYTES = constant("kRerankScratchBytes", src("pqhip_rerank.hip"))
RANGE_SCAN_MAX = constant("kRangeScanMax", src("pqhip_adc_range.hip"))
RANGE_WAVES = constant("kRangeWaves", src("kernels_adc_range.hip.h"))
RERANK_MAX_CAND = constant("kRerankMaxCand", src("kernels_rerank.hip.h"))
GRID_CAPS = {d: grid_cap(d) for d in DRIVER_FILES}
GRID_Y = 65535                                    # gridDim.y


def query_bytes(driver, G, k, n_probe, n_cand):
    """scratch one query of a chunk takes; G: the workgroups per query after the cap"""
    L = cells.search_list_regs(k)
    plan_q = (n_probe * 2 + 1) * 8
    if driver in ("lists", "flat_lists"):
        return plan_q + G * 64 * L * 12
    if driver == "among":
        return G * 64 * L * 12
    if driver == "range_lists":
        return plan_q + G * RANGE_WAVES * 8
    if driver == "rerank":
        return n_cand * 8
    raise ValueError(driver)


def chunk(driver, nq, G, k, n_probe=0, n_cand=0):
    """queries per launch; G: the value of the driver's grid option (> 0), capped as the driver caps it"""
    assert nq >= 1 and G >= 1
    if driver == "padding":
        return min(nq, GRID_Y)
    G = min(G, GRID_CAPS[driver])
    if driver == "rerank":
        return min(nq, GRID_Y, RERANK_SCRATCH_BYTES // query_bytes(driver, G, k, n_probe, n_cand))
    bounds = [nq, GRID_Y, LISTS_SCRATCH_BYTES // query_bytes(driver, G, k, n_probe, n_cand)]
    if driver == "range_lists":
        bounds.append(RANGE_SCAN_MAX // (G * RANGE_WAVES))
    return max(1, min(bounds))


def launches(driver, nq, G, k, n_probe=0, n_cand=0):
    return -(-nq // chunk(driver, nq, G, k, n_probe, n_cand))


def leased_bytes(case):
    if case.driver == "padding":
        return 0
    G = min(case.G, GRID_CAPS[case.driver])
    return case.chunk * query_bytes(case.driver, G, case.k, case.n_probe, case.n_cand)


# ---- the calls of test_gpu_query_chunks.py -------------------------------------------------------------------------
PERIOD = 7                      # route Y and rerank: query i is pattern i mod PERIOD
M, K_U8, K_P4 = 4, 16, 13       # the codebooks of the ADC calls
D = 20                          # width of the vectors of flat lists and rerank
N_ROWS = 300                    # rows of every matrix but the two below
N_ROWS_RANGE = 120              # the range calls: every query may return every row
N_ROWS_RERANK_S = 1200          # rerank, route S: 1,024 distinct candidates per query
N_LISTS, N_PROBE = 9, 3
P_RS, B_RS = 5, 4               # row strides of the probe and bias matrices (distinct, and neither is N_PROBE)
AMONG_MAX_IDS = 40              # ids per query of the per-query ranges
AMONG_B_RS = N_LISTS + 2        # row stride of the bias matrix of the residual search among rows
PAD = 3                         # output row strides k + PAD
PADDING_K = 2
SCRATCH_LIMIT = {"lists": 512 << 20, "flat_lists": 512 << 20, "among": 512 << 20, "range_lists": 512 << 20, "rerank": 64 << 20,
                 "padding": 0}
IO_LIMIT = 256 * 1000 * 1000

ITEMS = {"lists": ("l2", "ip_scaled", "masked", "residual", "packed4"),
         "flat_lists": ("l2_f32", "ip_f16", "masked"),
         "among": ("lims", "shared", "residual"),
         "range_lists": ("l2", "residual_ip_scaled"),
         "rerank": ("l2_f32", "ip_f16"),
         "padding": ("lists", "among", "flat_lists", "exhaustive")}

# period: the distinct (query, probe row, bias row, threshold, candidate row) patterns; chunk, launches: what the model says
Case = collections.namedtuple("Case", "driver item route nq period G k n_probe n_cand n chunk launches")

MANY = 1 << 40                  # more queries than any bound: chunk(driver, MANY, ...) is the bound itself


def _case(driver, item, route, G, k, n_cand, n, rest, periodic):
    n_probe = N_PROBE if driver in ("lists", "flat_lists", "range_lists", "padding") else 0
    c = chunk(driver, MANY, G, k, n_probe, n_cand)
    nq = 2 * c + rest
    return Case(driver, item, route, nq, PERIOD if periodic else nq, G, k, n_probe, n_cand, n, chunk(driver, nq, G, k, n_probe, n_cand),
                launches(driver, nq, G, k, n_probe, n_cand))


def _cases():
    out = []
    for driver in ("lists", "flat_lists", "among", "range_lists", "rerank"):
        cap = GRID_CAPS[driver]
        n = N_ROWS_RANGE if driver == "range_lists" else N_ROWS
        for item in ITEMS[driver]:
            if driver == "rerank":
                out.append(_case(driver, item, "S", cap, 5, RERANK_MAX_CAND, N_ROWS_RERANK_S, 5, True))
                out.append(_case(driver, item, "Y", 1, 3, 2, n, 5, True))
            else:
                out.append(_case(driver, item, "S", cap, cells.MAX_K, 0, n, 3 if driver != "range_lists" else 5, False))
                out.append(_case(driver, item, "Y", 1, 3, 0, n, 5, True))
    for item in ITEMS["padding"]:
        out.append(_case("padding", item, "Y", 1, PADDING_K, 0, 0, 5, True))
    return out


CASES = _cases()


def case(driver, item, route):
    found = [c for c in CASES if (c.driver, c.item, c.route) == (driver, item, route)]
    assert len(found) == 1, (driver, item, route)
    return found[0]


def case_ids(driver):
    return [(c.item, c.route) for c in CASES if c.driver == driver]


def io_bytes(c):
    """device inputs plus outputs of a case's largest call, from above: the matrices as the test lays them out, and for a
    range call every row of every query"""
    tables = c.nq * M * K_U8 * 4
    probes = c.nq * P_RS * 8
    topk = (c.nq * (c.k + PAD) + 2 * PAD) * 12
    if c.driver == "lists":
        return tables + probes + c.nq * B_RS * 4 + topk + c.n * (M + 4 + 4) + c.n // 8 + 4 + (N_LISTS + 1) * 8
    if c.driver == "flat_lists":
        return c.nq * (D + 3) * 4 + c.nq * (c.n_probe + 2) * 8 + topk + c.n * D * 4 + c.n // 8 + 4 + (N_LISTS + 1) * 8
    if c.driver == "among":
        return tables + (c.nq + 1) * 8 + c.nq * AMONG_MAX_IDS * 8 + c.nq * AMONG_B_RS * 4 + topk + c.n * (M + 8 + 4)
    if c.driver == "range_lists":
        return tables + probes + c.nq * B_RS * 4 + c.nq * 4 + (c.nq + 3) * 8 + c.nq * c.n * 12 + c.n * (M + 4) + (N_LISTS + 1) * 8
    if c.driver == "rerank":
        return c.nq * (D + 3) * 4 + c.nq * max(c.n_cand, 4) * 8 + topk + c.n * D * 4
    if c.driver == "padding":
        return max(tables, c.nq * (D + 3) * 4) + probes + topk
    raise ValueError(c.driver)


def _x(n):
    return " x%d" % n if n > 1 else ""


def log(c, ip=False, count_only=False):
    """what pqhip_launch_log returns after the case's call; item names the variant (ITEMS)"""
    n = c.launches
    ipn = "ip_" if ip else ""
    merge = "k_adc_%ssearch_merge%s" % (ipn, _x(n))
    if c.driver == "padding":
        return merge
    if c.driver == "lists":
        call = cells.Call("p4" if c.item == "packed4" else "u8", True, ip, c.item == "masked", c.item == "residual", M,
                          K_P4 if c.item == "packed4" else K_U8, c.k, c.nq, 1, c.n_probe, c.G)
        planned = cells.plan(call)
        assert planned is not None and all(cnt == n for name, cnt in planned.log), (planned, n)     # the two models agree
        return cells.log_text(planned.log)
    if c.driver == "flat_lists":
        return "k_adc_lists_plan%s + k_flat_%ssearch_lists%s + %s" % (_x(n), ipn, _x(n), merge)
    if c.driver == "among":
        return "k_adc_%samong_%su8%s + %s" % (ipn, "residual_" if c.item == "residual" else "", _x(n), merge)
    if c.driver == "range_lists":
        kern = "k_adc_%srange_lists_%su8" % (ipn, "residual_" if c.item.startswith("residual") else "")
        return "k_adc_lists_plan%s + %s%s + k_adc_range_scan%s" % (_x(n), kern, _x(n if count_only else 2 * n), _x(n))
    if c.driver == "rerank":
        return "k_rerank_dist%s + k_rerank_select%s" % (_x(n), _x(n))
    raise ValueError(c.driver)
