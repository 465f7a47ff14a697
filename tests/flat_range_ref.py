"""Reference of the exact range searches over resident vectors (include/pqhip.h: pqhip_flat_range_f32_dev,
pqhip_flat_range_lists_f32_dev) in numpy, from their definition: the value of every row is the one the exact searches
define (rerank_ref.row_values: 64 lane chains from +0, then the fixed tree), the predicate, the order and the CSR output
are those of the ADC range searches (adc_range_ref.ref_range / ref_range_lists).  Values are kept bit for bit.

Also the chunk arithmetic of the list driver (pqhip_flat_range.hip), restated from its source in the manner of
query_chunks.py: a chunk of queries is bounded by gridDim.y, by the scratch of plan, partial counts and hit bitmap, and
by what one prefix scan sums."""
import os
import re

import numpy as np

import adc_range_ref as arr
import rerank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reductive_amd", "csrc")
DRIVER = "pqhip_flat_range.hip"


def all_values(queries, vectors, ip=False):
    """[nq, n] f32: the value of every row for every query"""
    q2 = np.atleast_2d(np.asarray(queries, np.float32))
    x = np.asarray(vectors)
    if x.shape[0] == 0:
        return np.zeros((q2.shape[0], 0), np.float32)
    return np.stack([rr.row_values(q, x, ip=ip) for q in q2])


def ref_flat_range(queries, vectors, thr, ip=False, allow=None, values=None):
    """queries [nq, d] (or [d]), vectors [n, d] f32 / f16, thr a scalar or [nq], allow None or bool [n] -> CSR (lims, val,
    idx), the qualifying rows of each query in ascending row index.  values: all_values(..) if the caller has them."""
    v = all_values(queries, vectors, ip) if values is None else values
    return arr.ref_range(v, thr, ip=ip, allow=allow)


def ref_flat_range_lists(queries, vectors, list_off, probes, thr, ip=False, allow=None, values=None):
    """vectors in list order under list_off [n_lists + 1], probes [nq, n_probe], allow in position order -> CSR, idx =
    positions, in the order of the concatenation of the probed lists"""
    v = all_values(queries, vectors, ip) if values is None else values
    return arr.ref_range_lists(v, list_off, probes, thr, ip=ip, allow=allow)


# ---- the query chunks of pqhip_flat_range_lists_f32_dev ---------------------------------------------------------------
def src(name=DRIVER):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(name, text):
    """the value of `constexpr <type> name = <integer expression>;`: literals (a u suffix allowed), << and *"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9u<*\s]+);" % name, text)
    assert m, name
    return int(eval(re.sub(r"(\d)u", r"\1", m.group(1)), {"__builtins__": {}}))


GRID_Y = 65535                      # gridDim.y
TILE = 16                           # kFlatTile
OPTION_LISTS = "flat_range_wgs_per_query"
OPTION = "flat_range_wgs"


def constants():
    """read at call time, so that a missing driver fails the test that asks and not the import"""
    return {"scratch": constant("kListsScratchBytes", src("adc_search_launch.h")),
            "scan_max": constant("kFlatRangeScanMax", src()),
            "waves": constant("kRangeWaves", src("kernels_adc_range.hip.h")),
            "queries": constant("kFlatRangeQueries", src())}


def lists_grid_cap():
    caps = re.findall(r"flat_range_wgs_per_query\.load\(std::memory_order_relaxed\);\s*const int64_t G = forced > 0 \? "
                      r"std::min<int64_t>\(forced, (\d+)\)", src())
    assert len(caps) == 1, caps
    return int(caps[0])


def grid_cap():
    """the bound on "flat_range_wgs": one scan sums the counts of a pass of kFlatRangeQueries queries"""
    c = constants()
    assert "std::min<int64_t>(forced, kFlatRangeScanMax / (kFlatRangeQueries * kRangeWaves))" in src()
    return c["scan_max"] // (c["queries"] * c["waves"])


def bitmap_tiles(n, G):
    return -(-(n // TILE + 65 * G + 1) // 4) * 4


def lists_query_bytes(n, G, n_probe):
    """scratch one query of a chunk takes; G after the cap"""
    c = constants()
    return (n_probe * 2 + 1) * 8 + G * c["waves"] * 8 + bitmap_tiles(n, G) * 2


def lists_chunk(nq, n, G, n_probe):
    """queries per launch of the list call; G: the value of the grid option (> 0)"""
    c = constants()
    G = min(G, lists_grid_cap())
    return max(1, min(nq, GRID_Y, c["scratch"] // lists_query_bytes(n, G, n_probe), c["scan_max"] // (G * c["waves"])))


def used_tiles(total, G, waves=16):
    """tile slots the 16 G units of a query with `total` probed places use: what bitmap_tiles must cover for total <= n"""
    per = -(-total // G)
    sub = -(-(-(-per // waves)) // 64) * 64
    return G * waves * (sub // TILE)
