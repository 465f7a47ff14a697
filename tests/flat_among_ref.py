"""Reference of the exact searches among given rows (include/pqhip.h: pqhip_flat_among_f32_dev,
pqhip_flat_range_among_f32_dev) in numpy, from their definition: the places of a query are ids[lims[q] : lims[q + 1]]
(of ids itself without lims) -- lims clamped to [0, n_ids], an inverted range empty --, -1 is padding, any other id
outside [0, n) is skipped and flags; the value of a named row is the one the exact searches define
(rerank_ref.row_values via flat_range_ref.all_values); the top-k orders the candidates by the key of rerank_ref.ref_rerank
(NaN flag, value with -0 == +0, row id); the range keeps the places that pass the IEEE predicate in the order in which
they were named.  Values are kept bit for bit.

Also the chunk arithmetic of the two drivers (pqhip_flat_among.hip), restated from the source in the manner of
query_chunks.py / flat_range_ref.py."""
import re

import numpy as np

import adc_search_cells as cells
import flat_range_ref as frr

DRIVER = "pqhip_flat_among.hip"
OPTION = "flat_among_wgs_per_query"
OPTION_RANGE = "flat_range_among_wgs_per_query"
GRID_Y = 65535
TILE = 16


def places(ids, lims, q, n):
    """(the ids of query q's places that lie in [0, n), in the order named; whether the query raises the range flag)"""
    ids = np.asarray(ids, np.int64)
    flagged = False
    if lims is None:
        mine = ids
    else:
        b, e = int(lims[q]), int(lims[q + 1])
        cb, ce = min(max(b, 0), ids.size), min(max(e, 0), ids.size)
        flagged = cb != b or ce != e or e < b
        mine = ids[cb:ce] if ce > cb else ids[:0]
    inside = (mine >= 0) & (mine < n)
    flagged = flagged or bool((~inside & (mine != -1)).any())
    return mine[inside], flagged


def _values(queries, vectors, ip, values):
    return frr.all_values(queries, vectors, ip) if values is None else values


def ref_flat_among(queries, vectors, ids, k, lims=None, ip=False, values=None):
    """queries [nq, d] (or [d]), vectors [n, d] f32 / f16, ids int64 [n_ids], lims None or [nq + 1] -> (value [nq, k] f32,
    idx [nq, k] int64, flagged).  values: flat_range_ref.all_values(..) if the caller has them."""
    v_all = _values(queries, vectors, ip, values)
    nq, n = v_all.shape[0], np.asarray(vectors).shape[0]
    out_v = np.full((nq, k), -np.inf if ip else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    flagged = False
    for q in range(nq):
        rows, f = places(ids, lims, q, n)
        flagged = flagged or f
        if rows.size == 0:
            continue
        v32 = v_all[q][rows]
        v = v32.astype(np.float64)
        nan = np.isnan(v)
        key = (-1.0 if ip else 1.0) * np.where(nan, 0.0, v) + 0.0        # -0 -> +0; NaN rows ordered by the flag
        order = np.lexsort((rows, key, nan))[:min(k, rows.size)]         # last key is primary
        out_i[q, :order.size] = rows[order]
        out_v[q, :order.size] = v32[order] + np.float32(0.0)             # a zero comes back as +0
    return out_v, out_i, flagged


def ref_flat_range_among(queries, vectors, ids, thr, lims=None, ip=False, values=None):
    """-> (lims [nq + 1], val, idx, flagged): of every query's places those that qualify, in the order named"""
    v_all = _values(queries, vectors, ip, values)
    nq, n = v_all.shape[0], np.asarray(vectors).shape[0]
    t = np.broadcast_to(np.asarray(thr, np.float32).reshape(-1), (nq,)) if np.size(thr) in (1, nq) else None
    assert t is not None
    out_l, vals, idxs = [0], [], []
    flagged = False
    for q in range(nq):
        rows, f = places(ids, lims, q, n)
        flagged = flagged or f
        v = v_all[q][rows] if rows.size else np.zeros(0, np.float32)
        with np.errstate(invalid="ignore"):
            hit = (v >= t[q]) if ip else (v <= t[q])
        vals.append(v[hit])
        idxs.append(rows[hit])
        out_l.append(out_l[-1] + int(hit.sum()))
    return (np.array(out_l, np.int64), np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, np.float32),
            np.concatenate(idxs).astype(np.int64) if idxs else np.zeros(0, np.int64), flagged)


# ---- the query chunks of pqhip_flat_among.hip ---------------------------------------------------------------------------
def src():
    return frr.src(DRIVER)


def constants():
    """read at call time, so that a missing driver fails the test that asks and not the import"""
    return {"scratch": frr.constant("kListsScratchBytes", frr.src("adc_search_launch.h")),
            "scan_max": frr.constant("kFlatAmongScanMax", src()),
            "waves": frr.constant("kRangeWaves", frr.src("kernels_adc_range.hip.h"))}


def grid_caps():
    """the bounds on the two grid options, where the drivers read them: (top-k, range)"""
    text = src()
    caps = []
    for option in (OPTION, OPTION_RANGE):
        m = re.findall(r"%s\.load\(std::memory_order_relaxed\);\s*const int64_t G = forced > 0 \? "
                       r"std::min<int64_t>\(forced, (\d+)\)" % option, text)
        assert len(m) == 1, (option, m)
        caps.append(int(m[0]))
    return tuple(caps)


def topk_chunk(nq, G, k):
    """queries per launch of the top-k call; G: the value of the grid option (> 0)"""
    G = min(G, grid_caps()[0])
    return max(1, min(nq, GRID_Y, constants()["scratch"] // (G * 64 * cells.search_list_regs(k) * 12)))


def bitmap_span(nq, n_ids, shared):
    """the places a query's bitmap has slots for"""
    return n_ids if shared else min(n_ids, 4 * (n_ids // nq) + 1024)


def bitmap_tiles(span, G):
    return -(-(span // TILE + 65 * G + 1) // 4) * 4


def range_chunk(nq, n_ids, G, shared):
    """queries per launch of the range call"""
    c = constants()
    G = min(G, grid_caps()[1])
    per_q = G * c["waves"] * 8 + bitmap_tiles(bitmap_span(nq, n_ids, shared), G) * 2
    return max(1, min(nq, GRID_Y, c["scratch"] // per_q, c["scan_max"] // (G * c["waves"])))
