"""The merge of search results (Pq.merge_topk_device) and the searches of a MatrixGroup against what a caller has
without them, in one process, HIP events, on ONE device (nothing here has been measured on more than one GPU).

(a) The merge call alone: n_queries in {1, 64, 1024}, P in {2, 8} parts, k = k_in in {10, 100, 1024}, every part's row
    full and sorted.  Per cell, 3 warm-up rounds, then 9 timed batches of 20 calls each, the median batch / 20 and the spread:
      merge   pq.merge_topk_device(vals, ids, k, offsets=bases)
      torch   cat of the parts along k (values and ids + bases), stable sort by value, gather, slice to k -- the only
              merge a caller has today; it does not honour the library's order (-0 / +0, NaN, ties by part)
    Values are random normals, so the two agree on them; the cell records that they did.
(b) nearest() and most_similar() of a group of P in {2, 8} equal parts (views of the one matrix's rows) of a matrix of
    100 M rows (d = 300, M = 15, K = 256), 8 and 1,024 queries, k in {10, 100}, against the same search on the one matrix:
    1 warm-up, median of 5.  The group's result is compared with the one matrix's, bit for bit, before it is timed.

Writes JSON (default profiles/results_merge_time.json) and prints the tables of DESIGN.md.  Ratios are recorded as they come
out, cells where the merge loses to torch or where splitting costs time included.

usage: python tools/results_merge_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402
from reductive_amd import qmatrix  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "results_merge_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
D, M, K = 300, 15, 256


def timed(fn, warm, reps, inner=1):
    """median and all of `reps` timings of `inner` calls each, in ms per call"""
    for _ in range(warm * inner):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts)), [round(t, 5) for t in ts]


def torch_merge(vals, gids, k):
    """what a caller does today: gids = ids + bases, formed once outside"""
    P, nq, k_in = vals.shape
    v = vals.permute(1, 0, 2).reshape(nq, P * k_in)
    i = gids.permute(1, 0, 2).reshape(nq, P * k_in)
    s = torch.sort(v, dim=1, stable=True)
    return s.values[:, :k], torch.gather(i, 1, s.indices[:, :k])


def flat(pq, codes, norms):
    """a QuantizedMatrix around device tensors (its constructor takes host arrays)"""
    m = object.__new__(qmatrix.QuantizedMatrix)
    m.pq, m.codes, m.norms = pq, codes, norms
    return m


def same(a, b):
    return all(bool(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                y.view(torch.int32) if y.dtype == torch.float32 else y)) for x, y in zip(a, b))


def main():
    rng = np.random.default_rng(41)
    pq = ra.Pq(None, rng.standard_normal((M, K, D // M), dtype=np.float32))
    res = {"device": torch.cuda.get_device_name(0), "devices_used": 1,
           "note": "one GPU: nothing here has been measured on more than one device",
           "merge": {"warmup_rounds": 3, "reps": 9, "calls_per_rep": 20, "cells": []},
           "group": {"shape": {"n": N, "d": D, "M": M, "K": K}, "warmup": 1, "reps": 5, "cells": []}}
    g = torch.Generator(device="cuda").manual_seed(5)
    for nq in (1, 64, 1024):
        for P in (2, 8):
            for k in (10, 100, 1024):
                vals = torch.sort(torch.randn((P, nq, k), device="cuda", generator=g), dim=2).values
                ids = torch.randint(0, 1 << 30, (P, nq, k), device="cuda", generator=g)
                bases = torch.arange(P, device="cuda", dtype=torch.int64) << 32
                gids = ids + bases[:, None, None]
                ra.launch_log(reset=True)
                got = pq.merge_topk_device(vals, ids, k, offsets=bases)
                log = ra.launch_log(reset=True)
                agree = same(got, torch_merge(vals, gids, k))
                merge_ms, merge_all = timed(lambda: pq.merge_topk_device(vals, ids, k, offsets=bases), 3, 9, 20)
                torch_ms, torch_all = timed(lambda: torch_merge(vals, gids, k), 3, 9, 20)
                row = {"n_queries": nq, "parts": P, "k": k, "agrees_with_torch_on_random_values": agree,
                       "merge_us": round(merge_ms * 1e3, 2), "torch_us": round(torch_ms * 1e3, 2),
                       "merge_over_torch": round(merge_ms / torch_ms, 3),
                       "merge_us_min_max": [round(min(merge_all) * 1e3, 2), round(max(merge_all) * 1e3, 2)],
                       "torch_us_min_max": [round(min(torch_all) * 1e3, 2), round(max(torch_all) * 1e3, 2)], "launches": log}
                print(json.dumps(row), flush=True)
                res["merge"]["cells"].append(row)

    codes = torch.randint(0, 256, (N, M), dtype=torch.uint8, device="cuda", generator=g)
    norms = torch.rand(N, device="cuda", generator=g) + 0.5
    whole = flat(pq, codes, norms)
    for P in (2, 8):
        cuts = [N * p // P for p in range(P + 1)]
        group = ra.MatrixGroup([flat(pq, codes[a:b], norms[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
        for nq in (8, 1024):
            q = torch.randn((nq, D), device="cuda", generator=g)
            for fn in ("nearest", "most_similar"):
                for k in (10, 100):
                    one, many = getattr(whole, fn), getattr(group, fn)
                    ok = same(many(q, k), one(q, k))
                    group_ms, group_all = timed(lambda: many(q, k), 1, 5)
                    whole_ms, whole_all = timed(lambda: one(q, k), 1, 5)
                    row = {"search": fn, "parts": P, "n_queries": nq, "k": k, "same_as_one_matrix": ok,
                           "group_ms": round(group_ms, 3), "one_matrix_ms": round(whole_ms, 3),
                           "group_over_one_matrix": round(group_ms / whole_ms, 3),
                           "all_ms": {"group": group_all, "one_matrix": whole_all}}
                    print(json.dumps(row), flush=True)
                    res["group"]["cells"].append(row)
    res["merge_slower_than_torch"] = [[r["n_queries"], r["parts"], r["k"]] for r in res["merge"]["cells"] if r["merge_over_torch"] > 1]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print("| queries | parts | k | merge us | torch us | merge / torch |")
    print("|---|---|---|---|---|---|")
    for r in res["merge"]["cells"]:
        print("| %d | %d | %d | %.1f | %.1f | %.2f |" % (r["n_queries"], r["parts"], r["k"], r["merge_us"], r["torch_us"], r["merge_over_torch"]))
    print("| search | parts | queries | k | group ms | one matrix ms | group / one |")
    print("|---|---|---|---|---|---|---|")
    for r in res["group"]["cells"]:
        print("| %s | %d | %d | %d | %.2f | %.2f | %.2f |" % (r["search"], r["parts"], r["n_queries"], r["k"], r["group_ms"],
                                                             r["one_matrix_ms"], r["group_over_one_matrix"]))
    assert all(r["same_as_one_matrix"] for r in res["group"]["cells"]), "a group's search differs from the one matrix's"


if __name__ == "__main__":
    main()
