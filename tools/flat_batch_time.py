"""Exact search for query batches (Pq.flat_search_batch_device, Pq.flat_range_batch_device: matrix-core screen, exact
resolve) against the unchanged plain calls and against torch's matmul + topk, in one process on the same buffers, on one
MI355X.

10 M standard-normal rows of d = 300, f32 and f16; nq in {8, 16, 32, 64, 256, 1,024} queries; squared L2.  HIP events
around the call, median of 5 after 2 warm-up calls (3 after 1 where one call takes more than a second; the cell says so).
Every cell is compared bit for bit with the plain call before it is timed.
    top-k   k in {10, 100, 1,024}: flat_search_batch_device (x_exp given, as FlatMatrix caches it) against
            plain    flat_search_device
            torch    ||x||^2 (precomputed outside the timing) - 2 q x^T per chunk of 1 M rows in the rows' dtype, topk per
                     chunk, topk of the chunks' results: another rounding, so another result -- timed, not compared
    range   one selective radius per query (its 50th nearest row): flat_range_batch_device against flat_range_device
Each batch cell also records its stages, timed separately with the same protocol: sample (flat_among_device over the
sample), count (the screen as a count call), fill (the screen with its result's capacity, less the count), resolve
(flat_among_device resp. flat_range_among_device over the candidates), and the candidates per query.
"crossover" is the smallest nq from which the batch route wins a k by more than the larger spread of the two; a cell
where it loses is listed under "findings".

Writes JSON (default profiles/flat_batch_time.json).

usage: python tools/flat_batch_time.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_batch_time.json")
N, D = 10_000_000, 300
FORMS = ((torch.float32, "f32"), (torch.float16, "f16"))
NQS, KS = (8, 16, 32, 64, 256, 1024), (10, 100, 1024)
RANGE_RANK = 50
CHUNK = 1_000_000


def timed(fn):
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    slow = time.time() - t0 > 1.0
    warm, reps = (0, 3) if slow else (1, 5)        # the call above was the first warm-up
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def same(a, b):
    return all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
               for s, t in zip(a, b))


def torch_topk(q, x, xx, k):
    qx = q.to(x.dtype)
    vals, idxs = [], []
    for r0 in range(0, N, CHUNK):
        dist = torch.addmm(xx[r0:r0 + CHUNK][None].to(x.dtype), qx, x[r0:r0 + CHUNK].T, alpha=-2.0)
        v, i = torch.topk(dist, k, dim=1, largest=False)
        vals.append(v)
        idxs.append(i + r0)
    v, j = torch.topk(torch.cat(vals, 1), k, dim=1, largest=False)
    return v, torch.gather(torch.cat(idxs, 1), 1, j)


def stages(pq, q, x, k, x_exp, thr=None):
    """the stages of one batch call, each timed on its own; thr given: the range composition (no sample)"""
    out = {}
    nq = q.shape[0]
    if thr is None:
        S, t = rules.flat_batch_sample(N, k)
        ids = torch.arange(0, N, t, dtype=torch.int64, device="cuda")
        out["sample_ms"], _ = timed(lambda: pq.flat_among_device(q, x, ids, k))
        thr = pq.flat_among_device(q, x, ids, k)[0][:, k - 1].contiguous()
        out["sample_rows"] = int(ids.shape[0])
    out["count_ms"], _ = timed(lambda: pq._flat_screen(q, x, thr, False, None, x_exp, 0, None, False))
    lims, cand, total = pq._flat_screen(q, x, thr, False, None, x_exp, 0, None, True)
    both, _ = timed(lambda: pq._flat_screen(q, x, thr, False, None, x_exp, total, None, False))
    out["fill_ms"] = both - out["count_ms"]
    if k is not None:
        out["resolve_ms"], _ = timed(lambda: pq.flat_among_device(q, x, cand, k, lims=lims))
    else:
        out["resolve_ms"], _ = timed(lambda: pq.flat_range_among_device(q, x, cand, thr, lims=lims))
    out["candidates_per_query"] = total / nq
    return {a: (round(b, 4) if isinstance(b, float) else b) for a, b in out.items()}


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "d": D, "protocol": "HIP events, median of 5 after 2 warm-up calls "
           "(3 after 1 when a call takes more than a second)", "topk": [], "range": [], "crossover": {}, "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    pq = ra.Pq(None, np.zeros((1, 1, D), np.float32))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(53)
    qs = torch.randn((max(NQS), D), device="cuda", generator=gen)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for dtype, form in FORMS:
        x = torch.empty((N, D), dtype=dtype, device="cuda")
        for r0 in range(0, N, CHUNK):
            x[r0:r0 + CHUNK] = torch.randn((CHUNK, D), device="cuda", generator=gen).to(dtype)
        xx = torch.cat([(x[r0:r0 + CHUNK].float() ** 2).sum(1) for r0 in range(0, N, CHUNK)])
        x_exp = rules.flat_screen_x_exp(rules._matrix_max_abs(x))
        for k in KS:
            wins = []
            for nq in NQS:
                q = qs[:nq].contiguous()
                want = pq.flat_search_device(q, x, k)
                st = {}
                got = pq.flat_search_batch_device(q, x, k, x_exp=x_exp, stats=st)
                cell = {"form": form, "nq": nq, "k": k, "equal": same(got, want), "x_exp": x_exp,
                        "fallback_queries": st["fallback_queries"]}
                assert cell["equal"], cell
                cell["batch_ms"], cell["batch_all"] = timed(lambda: pq.flat_search_batch_device(q, x, k, x_exp=x_exp))
                cell["plain_ms"], cell["plain_all"] = timed(lambda: pq.flat_search_device(q, x, k))
                cell["torch_ms"], cell["torch_all"] = timed(lambda: torch_topk(q, x, xx, k))
                cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
                cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
                cell["batch_over_torch"] = round(cell["batch_ms"] / cell["torch_ms"], 4)
                cell["stages"] = stages(pq, q, x, k, x_exp)
                won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
                wins.append(won)
                if not won:
                    res["findings"].append("top-k %s nq=%d k=%d: batch %.3f ms, plain %.3f ms" % (form, nq, k, cell["batch_ms"], cell["plain_ms"]))
                res["topk"].append(cell)
                save()
                print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
            first = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
            res["crossover"]["%s k=%d" % (form, k)] = first
        for nq in NQS:
            q = qs[:nq].contiguous()
            thr = pq.flat_search_batch_device(q, x, RANGE_RANK, x_exp=x_exp)[0][:, RANGE_RANK - 1].contiguous()
            want = pq.flat_range_device(q, x, thr)
            got = pq.flat_range_batch_device(q, x, thr, x_exp=x_exp)
            cell = {"form": form, "nq": nq, "rank": RANGE_RANK, "equal": same(got, want), "results": int(want[0][-1])}
            assert cell["equal"], cell
            cell["batch_ms"], cell["batch_all"] = timed(lambda: pq.flat_range_batch_device(q, x, thr, x_exp=x_exp))
            cell["plain_ms"], cell["plain_all"] = timed(lambda: pq.flat_range_device(q, x, thr))
            cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
            cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
            cell["stages"] = stages(pq, q, x, None, x_exp, thr)
            if not cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]:
                res["findings"].append("range %s nq=%d: batch %.3f ms, plain %.3f ms" % (form, nq, cell["batch_ms"], cell["plain_ms"]))
            res["range"].append(cell)
            save()
            print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
        del x, xx
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
