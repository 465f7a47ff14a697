"""Exact search in probed lists for query batches (Pq.flat_search_lists_batch_device, Pq.flat_range_lists_batch_device:
matrix-core screen per list, exact resolve) against the unchanged plain list calls, in one process on the same buffers,
alternating, on one MI355X.

10 M standard-normal rows of d = 300 in 1,024 lists of multinomial lengths, f32 and f16; nq in {8, 16, 32, 64, 256,
1,024}; nprobe 8 and 64 (lists drawn without repetition, as tools/flat_lists_time.py draws them); squared L2.  HIP
events around the call, median of 5 after 2 warm-up calls.  Every cell is compared bit for bit with the plain call before it is timed.
    top-k   k in {10, 100}: flat_search_lists_batch_device (x_exp given, as PartitionedFlatMatrix caches it) against
            flat_search_lists_device
    range   one selective radius per query (its 50th nearest probed row): flat_range_lists_batch_device against
            flat_range_lists_device
"crossover" is the smallest nq from which the batch route wins a column by more than the larger spread of the two for
every larger nq; a cell where it loses is listed under "findings".

Writes JSON (default profiles/flat_lists_batch_time.json).

usage: python tools/flat_lists_batch_time.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_lists_batch_time.json")
N, D, LISTS = 10_000_000, 300, 1024
FORMS = ((torch.float32, "f32"), (torch.float16, "f16"))
NQS, KS, NPROBES = (8, 16, 32, 64, 256, 1024), (10, 100), (8, 64)
RANGE_RANK = 50
CHUNK = 1_000_000


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
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


def compare(res, kind, cell, batch, plain):
    """equality first, then the two routes alternating; the cell is recorded and printed"""
    cell["equal"] = same(batch(), plain())
    assert cell["equal"], cell
    cell["batch_ms"], cell["batch_all"] = timed(batch)
    cell["plain_ms"], cell["plain_all"] = timed(plain)
    cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
    cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
    won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
    if not won:
        res["findings"].append("%s %s: batch %.3f ms, plain %.3f ms" % (kind, {a: cell[a] for a in ("form", "nq", "nprobe", "k") if a in cell},
                                                                        cell["batch_ms"], cell["plain_ms"]))
    res[kind].append(cell)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
    return won


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "d": D, "lists": LISTS,
           "protocol": "HIP events, median of 5 after 2 warm-up calls, batch and plain route in the same run", "topk": [], "range": [],
           "crossover": {}, "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    pq = ra.Pq(None, np.zeros((1, 1, D), np.float32))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(59)
    qs = torch.randn((max(NQS), D), device="cuda", generator=gen)
    x32 = torch.empty((N, D), device="cuda")
    for r0 in range(0, N, CHUNK):
        x32[r0:r0 + CHUNK] = torch.randn((CHUNK, D), device="cuda", generator=gen)
    rng = np.random.default_rng(59)                 # lists and probes as tools/flat_lists_time.py draws them
    lens = np.zeros(LISTS + 1, np.int64)
    np.cumsum(rng.multinomial(N, np.full(LISTS, 1.0 / LISTS)), out=lens[1:])
    off = torch.from_numpy(lens).cuda()
    near = torch.from_numpy(np.stack([rng.permutation(LISTS)[:max(NPROBES)] for _ in range(max(NQS))]).astype(np.int64)).cuda()
    for dtype, form in FORMS:
        x = x32 if dtype == torch.float32 else x32.to(dtype)
        x_exp = rules.flat_screen_x_exp(rules._matrix_max_abs(x))
        for nprobe in NPROBES:
            for k in KS:
                wins = []
                for nq in NQS:
                    q, pr = qs[:nq].contiguous(), near[:nq, :nprobe].contiguous()
                    st = {}
                    pq.flat_search_lists_batch_device(q, x, off, pr, k, x_exp=x_exp, stats=st)
                    cell = {"form": form, "nq": nq, "nprobe": nprobe, "k": k, "fallback_queries": st["fallback_queries"],
                            "candidates_per_query": round(st["candidates"] / nq, 1), "sample_slots": st["sample_slots"]}
                    wins.append(compare(res, "topk", cell, lambda: pq.flat_search_lists_batch_device(q, x, off, pr, k, x_exp=x_exp),
                                        lambda: pq.flat_search_lists_device(q, x, off, pr, k)))
                res["crossover"]["%s nprobe=%d k=%d" % (form, nprobe, k)] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
            wins = []
            for nq in NQS:
                q, pr = qs[:nq].contiguous(), near[:nq, :nprobe].contiguous()
                thr = pq.flat_search_lists_device(q, x, off, pr, RANGE_RANK)[0][:, RANGE_RANK - 1].contiguous()
                cell = {"form": form, "nq": nq, "nprobe": nprobe, "rank": RANGE_RANK}
                wins.append(compare(res, "range", cell, lambda: pq.flat_range_lists_batch_device(q, x, off, pr, thr, x_exp=x_exp),
                                    lambda: pq.flat_range_lists_device(q, x, off, pr, thr)))
            res["crossover"]["%s nprobe=%d range" % (form, nprobe)] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
