"""ADC search in probed lists for query batches (Pq.adc_search_lists_batch_device: u8 table screen per list, exact resolve)
against the unchanged plain list searches (adc_search_lists_device, adc_ip_search_lists_device with scales), in one
process on the same buffers, on one MI355X.

Data: the clustered mixture and the quantizer of tools/adc_batch_time.py (1,024 centres, noise 0.35, log-normal lengths;
K = 256, 8 k-means iterations on 200,000 unit rows).  The coarse quantizer is the 1,024 mixture centres scaled to unit
length: a row goes to the list of the nearest one, the code matrix and the lengths are stored in list order, and a query
probes its nprobe nearest lists, nearest first.

Shapes: n rows (default 10 M) at d = 300 / M = 15 and d = 768 / M = 48; 1,024 lists; nprobe in {8, 64}; nq in {8, 32, 64,
256, 1,024}; k in {10, 100, 1,024}; squared L2 and the scaled inner product.  HIP events around the call, median of 5
after 2 warm-up calls (3 after 1 where one call takes more than a second).  Every cell is compared bit for bit with the
plain call before it is timed.  Each cell records the candidates as a share of the expected probed rows, the queries
that took the plain call inside the batch route, and the spread of both routes.  "crossover" is the smallest nq from
which the batch route wins a column by more than the larger spread of the two, for every larger nq; a cell where it does
not win is listed under "findings".  With unit_rows given, the screen alone is also timed at each of them (nq = 256 and
1,024, k = 10): what the default of option "adc_screen_lists_unit_rows" was chosen from.

Writes JSON (default profiles/adc_lists_batch_time.json).

usage: python tools/adc_lists_batch_time.py [out.json] [n_rows] [M ...] [--unit-rows R ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ARGS = sys.argv[1:]
UNIT_ROWS = [int(a) for a in ARGS[ARGS.index("--unit-rows") + 1:]] if "--unit-rows" in ARGS else []
ARGS = ARGS[:ARGS.index("--unit-rows")] if "--unit-rows" in ARGS else ARGS
sys.argv = sys.argv[:1] + ARGS                # the modules imported below read the same leading arguments
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402
from adc_batch_time import CENTRES, CHUNK, DIMS, K, KS, NQS, TRAIN_ITERATIONS, TRAIN_ROWS, draw, unit  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "adc_lists_batch_time.json")
N = int(ARGS[1]) if len(ARGS) > 1 else 10_000_000
MS = [int(a) for a in ARGS[2:]] or [15, 48]
NPROBES = (8, 64)


def index(M, gen):
    """-> (pq, codes [N, M] u8 and lengths [N] in list order, list_off, L2 tables, IP tables, probes [nq, 64])"""
    d = DIMS[M]
    centres = torch.randn((CENTRES, d), device="cuda", generator=gen)
    coarse = unit(centres)
    train = unit(draw(centres, TRAIN_ROWS, gen))
    init = train[:K].cpu().numpy().reshape(K, M, d // M).transpose(1, 0, 2)
    books, _ = rules.kmeans_iterations(init, train, TRAIN_ITERATIONS, want_loss=False)
    pq = ra.Pq(None, books)
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(N, dtype=torch.float32, device="cuda")
    assign = torch.empty(N, dtype=torch.int64, device="cuda")
    for r0 in range(0, N, CHUNK):
        x = draw(centres, min(CHUNK, N - r0), gen)
        lengths[r0:r0 + CHUNK] = x.norm(dim=1)
        u = unit(x)
        assign[r0:r0 + CHUNK] = (u @ coarse.T).argmax(dim=1)
        pq.quantize_batch_device(u, out=codes[r0:r0 + CHUNK])
    order = torch.sort(assign, stable=True).indices
    codes, lengths = codes[order].contiguous(), lengths[order].contiguous()
    list_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.bincount(assign, minlength=CENTRES), 0)])
    q = draw(centres, max(NQS), gen)
    probes = (unit(q) @ coarse.T).topk(max(NPROBES), dim=1).indices.contiguous()
    torch.cuda.synchronize()
    return pq, codes, lengths, list_off, pq.adc_tables_device(unit(q)), pq.adc_ip_tables_device(q.contiguous()), probes


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "lists": CENTRES, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
           "data": "the mixture and quantizer of adc_batch_time.py; lists: the nearest of the %d unit centres; codes and lengths in "
                   "list order; probes: the nprobe nearest lists of a query" % CENTRES,
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second)",
           "cells": [], "crossover": {}, "findings": [], "unit_rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in MS:
        pq, codes, lengths, list_off, t_l2, t_ip, probes = index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_search_lists_device if ip else pq.adc_search_lists_device
            for n_probe in NPROBES:
                expected = float(N) * n_probe / CENTRES
                for k in KS:
                    wins = []
                    for nq in NQS:
                        t, pr = tables[:nq].contiguous(), probes[:nq, :n_probe].contiguous()
                        want = plain(codes, t, list_off, pr, k, **kw)
                        st = {}
                        got = pq.adc_search_lists_batch_device(codes, t, list_off, pr, k, ip=ip, stats=st, **kw)
                        cell = {"M": M, "form": form, "nprobe": n_probe, "nq": nq, "k": k, "equal": same(got, want),
                                "fallback_queries": st["fallback_queries"], "sample_slots": st["sample_slots"],
                                "candidate_share": round(st["candidates"] / (expected * nq), 6)}
                        assert cell["equal"], cell
                        cell["batch_ms"], cell["batch_all"] = timed(lambda: pq.adc_search_lists_batch_device(codes, t, list_off, pr, k, ip=ip, **kw))
                        cell["plain_ms"], cell["plain_all"] = timed(lambda: plain(codes, t, list_off, pr, k, **kw))
                        cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
                        cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
                        won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
                        wins.append(won)
                        if not won:
                            res["findings"].append("M=%d %s nprobe=%d nq=%d k=%d: batch %.3f ms, plain %.3f ms"
                                                   % (M, form, n_probe, nq, k, cell["batch_ms"], cell["plain_ms"]))
                        res["cells"].append(cell)
                        save()
                        print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
                    res["crossover"]["M=%d %s nprobe=%d k=%d" % (M, form, n_probe, k)] = next(
                        (NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
        for rows in UNIT_ROWS:                                              # the screen alone, at the sample's thresholds
            ra.set_option("adc_screen_lists_unit_rows", rows)
            for nq in (256, 1024):
                t, pr = t_l2[:nq].contiguous(), probes[:nq, :64].contiguous()
                thr = pq.adc_search_lists_device(codes, t, list_off, pr[:, :2].contiguous(), 10)[0][:, 9].contiguous()
                ms, _ = timed(lambda: pq._adc_screen_lists(codes, t, list_off, pr, thr, False, None, None, 1 << 24, None, False))
                res["unit_rows"].append({"M": M, "nq": nq, "nprobe": 64, "unit_rows": rows, "screen_ms": round(ms, 4)})
                print(json.dumps(res["unit_rows"][-1]), flush=True)
        ra.set_option("adc_screen_lists_unit_rows", 0)
        save()
        del pq, codes, lengths, t_l2, t_ip
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
