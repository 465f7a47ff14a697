"""ADC search in probed lists for query batches over 4-BIT PACKED codes (Pq.adc_search_lists_batch_device(packed4=True):
one-hot i8 screen per list, exact resolve) against (a) the unchanged plain packed list searches
(adc_search_lists_device / adc_ip_search_lists_device with packed4=True) and (b) the u8 list batch route on the unpacked
codes, in one process on the same data, on one MI355X.

Data: the clustered mixture of tools/adc_batch_time.py with the K = 16 quantizer of tools/adc_packed4_batch_time.py
(d = 128 / M = 16 and d = 768 / M = 48), laid out in lists as in tools/adc_lists_batch_time.py: 1,024 lists around the
unit centres, codes and lengths in list order, a query probes its nprobe nearest lists, nearest first.

Shapes: n rows (default 10 M); nprobe in {8, 64}; nq in {8, 32, 64, 256, 1,024}; k in {10, 100, 1,024}; squared L2 and
the scaled inner product.  HIP events around the call, median of 5 after 2 warm-up calls (3 after 1 where one call takes
more than a second).  Every cell is compared bit for bit with the plain packed call -- and the u8 route with it -- before
it is timed.  A cell records the candidate share, the queries that took the plain call inside the route and the spread;
a cell where the packed route does not win against (a) or (b) by more than the spread is listed under "findings".

Writes JSON (default profiles/adc_packed4_lists_batch_time.json).

usage: python tools/adc_packed4_lists_batch_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402
from adc_batch_time import CENTRES, CHUNK, TRAIN_ITERATIONS, TRAIN_ROWS, draw, unit  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_packed4_lists_batch_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
DIMS = {16: 128, 48: 768}
MS = [int(a) for a in sys.argv[3:]] or [16, 48]
K = 16
NQS, KS, NPROBES = (8, 32, 64, 256, 1024), (10, 100, 1024), (8, 64)


def index(M, gen):
    """-> (pq, codes [N, M] u8, packed rows and lengths [N] in list order, list_off, L2 tables, IP tables, probes [nq, 64])"""
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
    return pq, codes, pq.pack_codes4_device(codes), lengths, list_off, pq.adc_tables_device(unit(q)), pq.adc_ip_tables_device(q.contiguous()), probes


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "lists": CENTRES, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
           "data": "the mixture of adc_batch_time.py, K = 16 quantizer; lists: the nearest of the %d unit centres; codes and "
                   "lengths in list order; probes: the nprobe nearest lists of a query" % CENTRES,
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second)",
           "cells": [], "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in MS:
        pq, codes, packed, lengths, list_off, t_l2, t_ip, probes = index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_search_lists_device if ip else pq.adc_search_lists_device
            for n_probe in NPROBES:
                expected = float(N) * n_probe / CENTRES
                for k in KS:
                    for nq in NQS:
                        t, pr = tables[:nq].contiguous(), probes[:nq, :n_probe].contiguous()
                        routes = {"packed": lambda st=None: pq.adc_search_lists_batch_device(packed, t, list_off, pr, k, ip=ip, stats=st, packed4=True, **kw),
                                  "plain": lambda: plain(packed, t, list_off, pr, k, packed4=True, **kw),
                                  "u8": lambda: pq.adc_search_lists_batch_device(codes, t, list_off, pr, k, ip=ip, **kw)}
                        want, st = routes["plain"](), {}
                        cell = {"M": M, "form": form, "nprobe": n_probe, "nq": nq, "k": k,
                                "equal": same(routes["packed"](st), want) and same(routes["u8"](), want),
                                "fallback_queries": st["fallback_queries"], "sample_slots": st["sample_slots"],
                                "candidate_share": round(st["candidates"] / (expected * nq), 6)}
                        assert cell["equal"], cell
                        for name, fn in routes.items():
                            cell[name + "_ms"], cell[name + "_all"] = timed(fn)
                        cell["spread_ms"] = round(max(max(cell[r + "_all"]) - min(cell[r + "_all"]) for r in routes), 4)
                        for other in ("plain", "u8"):
                            cell["packed_over_" + other] = round(cell["packed_ms"] / cell[other + "_ms"], 4)
                            if not cell[other + "_ms"] - cell["packed_ms"] > cell["spread_ms"]:
                                res["findings"].append("M=%d %s nprobe=%d nq=%d k=%d: packed %.3f ms, %s %.3f ms"
                                                       % (M, form, n_probe, nq, k, cell["packed_ms"], other, cell[other + "_ms"]))
                        res["cells"].append(cell)
                        save()
                        print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
        del pq, codes, packed, lengths, t_l2, t_ip
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
