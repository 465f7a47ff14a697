"""ADC search for query batches with the 16-bit table image (Pq.adc_search_batch_device(image_bits=16)) against the u8 route
(image_bits=8) and the unchanged plain calls, in one process on the same buffers, on one MI355X.  Data, quantizer,
queries, shapes and the timing helper are those of tools/adc_batch_time.py: n rows (default 10 M) of the
clustered mixture, K = 256, d = 300 / M = 15 and d = 768 / M = 48, squared L2 and the scaled inner product, nq in {8, 32,
64, 256, 1,024}, k in {10, 100, 1,024}.

Every cell is compared bit for bit with the plain call for both routes before anything is timed.  HIP events around the
call, median of 5 after 2 warm-up calls (3 after 1 where one call takes more than a second); the three are timed one after
the other within the cell, so a cell's numbers share the state of the machine.  A cell records, per route, the candidates
as a fraction of n nq and the queries that took the plain call inside the route.  "streams": the screen call alone at 4, 8
and 16 (u8: and 32) queries with thresholds from the k = 100 sample -- one stream of the codes where a pass holds them
(M = 15: every entry), ceil(nq / slots) streams where it does not (M = 48: 8 slots for u8, 4 for the 16-bit image).  "crossover": the smallest nq from which the 16-bit route beats the plain call by more than the larger spread, for
every larger nq; "findings": every cell where the 16-bit route does not beat the plain call, or not the u8 route.

Writes JSON (default profiles/adc_screen16_time.json).

usage: python tools/adc_screen16_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adc_batch_time as abt  # noqa: E402  (reads the same arguments: N, the shapes)
from adc_batch_time import rules, same, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_screen16_time.json")
N = abt.N


def streams(pq, codes, tables, ip, kw):
    """the screen call alone by image and batch size: ms per call, the candidates as a fraction of n nq"""
    among = pq.adc_ip_among_device if ip else pq.adc_among_device
    k = 100
    S, step = rules.flat_batch_sample(N, k)
    ids = torch.arange(0, N, step, dtype=torch.int64, device="cuda")
    out = {}
    for bits, entry in ((8, "pqhip_adc_screen_f32_dev"), (16, "pqhip_adc_screen16_f32_dev")):
        for nq in ((4, 8, 16, 32) if bits == 8 else (4, 8, 16)):
            t = tables[:nq].contiguous()
            thr = among(codes, t, ids, k, **kw)[0][:, k - 1].contiguous()
            cap = rules.flat_batch_capacity(N, nq, k, S)
            call = lambda: pq._adc_screen(codes, t, thr, ip, kw.get("scales"), None, cap, None, False, entry)  # noqa: E731
            ms, runs = timed(call)
            out["u%d nq=%d" % (bits, nq)] = {"ms": round(ms, 4), "all": runs, "candidate_fraction": round(call()[2] / (float(N) * nq), 6)}
    return out


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": abt.K, "shapes": {"M=%d" % M: {"d": abt.DIMS[M]} for M in abt.MS},
           "data": "that of tools/adc_batch_time.py: the same seeds, mixture, quantizer and queries",
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second); plain, u8 route "
                       "and 16-bit route timed one after the other within a cell",
           "cells": [], "streams": {}, "crossover": {}, "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in abt.MS:
        pq, codes, lengths, t_l2, t_ip = abt.index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_search_device if ip else pq.adc_search_device
            res["streams"]["M=%d %s" % (M, form)] = streams(pq, codes, tables, ip, kw)
            save()
            print(json.dumps({"streams M=%d %s" % (M, form): {a: b["ms"] for a, b in res["streams"]["M=%d %s" % (M, form)].items()}}), flush=True)
            for k in abt.KS:
                wins = []
                for nq in abt.NQS:
                    t = tables[:nq].contiguous()
                    want = plain(codes, t, k, **kw)
                    cell = {"M": M, "form": form, "nq": nq, "k": k}
                    for bits in (8, 16):
                        st = {}
                        got = pq.adc_search_batch_device(codes, t, k, ip=ip, stats=st, image_bits=bits, **kw)
                        assert same(got, want), (cell, bits)
                        cell["u%d_fallback_queries" % bits] = st["fallback_queries"]
                        cell["u%d_candidate_fraction" % bits] = round(st["candidates"] / (float(N) * nq), 6)
                    cell["equal"] = True
                    cell["plain_ms"], cell["plain_all"] = timed(lambda: plain(codes, t, k, **kw))
                    cell["u8_ms"], cell["u8_all"] = timed(lambda: pq.adc_search_batch_device(codes, t, k, ip=ip, **kw))
                    cell["u16_ms"], cell["u16_all"] = timed(lambda: pq.adc_search_batch_device(codes, t, k, ip=ip, image_bits=16, **kw))
                    cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["plain_all"], cell["u8_all"], cell["u16_all"])), 4)
                    cell["u16_over_plain"] = round(cell["u16_ms"] / cell["plain_ms"], 4)
                    cell["u16_over_u8"] = round(cell["u16_ms"] / cell["u8_ms"], 4)
                    won = cell["plain_ms"] - cell["u16_ms"] > cell["spread_ms"]
                    wins.append(won)
                    if not won or cell["u16_ms"] >= cell["u8_ms"]:
                        res["findings"].append("M=%d %s nq=%d k=%d: 16-bit %.3f ms, u8 %.3f ms, plain %.3f ms" % (
                            M, form, nq, k, cell["u16_ms"], cell["u8_ms"], cell["plain_ms"]))
                    res["cells"].append(cell)
                    save()
                    print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
                res["crossover"]["M=%d %s k=%d" % (M, form, k)] = next((abt.NQS[i] for i in range(len(abt.NQS)) if all(wins[i:])), None)
        del pq, codes, lengths, t_l2, t_ip
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
