"""ADC search for query batches (Pq.adc_search_batch_device: u8 table screen, exact resolve) against the unchanged plain
calls (adc_search_device, adc_ip_search_device with scales), in one process on the same buffers, on one MI355X.

Data: a mixture, not noise.  1,024 centres drawn standard normal in d dimensions; a row is a centre chosen uniformly plus
0.35 x standard-normal noise, times a log-normal length factor exp(0.25 g).  The quantizer (K = 256 centroids per
subquantizer) is trained on 200,000 such rows scaled to unit length: 256 of them as initial centroids, 8 k-means
iterations on the device.  The code matrix holds the codes of the rows scaled to unit length, `scales` their lengths, as a
QuantizedMatrix keeps them.  Queries are further draws from the mixture: scaled to unit length for squared L2
(adc_tables_device), as drawn for the scaled inner product (adc_ip_tables_device, score = fl(sum * length)).

Shapes: n rows (default 10 M) at d = 300 / M = 15 and d = 768 / M = 48; nq in {8, 32, 64, 256, 1,024}; k in {10, 100,
1,024}.  HIP events around the call, median of 5 after 2 warm-up calls (3 after 1 where one call takes more than a second).
Every cell is compared bit for bit with the plain call before it is timed.  Each cell records the candidates as a fraction
of n nq, the queries that took the plain call inside the batch route, and the route's stages timed separately with the
same protocol: sample (the candidate call over every t-th row), screen (adc_screen at the route's capacity, per chunk of
queries) and resolve (the candidate call over the screen's ids, for the chunks that did not fall back).
"crossover" is the smallest nq from which the batch route wins a column by more than the larger spread of the two, for
every larger nq; a cell where it does not win is listed under "findings".

Writes JSON (default profiles/adc_batch_time.json).

usage: python tools/adc_batch_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_batch_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
DIMS = {15: 300, 48: 768}
MS = [int(a) for a in sys.argv[3:]] or [15, 48]
K = 256
NQS, KS = (8, 32, 64, 256, 1024), (10, 100, 1024)
CENTRES, NOISE, LENGTH_SIGMA = 1024, 0.35, 0.25
TRAIN_ROWS, TRAIN_ITERATIONS = 200_000, 8
CHUNK = 500_000


def draw(centres, n, gen):
    d = centres.shape[1]
    x = centres[torch.randint(0, CENTRES, (n,), device="cuda", generator=gen)]
    x = x + NOISE * torch.randn((n, d), device="cuda", generator=gen)
    return x * torch.exp(LENGTH_SIGMA * torch.randn((n, 1), device="cuda", generator=gen))


def unit(x):
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def index(M, gen):
    """-> (pq, codes [N, M] u8, lengths [N], L2 tables, IP tables) of the mixture"""
    d = DIMS[M]
    centres = torch.randn((CENTRES, d), device="cuda", generator=gen)
    train = unit(draw(centres, TRAIN_ROWS, gen))
    init = train[:K].cpu().numpy().reshape(K, M, d // M).transpose(1, 0, 2)
    books, _ = rules.kmeans_iterations(init, train, TRAIN_ITERATIONS, want_loss=False)
    pq = ra.Pq(None, books)
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(N, dtype=torch.float32, device="cuda")
    for r0 in range(0, N, CHUNK):
        x = draw(centres, min(CHUNK, N - r0), gen)
        lengths[r0:r0 + CHUNK] = x.norm(dim=1)
        pq.quantize_batch_device(unit(x), out=codes[r0:r0 + CHUNK])
    q = draw(centres, max(NQS), gen)
    torch.cuda.synchronize()
    return pq, codes, lengths, pq.adc_tables_device(unit(q)), pq.adc_ip_tables_device(q.contiguous())


def stages(pq, codes, t, k, ip, kw):
    """the stages of one batch call, each timed on its own, as Pq.adc_search_batch_device runs them"""
    among = pq.adc_ip_among_device if ip else pq.adc_among_device
    nq = t.shape[0]
    S, step = rules.flat_batch_sample(N, k)
    ids = torch.arange(0, N, step, dtype=torch.int64, device="cuda")
    out = {"sample_rows": int(ids.shape[0])}
    out["sample_ms"], _ = timed(lambda: among(codes, t, ids, k, **kw))
    thr = among(codes, t, ids, k, **kw)[0][:, k - 1].contiguous()
    chunks = [(q0, min(nq, q0 + rules.FLAT_BATCH_CHUNK)) for q0 in range(0, nq, rules.FLAT_BATCH_CHUNK)]

    def screen():
        return [pq._adc_screen(codes, t[a:b], thr[a:b], ip, kw.get("scales"), None, rules.flat_batch_capacity(N, b - a, k, S), None, False)
                for a, b in chunks]
    out["screen_ms"], _ = timed(screen)
    kept = [(a, b, r[0], r[1]) for (a, b), r in zip(chunks, screen()) if not rules.flat_batch_falls_back(r[2], N, b - a)]
    out["chunks_resolved"] = "%d of %d" % (len(kept), len(chunks))
    out["resolve_ms"] = None
    if kept:
        out["resolve_ms"], _ = timed(lambda: [among(codes, t[a:b], cand, k, lims=lims, **kw) for a, b, lims, cand in kept])
    return {a: (round(b, 4) if isinstance(b, float) else b) for a, b in out.items()}


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
           "data": "mixture of %d standard-normal centres, noise %.2f, log-normal lengths (sigma %.2f); quantizer: %d k-means "
                   "iterations on %d unit rows; codes of the unit rows, scales their lengths" % (CENTRES, NOISE, LENGTH_SIGMA,
                                                                                               TRAIN_ITERATIONS, TRAIN_ROWS),
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second)",
           "cells": [], "crossover": {}, "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in MS:
        pq, codes, lengths, t_l2, t_ip = index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_search_device if ip else pq.adc_search_device
            for k in KS:
                wins = []
                for nq in NQS:
                    t = tables[:nq].contiguous()
                    want = plain(codes, t, k, **kw)
                    st = {}
                    got = pq.adc_search_batch_device(codes, t, k, ip=ip, stats=st, **kw)
                    cell = {"M": M, "form": form, "nq": nq, "k": k, "equal": same(got, want), "fallback_queries": st["fallback_queries"],
                            "candidate_fraction": round(st["candidates"] / (float(N) * nq), 6)}
                    assert cell["equal"], cell
                    cell["batch_ms"], cell["batch_all"] = timed(lambda: pq.adc_search_batch_device(codes, t, k, ip=ip, **kw))
                    cell["plain_ms"], cell["plain_all"] = timed(lambda: plain(codes, t, k, **kw))
                    cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
                    cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
                    cell["stages"] = stages(pq, codes, t, k, ip, kw)
                    won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
                    wins.append(won)
                    if not won:
                        res["findings"].append("M=%d %s nq=%d k=%d: batch %.3f ms, plain %.3f ms" % (M, form, nq, k, cell["batch_ms"],
                                                                                                   cell["plain_ms"]))
                    res["cells"].append(cell)
                    save()
                    print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
                res["crossover"]["M=%d %s k=%d" % (M, form, k)] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
        del pq, codes, lengths, t_l2, t_ip
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
