"""IVFADC residual search for query batches (Pq.adc_search_lists_residual_batch_device: u8 table screen with list and row
terms, exact resolve) against the unchanged plain residual list searches (adc_search_lists_residual_device,
adc_ip_search_lists_residual_device with scales), in one process on the same buffers, on one MI355X.

Data, shapes, `timed` and `same` are those of tools/adc_lists_batch_time.py: the clustered mixture of
tools/adc_batch_time.py (1,024 centres, noise 0.35, log-normal lengths; K = 256), nprobe in {8, 64}, nq in {8, 32, 64, 256,
1,024}, k in {10, 100, 1,024}, squared L2 and the scaled inner product.  The index is built from the unit rows by
QuantizedMatrix.partition_residual(1,024 lists, on_device=True), coarse and residual quantizer trained on 200,000 rows;
a query probes its nprobe nearest non-empty lists by the coarse table, whose entries are the biases (probes_of).  Every cell is compared bit for bit with the
plain residual call of the same run before it is timed, and records both medians and spreads, the rows a query really probes, the candidates as a share
of them and the queries that took the plain call inside the batch route.  "crossover" is the
smallest nq from which the batch route wins a column by more than the larger spread of the two, for every larger nq; a
cell where it does not win is listed under "findings".  "screen_alone" (nq = 256 and 1,024, nprobe 64, k = 10): the stages of the batch
route each alone -- sample, screen, resolve -- and the residual screen's count pass against the table screen's on the same
codes, tables and probes, both as count calls (capacity 0): the ratio is what the per-(row, pair) epilogue costs.

Writes JSON (default profiles/adc_residual_batch_time.json).

usage: python tools/adc_residual_batch_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ARGS = sys.argv[1:]
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules, qmatrix  # noqa: E402
from adc_batch_time import CENTRES, CHUNK, DIMS, K, KS, NQS, TRAIN_ITERATIONS, TRAIN_ROWS, draw, unit  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "adc_residual_batch_time.json")
N = int(ARGS[1]) if len(ARGS) > 1 else 10_000_000
MS = [int(a) for a in ARGS[2:]] or [15, 48]
NPROBES = (8, 64)


def index(M, gen):
    """-> (the residual matrix, queries [max nq, d] on the device)"""
    d = DIMS[M]
    centres = torch.randn((CENTRES, d), device="cuda", generator=gen)
    train = unit(draw(centres, TRAIN_ROWS, gen))
    init = train[:K].cpu().numpy().reshape(K, M, d // M).transpose(1, 0, 2)
    books, _ = rules.kmeans_iterations(init, train, TRAIN_ITERATIONS, want_loss=False)
    flat = ra.Pq(None, books)
    x = torch.empty((N, d), dtype=torch.float32, device="cuda")
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(N, dtype=torch.float32, device="cuda")
    for r0 in range(0, N, CHUNK):
        rows = draw(centres, min(CHUNK, N - r0), gen)
        lengths[r0:r0 + CHUNK] = rows.norm(dim=1)
        x[r0:r0 + CHUNK] = unit(rows)
        flat.quantize_batch_device(x[r0:r0 + CHUNK], out=codes[r0:r0 + CHUNK])
    qm = qmatrix.QuantizedMatrix(flat, codes.cpu().numpy(), norms=lengths.cpu().numpy())
    rm = qm.partition_residual(CENTRES, n_iterations=TRAIN_ITERATIONS, pq_iterations=TRAIN_ITERATIONS, vectors=x, train_rows=TRAIN_ROWS,
                               rng=np.random.default_rng(61 + M), on_device=True)
    q = draw(centres, max(NQS), gen).contiguous()
    torch.cuda.synchronize()
    return rm, q


def probes_of(rm, qq, ip, n_probe, sizes):
    """(probes, biases): the n_probe nearest NON-EMPTY lists of every query by the coarse table -- |q - c_l|^2 resp. <q, c_l>,
    the entries the matrix itself hands to the searches as biases.  The coarse k-means leaves lists without rows, whose
    centroids at the origin are nearer to a unit query than any other list but its own: probing them would stream nothing."""
    ct = (rm.coarse.adc_ip_tables_device(qq) if ip else rm.coarse.adc_tables_device(qq))[:, 0, :]
    key = torch.where(sizes[None] > 0, ct if ip else -ct, torch.full_like(ct, float("-inf")))
    pr = key.topk(n_probe, dim=1).indices.contiguous()
    return pr, torch.gather(ct, 1, pr).contiguous()


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "lists": CENTRES, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
           "data": "the mixture of adc_batch_time.py, unit rows; index: QuantizedMatrix.partition_residual(%d lists, on_device=True), "
                   "coarse and residual quantizer trained on %d rows; probes: the nprobe nearest non-empty lists by the coarse table" % (CENTRES, TRAIN_ROWS),
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second)",
           "cells": [], "crossover": {}, "findings": [], "screen_alone": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in MS:
        rm, q = index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        pq, codes, off = rm.pq, rm.codes, rm.list_off
        sizes = off[1:] - off[:-1]
        res["shapes"]["M=%d" % M]["list_rows"] = {"min": int(sizes.min()), "median": int(sizes.median()), "max": int(sizes.max())}
        for ip, form in ((False, "l2"), (True, "ip_scaled")):
            for n_probe in NPROBES:
                qq = q if ip else unit(q)
                pr_all, b_all = probes_of(rm, qq, ip, n_probe, sizes)
                t_all = pq.adc_ip_tables_device(qq)
                for k in KS:
                    wins = []
                    for nq in NQS:
                        t, pr, b = t_all[:nq].contiguous(), pr_all[:nq].contiguous(), b_all[:nq].contiguous()
                        if ip:
                            plain = lambda: pq.adc_ip_search_lists_residual_device(codes, t, off, pr, b, k, scales=rm.norms)
                            batch = lambda st=None: pq.adc_search_lists_residual_batch_device(codes, t, off, pr, b, None, rm.lists, k, ip=True,
                                                                                              scales=rm.norms, stats=st)
                        else:
                            plain = lambda: pq.adc_search_lists_residual_device(codes, t, off, pr, b, rm.row_terms, k)
                            batch = lambda st=None: pq.adc_search_lists_residual_batch_device(codes, t, off, pr, b, rm.row_terms, rm.lists, k,
                                                                                              stats=st)
                        st, probed = {}, int(sizes[pr.clamp(min=0)].sum())         # the rows the cell's queries really probe
                        cell = {"M": M, "form": form, "nprobe": n_probe, "nq": nq, "k": k, "equal": same(batch(st), plain()),
                                "fallback_queries": st["fallback_queries"], "sample_slots": st["sample_slots"],
                                "probed_rows_per_query": probed // nq, "candidate_share": round(st["candidates"] / max(probed, 1), 6)}
                        assert cell["equal"], cell
                        cell["batch_ms"], cell["batch_all"] = timed(batch)
                        cell["plain_ms"], cell["plain_all"] = timed(plain)
                        cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
                        cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
                        won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
                        wins.append(won)
                        if not won:
                            res["findings"].append("M=%d %s nprobe=%d nq=%d k=%d: batch %.3f ms, plain %.3f ms"
                                                   % (M, form, n_probe, nq, k, cell["batch_ms"], cell["plain_ms"]))
                        res["cells"].append(cell)
                        save()
                        print(json.dumps({a: c for a, c in cell.items() if not a.endswith("_all")}), flush=True)
                    res["crossover"]["M=%d %s nprobe=%d k=%d" % (M, form, n_probe, k)] = next(
                        (NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
        pr_all, b_all = probes_of(rm, unit(q), False, 64, sizes)                # the screens alone, at the sample's thresholds
        t_all = pq.adc_ip_tables_device(unit(q))
        for nq in (256, 1024):
            t, pr, b = t_all[:nq].contiguous(), pr_all[:nq].contiguous(), b_all[:nq].contiguous()
            thr = pq.adc_search_lists_residual_device(codes, t, off, pr[:, :2].contiguous(), b[:, :2].contiguous(), rm.row_terms, 10)[0][:, 9].contiguous()
            full_ms, _ = timed(lambda: pq.adc_screen_lists_residual_device(codes, t, off, pr, b, rm.row_terms, thr, capacity=1 << 26))
            # the two count passes alone (capacity 0, no second call): the table screen's candidates are not the residual screen's
            count = dict(ip=False, scales=None, allow=None, cap=0, stream=None, retry=False)
            res_ms, _ = timed(lambda: pq._adc_screen_lists_residual(codes, t, off, pr, b, rm.row_terms, thr, **count))
            # the table screen reads the same codes through the same image machinery; its thresholds are its own sample's
            thr0 = pq.adc_search_lists_device(codes, t, off, pr[:, :2].contiguous(), 10)[0][:, 9].contiguous()
            tab_ms, _ = timed(lambda: pq._adc_screen_lists(codes, t, off, pr, thr0, **count))
            # the stages of the batch route at k = 10, each alone: the sample over its first slots and the resolve of the candidates
            slots = rules.flat_lists_batch_sample(N, CENTRES, 64, 10)
            ps, bs = pr[:, :slots].contiguous(), b[:, :slots].contiguous()
            sample_ms, _ = timed(lambda: pq.adc_search_lists_residual_device(codes, t, off, ps, bs, rm.row_terms, 10))
            lims, cand = pq.adc_screen_lists_residual_device(codes, t, off, pr, b, rm.row_terms, thr, capacity=1 << 26)
            lb = torch.zeros((nq, CENTRES + 1), device="cuda").scatter_(1, pr.clamp(min=0), b)[:, :CENTRES]   # probes_of yields no pads
            among_ms, _ = timed(lambda: pq.adc_among_device(codes, t, cand, 10, lims=lims, row_list=rm.lists, list_bias=lb, row_terms=rm.row_terms))
            res["screen_alone"].append({"M": M, "nq": nq, "nprobe": 64, "screen_ms": round(full_ms, 4), "residual_count_ms": round(res_ms, 4), "table_count_ms": round(tab_ms, 4),
                                        "ratio": round(res_ms / tab_ms, 4), "sample_ms": round(sample_ms, 4), "resolve_ms": round(among_ms, 4),
                                        "candidates": int(cand.shape[0])})
            print(json.dumps(res["screen_alone"][-1]), flush=True)
        save()
        del rm, codes, t_all
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
