"""ADC search for query batches over 4-bit packed codes (Pq.adc_search_batch_device(packed4=True): one-hot screen on the
i8 matrix cores, exact resolve) against the plain packed search and against the u8 batch route on the unpacked codes, in
one process on the same data, on one MI355X.

Data: the mixture of tools/adc_batch_time.py (1,024 standard-normal centres, noise 0.35, log-normal lengths), a quantizer
of K = 16 centroids per subquantizer trained by 8 k-means iterations on 200,000 unit rows; the code matrix holds the codes
of the unit rows, `scales` their lengths, once unpacked and once packed (pack_codes4_device).

Shapes: n rows (default 10 M) at d = 128 / M = 16 and d = 768 / M = 48; nq in {8, 32, 64, 256, 1,024}; k in {10, 100,
1,024}; squared L2 and the scaled inner product.  HIP events around the call, median of 5 after 2 warm-up calls (3 after 1
where one call takes more than a second).  Every cell is compared bit for bit with the plain packed search before it is
timed.  Each cell records the candidates as a fraction of n nq and the queries that took the plain call inside the route.
Per (M, form, nq), at the thresholds of k = 100, the COUNT KERNEL alone of the one-hot screen (k_adc_screen_p4) beside the
u8 screen's (k_adc_screen_u8): device time of the kernel from torch.profiler's kernel records, summed over the passes of a
capacity-0 call, mean of 5 calls after a warm-up call, and the (row, query) pairs per second it implies against the paper
figure.  The whole capacity-0 call (prep, count, scan and the read of lims[-1]) is recorded beside it as count_call_ms.
"crossover" is the smallest nq from which the packed batch route beats the plain packed search by more than the larger
spread of the two, for every larger nq; a cell where it does not win is listed under "findings".

Writes JSON (default profiles/adc_packed4_batch_time.json).

usage: python tools/adc_packed4_batch_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from reductive_amd import pq as rules  # noqa: E402
from adc_batch_time import CENTRES, CHUNK, LENGTH_SIGMA, NOISE, TRAIN_ITERATIONS, TRAIN_ROWS, draw, unit  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_packed4_batch_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
DIMS = {16: 128, 48: 768}
MS = [int(a) for a in sys.argv[3:]] or [16, 48]
K = 16
NQS, KS = (8, 32, 64, 256, 1024), (10, 100, 1024)
PAPER_PAIRS_PER_S = 5e12


def index(M, gen):
    """-> (pq, codes [N, M] u8, packed [N, M / 2] u8, lengths [N], L2 tables, IP tables) of the mixture"""
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
    return pq, codes, pq.pack_codes4_device(codes), lengths, pq.adc_tables_device(unit(q)), pq.adc_ip_tables_device(q.contiguous())


def kernel_ms(fn, needle, reps=5):
    """device time per call of fn, in ms, of the kernels whose name contains `needle` (torch.profiler's kernel records)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    us = [getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0) for e in prof.key_averages() if needle in e.key and "prep" not in e.key]
    assert us and sum(us) > 0, "no kernel record of %s" % needle
    return sum(us) / reps / 1000.0


def count_calls(pq, codes, packed, t, thr, ip, kw):
    """the count kernel alone and the whole capacity-0 call of both screens at the same thresholds"""
    out = {}
    for name, c, packed4, kernel in (("onehot", packed, True, "k_adc_screen_p4"), ("u8", codes, False, "k_adc_screen_u8")):
        def call():
            return pq._adc_screen(c, t, thr, ip, kw.get("scales"), None, 0, None, False, pq._adc_screen_entry(8, packed4), packed4)
        ms = kernel_ms(call, kernel)
        out[name + "_count_kernel_ms"] = round(ms, 4)
        out[name + "_count_call_ms"] = round(timed(call)[0], 4)
        out[name + "_pairs_per_s"] = float("%.4g" % (float(N) * t.shape[0] / (ms * 1e-3)))
    out["onehot_share_of_paper"] = round(out["onehot_pairs_per_s"] / PAPER_PAIRS_PER_S, 4)
    return out


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
           "data": "mixture of %d standard-normal centres, noise %.2f, log-normal lengths (sigma %.2f); quantizer: %d k-means "
                   "iterations on %d unit rows; codes of the unit rows, scales their lengths" % (CENTRES, NOISE, LENGTH_SIGMA,
                                                                                               TRAIN_ITERATIONS, TRAIN_ROWS),
           "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second)",
           "paper_pairs_per_s": PAPER_PAIRS_PER_S, "cells": [], "count_calls": [], "crossover": {}, "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    for M in MS:
        pq, codes, packed, lengths, t_l2, t_ip = index(M, torch.Generator(device="cuda").manual_seed(61 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_search_device if ip else pq.adc_search_device
            for k in KS:
                wins = []
                for nq in NQS:
                    t = tables[:nq].contiguous()
                    want = plain(packed, t, k, packed4=True, **kw)
                    st = {}
                    got = pq.adc_search_batch_device(packed, t, k, ip=ip, stats=st, packed4=True, **kw)
                    cell = {"M": M, "form": form, "nq": nq, "k": k, "equal": same(got, want), "fallback_queries": st["fallback_queries"],
                            "candidate_fraction": round(st["candidates"] / (float(N) * nq), 6)}
                    assert cell["equal"], cell
                    cell["onehot_batch_ms"], a = timed(lambda: pq.adc_search_batch_device(packed, t, k, ip=ip, packed4=True, **kw))
                    cell["plain_packed_ms"], b = timed(lambda: plain(packed, t, k, packed4=True, **kw))
                    cell["u8_batch_ms"], _ = timed(lambda: pq.adc_search_batch_device(codes, t, k, ip=ip, **kw))
                    cell["spread_ms"] = round(max(max(x) - min(x) for x in (a, b)), 4)
                    cell["onehot_over_plain_packed"] = round(cell["onehot_batch_ms"] / cell["plain_packed_ms"], 4)
                    cell["onehot_over_u8_batch"] = round(cell["onehot_batch_ms"] / cell["u8_batch_ms"], 4)
                    if k == 100:
                        res["count_calls"].append(dict(M=M, form=form, nq=nq, **count_calls(pq, codes, packed, t, want[0][:, k - 1].contiguous(),
                                                                                             ip, kw)))
                    won = cell["plain_packed_ms"] - cell["onehot_batch_ms"] > cell["spread_ms"]
                    wins.append(won)
                    if not won:
                        res["findings"].append("M=%d %s nq=%d k=%d: one-hot batch %.3f ms, plain packed %.3f ms" %
                                               (M, form, nq, k, cell["onehot_batch_ms"], cell["plain_packed_ms"]))
                    res["cells"].append(cell)
                    save()
                    print(json.dumps(cell), flush=True)
                res["crossover"]["M=%d %s k=%d" % (M, form, k)] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
        del pq, codes, packed, lengths, t_l2, t_ip
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
