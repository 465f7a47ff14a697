"""ADC similarity search (inner product, top-k largest) against the L2 search and the route it replaces: 100 M resident
rows, M = 15, K = 256, nq in {1, 8, 32}, k in {1, 10, 100, 1024}.  Times with HIP events (warmed up, median of
repeats), in one process: adc_ip_search_device without scales; with scales (one f32 per row); adc_search_device (L2) on
the same codes; adc_scan_device over the IP tables * scales + torch.topk(largest=True).  Every similarity result is checked
against the scan + an exact selection on the device (torch.topk over the distinct 64-bit keys (order key of -score) *
2^27 + row).  Writes JSON (default profiles/adc_ip_search_time.json).

usage: python tools/adc_ip_search_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_search_time import order_keys, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_ip_search_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
M, K, DSUB = 15, 256, 20
NQS, KS = (1, 8, 32), (1, 10, 100, 1024)


def exact(score_all, idx, score, k):
    """idx / score [nq, k] against the exact selection over score_all [nq, n] (largest first, ties to the smaller row)"""
    ok = True
    for j in range(score_all.shape[0]):
        want = torch.topk(order_keys(-score_all[j]), k, largest=False, sorted=True).values & ((1 << 27) - 1)
        ok &= bool(torch.equal(idx[j], want))
        ok &= bool(torch.equal(score[j].view(torch.int32), (score_all[j][want] + 0.0).view(torch.int32)))
    return ok


def main():
    assert N < (1 << 27)
    rng = np.random.default_rng(7)
    q = rng.standard_normal((M, K, DSUB), dtype=np.float32)
    pq = ra.Pq(None, q)
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    scales = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda()
    ys = torch.from_numpy(rng.standard_normal((max(NQS), M * DSUB), dtype=np.float32)).cuda()
    ip_all = pq.adc_ip_tables_device(ys)
    l2_all = pq.adc_tables_device(ys)
    res = {"shape": {"n": N, "M": M, "K": K}, "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0),
           "runs": []}
    for nq in NQS:
        t, t2 = ip_all[:nq].contiguous(), l2_all[:nq].contiguous()
        out = torch.empty((nq, N), dtype=torch.float32, device="cuda")
        scan = pq.adc_scan_device(codes, t, out=out).clone()
        scaled = scan * scales
        for k in KS:
            ra.launch_log(reset=True)
            pq.adc_ip_search_device(codes, t, k, scales=scales)
            torch.cuda.synchronize()
            log = ra.launch_log(reset=True)
            ip_ms, ip_all_ms = timed(lambda: pq.adc_ip_search_device(codes, t, k))
            ips_ms, ips_all_ms = timed(lambda: pq.adc_ip_search_device(codes, t, k, scales=scales))
            l2_ms, l2_all_ms = timed(lambda: pq.adc_search_device(codes, t2, k))
            topk_ms, topk_all_ms = timed(
                lambda: torch.topk(pq.adc_scan_device(codes, t, out=out) * scales, k, dim=1, largest=True))
            s, i = pq.adc_ip_search_device(codes, t, k, check=True)
            ok = exact(scan, i, s, k)
            s, i = pq.adc_ip_search_device(codes, t, k, scales=scales, check=True)
            ok &= exact(scaled, i, s, k)
            row = {"nq": nq, "k": k, "ip_ms": round(ip_ms, 4), "ip_scaled_ms": round(ips_ms, 4),
                   "l2_ms": round(l2_ms, 4), "scan_mul_topk_ms": round(topk_ms, 4),
                   "ip_over_l2": round(ip_ms / l2_ms, 3), "ip_scaled_over_l2": round(ips_ms / l2_ms, 3),
                   "scan_mul_topk_over_ip_scaled": round(topk_ms / ips_ms, 2), "exact": ok, "ip_launches": log,
                   "all_ms": {"ip": ip_all_ms, "ip_scaled": ips_all_ms, "l2": l2_all_ms, "scan_mul_topk": topk_all_ms}}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
        del out, scan, scaled
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "similarity search differs from scan + selection"


if __name__ == "__main__":
    main()
