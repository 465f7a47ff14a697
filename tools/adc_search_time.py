"""ADC search against the scan it replaces: 100 M resident rows, M = 15, K = 256, nq in {1, 8, 32}, k in {1, 10, 100, 1024}.
Times with HIP events (warmed up, median of repeats): adc_search_device; adc_scan_device; adc_scan_device + torch.topk(largest=False).
Every search result is checked against the scan + an exact selection on the device (torch.topk over the distinct 64-bit keys
(order key of the distance) * 2^27 + row: one answer, ties to the smaller row).  Writes JSON (default profiles/adc_search_time.json).

usage: python tools/adc_search_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_search_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
M, K, DSUB = 15, 256, 20
NQS, KS = (1, 8, 32), (1, 10, 100, 1024)
WARM, REPS = 2, 7


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def order_keys(dist):
    """[n] f32 -> int64 (order key << 27) | row: NaN above +Inf, -0 == +0, distinct per row (n < 2^27)."""
    b = dist.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where(b >= 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    key = torch.where(torch.isnan(dist), torch.full_like(key, 0xFFFFFFFF), key)
    return (key << 27) | torch.arange(dist.numel(), device=dist.device, dtype=torch.int64)


def main():
    assert N < (1 << 27)
    rng = np.random.default_rng(7)
    q = rng.standard_normal((M, K, DSUB), dtype=np.float32)
    pq = ra.Pq(None, q)
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    ys = torch.from_numpy(rng.standard_normal((max(NQS), M * DSUB), dtype=np.float32)).cuda()
    tables_all = pq.adc_tables_device(ys)
    res = {"shape": {"n": N, "M": M, "K": K}, "warmup": WARM, "reps": REPS, "device": torch.cuda.get_device_name(0),
           "runs": []}
    for nq in NQS:
        t = tables_all[:nq].contiguous()
        out = torch.empty((nq, N), dtype=torch.float32, device="cuda")
        ra.launch_log(reset=True)
        scan_ms, scan_all = timed(lambda: pq.adc_scan_device(codes, t, out=out))
        scan_log = ra.launch_log(reset=True)
        scan = out.clone()
        for k in KS:
            ra.launch_log(reset=True)
            pq.adc_search_device(codes, t, k)
            torch.cuda.synchronize()
            search_log = ra.launch_log(reset=True)
            search_ms, search_all = timed(lambda: pq.adc_search_device(codes, t, k))
            topk_ms, topk_all = timed(lambda: torch.topk(pq.adc_scan_device(codes, t, out=out), k, dim=1, largest=False))
            d, i = pq.adc_search_device(codes, t, k, check=True)
            ok = True
            for j in range(nq):
                want = torch.topk(order_keys(scan[j]), k, largest=False, sorted=True).values & ((1 << 27) - 1)
                ok &= bool(torch.equal(i[j], want))
                ok &= bool(torch.equal(d[j].view(torch.int32), scan[j][want].view(torch.int32)))
            row = {"nq": nq, "k": k, "search_ms": round(search_ms, 4), "scan_ms": round(scan_ms, 4),
                   "scan_topk_ms": round(topk_ms, 4), "search_over_scan": round(search_ms / scan_ms, 3),
                   "search_over_scan_topk": round(search_ms / topk_ms, 3), "exact": ok,
                   "search_launches": search_log, "scan_launches": scan_log,
                   "all_ms": {"search": search_all, "scan": scan_all, "scan_topk": topk_all}}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
        del out, scan
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "search differs from scan + selection"


if __name__ == "__main__":
    main()
