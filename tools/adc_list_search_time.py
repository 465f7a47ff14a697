"""ADC search over a partitioned code matrix against the exhaustive search of the same run on the same data: 100 M
resident rows, M = 15, K = 256, n_lists = 1024 with a synthetic assignment (list sizes drawn from a log-normal, their
spread is recorded; timing needs no trained centroids), nprobe in {1, 8, 64, 1024}, nq in {1, 8, 256}, k in {10, 100},
distance (L2) and similarity (IP, with one f32 scale per row).  Times with HIP events (warmed up, median of repeats),
list search and exhaustive search alternating in one process.  Every cell is checked on the device for its first and
last query: adc_scan_device over the gathered probed rows + an exact selection (torch.topk over the distinct 64-bit
keys (order key << 27) | position).  One cell (nq = 1, nprobe = 64, k = 10) is also timed for forced workgroup counts
per query.  A small trained case (1 M clustered rows, n_lists = 256) records recall@10 of PartitionedMatrix.nearest
against the exhaustive search per nprobe -- information, not an assertion.  Writes JSON (default
profiles/adc_list_search_time.json).

usage: python tools/adc_list_search_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_search_time import timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_list_search_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
M, K, DSUB = 15, 256, 20
N_LISTS = 1024
NPROBES, NQS, KS = (1, 8, 64, 1024), (1, 8, 256), (10, 100)


def keys_of(value, pos):
    """[t] f32 values, [t] int64 positions -> int64 (order key << 27) | position: NaN above +Inf, -0 == +0"""
    b = value.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where(b >= 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    key = torch.where(torch.isnan(value), torch.full_like(key, 0xFFFFFFFF), key)
    return (key << 27) | pos


def exact(pq, codes, scales, table, list_off_host, probe_row, got_v, got_i, k, ip):
    """one query's result against scan + exact selection over the rows of its probed lists"""
    pos = torch.cat([torch.arange(int(list_off_host[l]), int(list_off_host[l + 1]), device="cuda")
                     for l in probe_row.tolist()])
    v = pq.adc_scan_device(codes[pos], table)
    if ip:
        v = v * scales[pos]
    kk = min(k, pos.numel())
    want = torch.topk(keys_of(-v if ip else v, pos), kk, largest=False, sorted=True).values & ((1 << 27) - 1)
    ok = bool(torch.equal(got_i[:kk], want)) and bool((got_i[kk:] == -1).all())
    all_v = torch.zeros(codes.shape[0], dtype=torch.float32, device="cuda")
    all_v[pos] = v
    want_v = all_v[want] + 0.0 if ip else all_v[want]
    return ok and bool(torch.equal(got_v[:kk].view(torch.int32), want_v.view(torch.int32)))


def synthetic_lists(rng, n, n_lists):
    w = rng.lognormal(0.0, 0.5, n_lists)
    sizes = np.floor(w / w.sum() * n).astype(np.int64)
    sizes[0] += n - sizes.sum()
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), sizes


def timing(res):
    assert N < (1 << 27)
    rng = np.random.default_rng(11)
    pq = ra.Pq(None, rng.standard_normal((M, K, DSUB), dtype=np.float32))
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    scales = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda()
    off_host, sizes = synthetic_lists(rng, N, N_LISTS)
    list_off = torch.from_numpy(off_host).cuda()
    res["lists"] = {"n_lists": N_LISTS, "assignment": "synthetic: sizes ~ log-normal(0, 0.5), rows of a list contiguous",
                    "size_min": int(sizes.min()), "size_median": int(np.median(sizes)), "size_max": int(sizes.max())}
    ys = torch.from_numpy(rng.standard_normal((max(NQS), M * DSUB), dtype=np.float32)).cuda()
    tabs = {False: pq.adc_tables_device(ys), True: pq.adc_ip_tables_device(ys)}

    def lists(ip, t, pr, k, check=False):
        if ip:
            return pq.adc_ip_search_lists_device(codes, t, list_off, pr, k, scales=scales, check=check)
        return pq.adc_search_lists_device(codes, t, list_off, pr, k, check=check)

    def exhaustive(ip, t, k):
        if ip:
            return pq.adc_ip_search_device(codes, t, k, scales=scales)
        return pq.adc_search_device(codes, t, k)

    for nq in NQS:
        for nprobe in NPROBES:
            probes = np.stack([rng.permutation(N_LISTS)[:nprobe] for _ in range(nq)]).astype(np.int64)
            pr = torch.from_numpy(probes).cuda()
            rows_mean = float(np.mean([sizes[p].sum() for p in probes]))
            for ip in (False, True):
                t = tabs[ip][:nq].contiguous()
                for k in KS:
                    ra.launch_log(reset=True)
                    v, i = lists(ip, t, pr, k, check=True)
                    torch.cuda.synchronize()
                    log = ra.launch_log(reset=True)
                    ok = all(exact(pq, codes, scales, t[j].contiguous(), off_host, probes[j], v[j], i[j], k, ip)
                             for j in sorted({0, nq - 1}))
                    lists_ms, lists_all = timed(lambda: lists(ip, t, pr, k))
                    full_ms, full_all = timed(lambda: exhaustive(ip, t, k))
                    row = {"metric": "ip_scaled" if ip else "l2", "nq": nq, "nprobe": nprobe, "k": k,
                           "probed_rows_mean": round(rows_mean), "lists_ms": round(lists_ms, 4),
                           "exhaustive_ms": round(full_ms, 4), "lists_over_exhaustive": round(lists_ms / full_ms, 4),
                           "exact": ok, "lists_launches": log, "all_ms": {"lists": lists_all, "exhaustive": full_all}}
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)
    # workgroups per query: one latency cell, forced counts against the automatic choice
    probes = torch.from_numpy(rng.permutation(N_LISTS)[None, :64].astype(np.int64)).cuda()
    t = tabs[False][:1].contiguous()
    sweep = []
    try:
        for g in (0, 16, 32, 64, 128, 256, 512, 1024):
            ra.set_option("adc_lists_wgs_per_query", g)
            ms, all_ms = timed(lambda: lists(False, t, probes, 10))
            sweep.append({"wgs_per_query": g or "auto", "lists_ms": round(ms, 4), "all_ms": all_ms})
            print(json.dumps(sweep[-1]), flush=True)
    finally:
        ra.set_option("adc_lists_wgs_per_query", 0)
    res["wgs_per_query_sweep"] = {"metric": "l2", "nq": 1, "nprobe": 64, "k": 10, "runs": sweep}
    del codes, scales
    torch.cuda.empty_cache()


def recall(res):
    """1 M rows around 512 centres, a trained 15 x 256 quantizer, 256 lists trained on the vectors: recall@10 of the list
    search against the exhaustive ADC search (the same codes, so nprobe = n_lists gives 1)"""
    from reductive_amd import qmatrix
    n, d, n_lists, nq, k = 1_000_000, 60, 256, 256, 10
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((512, d), dtype=np.float32) * np.float32(2.0)
    x = centres[rng.integers(0, 512, n)] + rng.standard_normal((n, d), dtype=np.float32)
    pq = ra.train_pq(15, 8, 5, 1, x[:200_000], rng=rng)
    xd = torch.from_numpy(x).cuda()
    codes = pq.quantize_batch_device(xd)
    qm = qmatrix.QuantizedMatrix(pq, codes.cpu().numpy())
    pm = qm.partition(n_lists, n_iterations=10, vectors=xd, train_rows=200_000, rng=rng)
    sizes = np.diff(pm.list_off.cpu().numpy())
    ys = torch.from_numpy(x[rng.integers(0, n, nq)] + np.float32(0.3) * rng.standard_normal((nq, d), dtype=np.float32)).cuda()
    _, want = pq.adc_search_device(qm.codes, pq.adc_tables_device(ys), k)
    runs = []
    for nprobe in (1, 2, 4, 8, 16, 32, 64, 256):
        _, got = pm.nearest(ys, k, nprobe)
        hit = (got[:, :, None] == want[:, None, :]).any(dim=2).float().mean().item()
        runs.append({"nprobe": nprobe, "recall_at_10": round(hit, 4)})
        print(json.dumps(runs[-1]), flush=True)
    res["trained_case"] = {"n": n, "d": d, "M": 15, "K": 256, "n_lists": n_lists, "queries": nq,
                           "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
                           "note": "recall@10 against the exhaustive ADC search over the same codes; information only",
                           "runs": runs}


def main():
    res = {"shape": {"n": N, "M": M, "K": K}, "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0),
           "runs": []}
    timing(res)
    recall(res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "list search differs from scan + selection over the probed rows"


if __name__ == "__main__":
    main()
