"""ADC list searches over residual codes against the plain list searches of the same run on the same data: the matrix of
tools/adc_list_search_time.py (100 M resident rows, M = 15, K = 256, 1,024 lists with log-normal sizes, random distinct
probes per query, scales uniform in [0.5, 2)), plus one f32 row term per row and one f32 bias per (query, probe slot),
both random: timing needs no trained quantizer.  Per cell of nq in {1, 8, 256} x nprobe in {1, 8, 64, 1024} x k in
{10, 100}, in one process: adc_search_lists_device (L2), adc_ip_search_lists_device with scales, and the two residual
searches (the similarity one with scales), HIP events, median of 7 after 2 warm-up calls.  The biases are uniform in
[0, 60), about the spread of a row sum, so the selection's threshold meets a jump at every list boundary; both residual
searches are timed a second time under one constant bias, which has no such jump ("..._const_bias").  Both residual results of
every cell are checked on the device for the first and last query: adc_scan_device over the gathered probed rows, the
two formulas of include/pqhip.h in f32 (one rounded torch operation each) and an exact selection (torch.topk over the
distinct 64-bit keys (order key << 27) | position).

Expectation recorded per cell (not asserted): the residual distance search reads 19 bytes per row where the plain one
reads 15, so it should take at most 19/15 of the plain L2 list search plus the spread (max - min) of that cell's seven
plain timings; the residual similarity search with scales reads what the plain scaled one reads and should be within
that one's spread of it.

A trained case with the project's own trainers (20,000 x 32 around 40 centres of scale 3, M = 8, 4 bits, 64 lists, 200
queries near data points, k = 10): mean squared reconstruction error and recall@10 against the true float64 neighbours,
for partition() over flat codes and for partition_residual(), per nprobe.  Writes JSON (default
profiles/adc_residual_search_time.json).

usage: python tools/adc_residual_search_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_list_search_time import keys_of, synthetic_lists  # noqa: E402
from adc_search_time import timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_residual_search_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
M, K, DSUB = 15, 256, 20
N_LISTS = 1024
NPROBES, NQS, KS = (1, 8, 64, 1024), (1, 8, 256), (10, 100)


def exact(pq, codes, extra, table, list_off_host, probe_row, bias_row, got_v, got_i, k, ip):
    """one query's residual result against scan + the header's formulas + exact selection over its probed rows"""
    lists = probe_row.tolist()
    pos = torch.cat([torch.arange(int(list_off_host[l]), int(list_off_host[l + 1]), device="cuda") for l in lists])
    sizes = torch.tensor([int(list_off_host[l + 1] - list_off_host[l]) for l in lists], device="cuda")
    b = torch.repeat_interleave(bias_row, sizes)
    s = pq.adc_scan_device(codes[pos], table)
    v = (b + s) * extra[pos] if ip else (b + extra[pos]) - (s + s)
    kk = min(k, pos.numel())
    want = torch.topk(keys_of(-v if ip else v, pos), kk, largest=False, sorted=True).values & ((1 << 27) - 1)
    ok = bool(torch.equal(got_i[:kk], want)) and bool((got_i[kk:] == -1).all())
    all_v = torch.zeros(codes.shape[0], dtype=torch.float32, device="cuda")
    all_v[pos] = v
    want_v = all_v[want] + 0.0
    return ok and bool(torch.equal(got_v[:kk].view(torch.int32), want_v.view(torch.int32)))


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
    t_l2, t_ip = pq.adc_tables_device(ys), pq.adc_ip_tables_device(ys)
    terms = torch.from_numpy(rng.uniform(0.0, 40.0, N).astype(np.float32)).cuda()

    for nq in NQS:
        for nprobe in NPROBES:
            probes = np.stack([rng.permutation(N_LISTS)[:nprobe] for _ in range(nq)]).astype(np.int64)
            pr = torch.from_numpy(probes).cuda()
            bias = torch.from_numpy(rng.uniform(0.0, 60.0, (nq, nprobe)).astype(np.float32)).cuda()
            flat = torch.full_like(bias, 30.0)
            rows_mean = float(np.mean([sizes[p].sum() for p in probes]))
            tl, ti = t_l2[:nq].contiguous(), t_ip[:nq].contiguous()
            for k in KS:
                calls = {
                    "l2": lambda: pq.adc_search_lists_device(codes, tl, list_off, pr, k),
                    "ip_scaled": lambda: pq.adc_ip_search_lists_device(codes, ti, list_off, pr, k, scales=scales),
                    "residual_l2": lambda: pq.adc_search_lists_residual_device(codes, ti, list_off, pr, bias, terms, k),
                    "residual_ip_scaled": lambda: pq.adc_ip_search_lists_residual_device(codes, ti, list_off, pr, bias, k,
                                                                                         scales=scales),
                }
                # the same two calls under one bias for every list: the threshold of the selection then meets no jump from
                # list to list, which separates what the kernel costs from what the values cost
                calls["residual_l2_const_bias"] = lambda: pq.adc_search_lists_residual_device(codes, ti, list_off, pr, flat, terms, k)
                calls["residual_ip_scaled_const_bias"] = lambda: pq.adc_ip_search_lists_residual_device(
                    codes, ti, list_off, pr, flat, k, scales=scales)
                ok, logs = {}, {}
                for name, ip in (("residual_l2", False), ("residual_ip_scaled", True)):
                    ra.launch_log(reset=True)
                    v, i = calls[name]()
                    torch.cuda.synchronize()
                    logs[name] = ra.launch_log(reset=True)
                    ok[name] = all(exact(pq, codes, scales if ip else terms, ti[j].contiguous(), off_host, probes[j], bias[j],
                                         v[j], i[j], k, ip) for j in sorted({0, nq - 1}))
                ms, all_ms = {}, {}
                for name, fn in calls.items():
                    ms[name], all_ms[name] = timed(fn)
                spread = {name: max(a) - min(a) for name, a in all_ms.items()}
                row = {"nq": nq, "nprobe": nprobe, "k": k, "probed_rows_mean": round(rows_mean),
                       "ms": {name: round(t, 4) for name, t in ms.items()},
                       "residual_l2_over_l2": round(ms["residual_l2"] / ms["l2"], 4),
                       "residual_ip_over_ip": round(ms["residual_ip_scaled"] / ms["ip_scaled"], 4),
                       "residual_l2_const_bias_over_l2": round(ms["residual_l2_const_bias"] / ms["l2"], 4),
                       "residual_ip_const_bias_over_ip": round(ms["residual_ip_scaled_const_bias"] / ms["ip_scaled"], 4),
                       "l2_spread_ms": round(spread["l2"], 4), "ip_scaled_spread_ms": round(spread["ip_scaled"], 4),
                       "residual_l2_within_expectation": bool(ms["residual_l2"] <= ms["l2"] * 19.0 / 15.0 + spread["l2"]),
                       "residual_ip_within_expectation": bool(ms["residual_ip_scaled"] <= ms["ip_scaled"] + spread["ip_scaled"]),
                       "exact": ok, "launches": logs, "all_ms": all_ms}
                print(json.dumps(row), flush=True)
                res["runs"].append(row)
    del codes, scales, terms
    torch.cuda.empty_cache()


def trained(res):
    """flat codes against residual codes at equal M, K, lists and nprobe, with the project's own trainers; the fixture
    and seeds of tests/test_gpu_adc_search_lists_residual.py"""
    from reductive_amd import qmatrix
    n, d, m, bits, n_lists, nq, k = 20000, 32, 8, 4, 64, 200, 10
    rng = np.random.default_rng(9830)
    centres = (rng.standard_normal((40, d)) * 3.0).astype(np.float32)
    x = (centres[rng.integers(0, 40, n)] + rng.standard_normal((n, d))).astype(np.float32)
    ys = (x[rng.choice(n, nq, replace=False)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    flat = ra.train_pq(m, bits, 10, 1, x, rng=np.random.default_rng(9831))
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x))
    pm = qm.partition(n_lists, vectors=x, rng=np.random.default_rng(9832))
    rm = qm.partition_residual(n_lists, vectors=x, rng=np.random.default_rng(9832))
    rows = torch.arange(n, device="cuda")
    x64, y64 = x.astype(np.float64), ys.astype(np.float64)
    mse = {"flat": float(((qm.embeddings(rows).cpu().numpy().astype(np.float64) - x64) ** 2).sum(1).mean()),
           "residual": float(((rm.embeddings(rows).cpu().numpy().astype(np.float64) - x64) ** 2).sum(1).mean())}
    d2 = (y64 ** 2).sum(1)[:, None] - 2.0 * y64 @ x64.T + (x64 ** 2).sum(1)[None]
    truth = np.argsort(d2, axis=1, kind="stable")[:, :k]
    yd = torch.from_numpy(ys).cuda()

    def recall(found):
        f = found.cpu().numpy()
        return float(np.mean([len(set(f[q].tolist()) & set(truth[q].tolist())) / k for q in range(nq)]))
    runs = []
    for nprobe in (1, 2, 4, 8, 16, 64):
        runs.append({"nprobe": nprobe, "recall_at_10_flat": round(recall(pm.nearest(yd, k, nprobe)[1]), 4),
                     "recall_at_10_residual": round(recall(rm.nearest(yd, k, nprobe)[1]), 4)})
        print(json.dumps(runs[-1]), flush=True)
    sizes = np.diff(rm.list_off.cpu().numpy())
    res["trained_case"] = {"n": n, "d": d, "M": m, "K": 1 << bits, "n_lists": n_lists, "queries": nq, "k": k,
                           "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
                           "mean_squared_reconstruction_error": {name: round(v, 4) for name, v in mse.items()},
                           "note": "recall@10 against the true float64 neighbours; flat = partition() over the codes of "
                                   "train_pq on the vectors, residual = partition_residual() with the same seeds",
                           "runs": runs}
    print(json.dumps(res["trained_case"]["mean_squared_reconstruction_error"]), flush=True)


def main():
    res = {"shape": {"n": N, "M": M, "K": K}, "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0),
           "expectation": "residual_l2 <= 19/15 l2 + spread(l2); residual_ip_scaled <= ip_scaled + spread(ip_scaled); "
                          "spread = max - min of the cell's seven plain timings", "runs": []}
    trained(res)
    timing(res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(all(r["exact"].values()) for r in res["runs"]), "residual search differs from scan + formulas + selection"


if __name__ == "__main__":
    main()
