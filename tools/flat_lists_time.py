"""Exact search in probed lists (Pq.flat_search_lists_device, pqhip_flat_search_lists_f32_dev) against the only way to the
same result without it -- Pq.flat_search_device with the mask of the probed lists, one call per query -- and against the
unmasked exhaustive call, in one process on the same buffers, on one MI355X.

10 M standard-normal rows of d = 300, f32 and f16, in 1,024 lists of random lengths (a multinomial draw around the mean;
the rows are not clustered: the time of all three calls depends on the layout alone).  Per cell of nq in {1, 8, 64} x
nprobe in {1, 8, 64, 1,024} x k in {10, 100}, squared L2, distinct random lists per query: HIP events around the call,
median of 5 after 2 warm-up calls, for
    lists      flat_search_lists_device: plan + k_flat_search_lists + merge
    masked     flat_search_device(allow = the mask of query q's lists) for q = 0 .. nq - 1; the masks are packed outside
               the timing.  The results are compared with the lists' bit for bit in every cell.
    unmasked   flat_search_device over all rows, all queries in one call
Reported: both ratios, the spread (max - min of the 5) of the masked call, the probed bytes (sum over the queries of the
probed rows x d x element size) over the lists' time as a fraction of 8 TB/s, and the unmasked call's own fraction (the
matrix once over its time).  A cell with at most 1/8 of the lists probed whose lists time is not below the masked
median by more than the masked spread is listed under "findings".  One sweep of the forced workgroups per query
(option "flat_lists_wgs_per_query") at nq = 1 records what the host rule was not measured against.

Writes JSON (default profiles/flat_lists_search_time.json).

usage: python tools/flat_lists_time.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_lists_search_time.json")
N, D, LISTS = 10_000_000, 300, 1024
FORMS = ((torch.float32, "f32"), (torch.float16, "f16"))
NQS, NPROBES, KS = (1, 8, 64), (1, 8, 64, 1024), (10, 100)
SWEEP_G = (0, 1, 4, 16, 64, 256)
WARM, REPS = 2, 5
HBM_BYTES_PER_S = 8e12
OPTION = "flat_lists_wgs_per_query"


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


def masks_of(pq, off, probes):
    """the mask words of every query's probed lists"""
    words = []
    for row in probes.tolist():
        flags = torch.zeros(N, dtype=torch.bool, device="cuda")
        for l in row:
            flags[off[l]:off[l + 1]] = True
        words.append(pq.pack_row_mask_device(flags))
    return words


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "d": D, "n_lists": LISTS, "warmup": WARM, "reps": REPS,
           "masked_baseline": "flat_search_device with the mask of the probed lists, one call per query, masks packed before",
           "runs": [], "findings": [], "wgs_per_query_sweep": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    pq = ra.Pq(None, np.zeros((1, 1, D), np.float32))
    rng = np.random.default_rng(41)
    off = np.zeros(LISTS + 1, np.int64)
    np.cumsum(rng.multinomial(N, np.full(LISTS, 1.0 / LISTS)), out=off[1:])
    od = torch.from_numpy(off).cuda()
    ys = torch.from_numpy(rng.standard_normal((max(NQS), D), dtype=np.float32)).cuda()
    probes = {(nq, p): np.stack([rng.permutation(LISTS)[:p] for _ in range(nq)]).astype(np.int64) for nq in NQS for p in NPROBES}
    for dtype, name in FORMS:
        x = torch.empty((N, D), dtype=dtype, device="cuda")
        for r0 in range(0, N, 2_000_000):
            x[r0:r0 + 2_000_000].normal_()
        matrix_bytes = N * D * x.element_size()
        for nq in NQS:
            q = ys[:nq].contiguous()
            unmasked = {k: timed(lambda: pq.flat_search_device(q, x, k)) for k in KS}
            for p in NPROBES:
                pr = probes[(nq, p)]
                pd = torch.from_numpy(pr).cuda()
                words = masks_of(pq, off, pr)
                probed_rows = int(sum(int(off[l + 1] - off[l]) for row in pr.tolist() for l in row))
                for k in KS:
                    ra.launch_log(reset=True)
                    v, i = pq.flat_search_lists_device(q, x, od, pd, k, check=True)
                    log = ra.launch_log(reset=True)
                    for j in range(nq):
                        wv, wi = pq.flat_search_device(q[j], x, k, allow=words[j])
                        assert torch.equal(i[j], wi) and torch.equal(v[j].view(torch.int32), wv.view(torch.int32))
                    ms_l, all_l = timed(lambda: pq.flat_search_lists_device(q, x, od, pd, k))
                    ms_m, all_m = timed(lambda: [pq.flat_search_device(q[j], x, k, allow=words[j]) for j in range(nq)])
                    ms_u, all_u = unmasked[k]
                    spread = max(all_m) - min(all_m)
                    probed_bytes = probed_rows * D * x.element_size()
                    row = {"vectors": name, "nq": nq, "nprobe": p, "k": k, "probed_rows": probed_rows,
                           "ms": {"lists": round(ms_l, 4), "masked": round(ms_m, 4), "unmasked": round(ms_u, 4)},
                           "lists_over_masked": round(ms_l / ms_m, 4), "lists_over_unmasked": round(ms_l / ms_u, 4),
                           "masked_spread_ms": round(spread, 4), "probed_bytes": probed_bytes,
                           "lists_fraction_of_8TBps": round(probed_bytes / (ms_l * 1e-3) / HBM_BYTES_PER_S, 5),
                           "unmasked_fraction_of_8TBps": round(matrix_bytes / (ms_u * 1e-3) / HBM_BYTES_PER_S, 5),
                           "launches": log, "all_ms": {"lists": all_l, "masked": all_m, "unmasked": all_u}}
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)
                    if p * 8 <= LISTS and not ms_l < ms_m - spread:
                        res["findings"].append({key: row[key] for key in ("vectors", "nq", "nprobe", "k", "ms", "masked_spread_ms")})
                    with open(OUT, "w") as f:
                        json.dump(res, f, indent=1)
        q = ys[:1].contiguous()
        try:
            for p in (8, 64, 1024):
                pd = torch.from_numpy(probes[(1, p)]).cuda()
                for g in SWEEP_G:
                    ra.set_option(OPTION, g)
                    ms, all_ms = timed(lambda: pq.flat_search_lists_device(q, x, od, pd, 10))
                    row = {"vectors": name, "nq": 1, "nprobe": p, "k": 10, "forced_wgs_per_query": g, "ms": round(ms, 4), "all_ms": all_ms}
                    print(json.dumps(row), flush=True)
                    res["wgs_per_query_sweep"].append(row)
        finally:
            ra.set_option(OPTION, 0)
        del x
        torch.cuda.empty_cache()
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
