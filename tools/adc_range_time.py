"""ADC range searches against what a caller had before them: 100 M resident rows, M = 15, K = 256, the synthetic 1,024
lists of tools/adc_list_search_time.py.  Cells: exhaustive L2 and scaled IP at 1 / 8 / 32 queries; flat and residual list
L2 at 1 / 8 / 256 queries, nprobe = 8 / 64; per cell three thresholds, set per query from a sample of rows so that about
1e-5, 1e-3 and 1e-2 of the (probed) rows qualify.  HIP events, median of 7 after 2 warm-up calls.  Every cell's first and
last query is checked on the device against adc_scan_device + compare (+ nonzero: ascending rows / the concatenation's
order).  The range call is timed through Pq.adc_*range*_device with a capacity that holds the result, i.e. count, scan and
fill plus the one read of the total.

Exhaustive cells are also measured, in the same process, against the PARENT'S COMPOSITION -- adc_scan_device -> compare
(NaN-safe: a comparison is false for NaN) -> nonzero -> gather of the values -- and against the top-k search of the same
cell with k = 10.  The expectation, written down from the bytes before any run, is recorded per cell:
  within_composition:  range <= composition
  within_search:       range <= 2 * search(k = 10) + (max - min of the search's seven timings)
Information, not an assertion; the run only fails when a result is not exact.  Writes JSON (default
profiles/adc_range_time.json).  Run each step under a time limit of its own, e.g. `timeout 900 python tools/adc_range_time.py`.

usage: python tools/adc_range_time.py [out.json] [n_rows] [exhaustive|lists|all]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_list_search_time import synthetic_lists  # noqa: E402
from adc_search_time import timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_range_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
WHAT = sys.argv[3] if len(sys.argv) > 3 else "all"
M, K, DSUB = 15, 256, 20
N_LISTS = 1024
FRACTIONS = (1e-5, 1e-3, 1e-2)
SAMPLE = 1 << 20


def quantiles(sample, ip):
    """sample [nq, s] of values -> {fraction: thr [nq]} so that about that fraction of rows qualifies"""
    s = torch.sort(sample, dim=1, descending=ip).values
    return {f: s[:, max(int(f * s.shape[1]) - 1, 0)].contiguous() for f in FRACTIONS}


def main():
    res = {"shape": {"n": N, "M": M, "K": K, "n_lists": N_LISTS}, "warmup": 2, "reps": 7,
           "device": torch.cuda.get_device_name(0), "fractions": list(FRACTIONS), "runs": []}
    rng = np.random.default_rng(11)
    pq = ra.Pq(None, rng.standard_normal((M, K, DSUB), dtype=np.float32))
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    scales = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda()
    terms = torch.from_numpy(rng.uniform(0.0, 4.0, N).astype(np.float32)).cuda()
    off_host, sizes = synthetic_lists(rng, N, N_LISTS)
    list_off = torch.from_numpy(off_host).cuda()
    ys = torch.from_numpy(rng.standard_normal((256, M * DSUB), dtype=np.float32)).cuda()
    tabs = {False: pq.adc_tables_device(ys), True: pq.adc_ip_tables_device(ys)}
    srows = torch.randint(0, N, (min(SAMPLE, N),), device="cuda")

    # ---- exhaustive: L2 and scaled IP, against the composition and the top-k search ----
    for ip in (False, True) if WHAT in ("all", "exhaustive") else ():
        for nq in (1, 8, 32):
            t = tabs[ip][:nq].contiguous()
            sample = pq.adc_scan_device(codes[srows], t)
            if ip:
                sample = sample * scales[srows]
            thr_of = quantiles(sample, ip)
            del sample

            def search(t=t, ip=ip):
                return pq.adc_ip_search_device(codes, t, 10, scales=scales) if ip else pq.adc_search_device(codes, t, 10)
            s_ms, s_all = timed(search)
            for frac in FRACTIONS:
                thr = thr_of[frac]

                def run(cap=None, t=t, thr=thr, ip=ip):
                    if ip:
                        return pq.adc_ip_range_device(codes, t, thr, scales=scales, capacity=cap)
                    return pq.adc_range_device(codes, t, thr, capacity=cap)

                def composition(t=t, thr=thr, ip=ip, nq=nq):
                    v = pq.adc_scan_device(codes, t).reshape(nq, -1)
                    rows, vals = [], []
                    for j in range(nq):                                            # per query: nonzero of one row of the matrix
                        vj = v[j] * scales if ip else v[j]
                        r = torch.nonzero((vj >= thr[j]) if ip else (vj <= thr[j])).flatten()   # false for NaN on either side
                        rows.append(r)
                        vals.append(vj[r])
                    return rows, vals
                ra.launch_log(reset=True)
                lims, val, idx = run()
                torch.cuda.synchronize()
                log = ra.launch_log(reset=True)
                total = int(lims[-1])
                rows, vals = composition()
                counts = torch.tensor([0] + [r.numel() for r in rows], device="cuda")
                ok = bool(torch.equal(lims, torch.cumsum(counts, 0))) and bool(torch.equal(idx, torch.cat(rows)))
                ok = ok and bool(torch.equal(val.view(torch.int32), torch.cat(vals).view(torch.int32)))
                del rows, vals
                cap = max(total, 1)
                r_ms, r_all = timed(lambda: run(cap))
                c_ms, c_all = timed(composition)
                torch.cuda.empty_cache()
                row = {"search": "exhaustive", "metric": "ip_scaled" if ip else "l2", "nq": nq, "fraction": frac, "hits": total,
                       "range_ms": round(r_ms, 4), "composition_ms": round(c_ms, 4), "search_k10_ms": round(s_ms, 4),
                       "range_over_composition": round(r_ms / c_ms, 4), "range_over_search": round(r_ms / s_ms, 4),
                       "within_composition": bool(r_ms <= c_ms),
                       "within_search": bool(r_ms <= 2 * s_ms + (max(s_all) - min(s_all))),
                       "exact": ok, "launches": log, "all_ms": {"range": r_all, "composition": c_all, "search": s_all}}
                print(json.dumps(row), flush=True)
                res["runs"].append(row)

    # ---- lists: L2 over the codes themselves, and L2 over residual codes ----
    for residual in (False, True) if WHAT in ("all", "lists") else ():
        for nq in (1, 8, 256):
            t = tabs[residual][:nq].contiguous()            # the residual search reads the inner-product tables
            for nprobe in (8, 64):
                probes = np.stack([rng.permutation(N_LISTS)[:nprobe] for _ in range(nq)]).astype(np.int64)
                pr = torch.from_numpy(probes).cuda()
                bias = torch.from_numpy(rng.uniform(0.0, 8.0, probes.shape).astype(np.float32)).cuda()

                def values_of(j, t=t, probes=probes, bias=bias, residual=residual):
                    pos = torch.cat([torch.arange(int(off_host[l]), int(off_host[l + 1]), device="cuda") for l in probes[j].tolist()])
                    s = pq.adc_scan_device(codes[pos], t[j].contiguous())
                    if not residual:
                        return pos, s
                    b = torch.cat([bias[j, p].expand(int(sizes[l])) for p, l in enumerate(probes[j].tolist())])
                    return pos, (b + terms[pos]) - (s + s)
                # thresholds per query from the probed rows of the first query's lists (the tables differ per query)
                thr_of = {f: [] for f in FRACTIONS}
                for j in range(nq):
                    _, v = values_of(j) if j in (0, nq - 1) or nq <= 8 else (None, None)
                    if v is None:                            # the other queries of a large batch: the first query's level
                        for f in FRACTIONS:
                            thr_of[f].append(thr_of[f][0])
                        continue
                    qs = quantiles(v[None][:, :SAMPLE], False)
                    for f in FRACTIONS:
                        thr_of[f].append(float(qs[f][0]))

                def search(t=t, pr=pr, bias=bias, residual=residual):
                    if residual:
                        return pq.adc_search_lists_residual_device(codes, t, list_off, pr, bias, terms, 10)
                    return pq.adc_search_lists_device(codes, t, list_off, pr, 10)
                s_ms, s_all = timed(search)
                for frac in FRACTIONS:
                    thr = torch.tensor(thr_of[frac], dtype=torch.float32, device="cuda")

                    def run(cap=None, t=t, pr=pr, bias=bias, thr=thr, residual=residual):
                        if residual:
                            return pq.adc_range_lists_residual_device(codes, t, list_off, pr, bias, terms, thr, capacity=cap)
                        return pq.adc_range_lists_device(codes, t, list_off, pr, thr, capacity=cap)
                    ra.launch_log(reset=True)
                    lims, val, idx = run()
                    torch.cuda.synchronize()
                    log = ra.launch_log(reset=True)
                    total = int(lims[-1])
                    ok = True
                    for j in sorted({0, nq - 1}):
                        pos, v = values_of(j)
                        hit = torch.nonzero(v <= thr[j]).flatten()
                        a, b = int(lims[j]), int(lims[j + 1])
                        ok = ok and b - a == hit.numel() and bool(torch.equal(idx[a:b], pos[hit]))
                        ok = ok and bool(torch.equal(val[a:b].view(torch.int32), v[hit].view(torch.int32)))
                    cap = max(total, 1)
                    r_ms, r_all = timed(lambda: run(cap))
                    row = {"search": "lists_residual" if residual else "lists", "metric": "l2", "nq": nq, "nprobe": nprobe,
                           "fraction": frac, "hits": total, "range_ms": round(r_ms, 4), "search_k10_ms": round(s_ms, 4),
                           "range_over_search": round(r_ms / s_ms, 4),
                           "within_search": bool(r_ms <= 2 * s_ms + (max(s_all) - min(s_all))),
                           "exact": ok, "launches": log, "all_ms": {"range": r_all, "search": s_all}}
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)

    res["outside_expectation"] = [{key: r[key] for key in ("search", "metric", "nq", "nprobe", "fraction", "range_ms", "composition_ms",
                                                           "search_k10_ms", "within_composition", "within_search") if key in r}
                                  for r in res["runs"] if not (r.get("within_composition", True) and r["within_search"])]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "a range search differs from scan + compare"


if __name__ == "__main__":
    main()
