"""Masked ADC searches against the unmasked searches of the same run on the same data: 100 M resident rows, M = 15,
K = 256, the synthetic 1,024 lists of tools/adc_list_search_time.py, masks of density 1.0 (all ones), 0.5 and 0.01 (rows
drawn independently).  Cells: exhaustive L2 and scaled IP at 1 / 8 / 32 queries and k = 10 / 100; list L2 and residual
list L2 at 1 / 8 / 256 queries, nprobe = 8 / 64, k = 10.  HIP events, median of 7 after 2 warm-up calls, masked and
unmasked in one process.  Every masked cell is checked on the device for its first and last query against
adc_scan_device over the gathered allowed rows (of the probed lists) + an exact selection (torch.topk over the distinct
64-bit keys (order key << 27) | position).

The expectation, set from the bytes before anything was measured, is recorded per cell as `within`:
  density 1.0:        masked <= unmasked * (B + 1/8) / B + (max - min of the unmasked cell's seven timings), B = 15 bytes
                      per row, 19 with a scale or a row term;
  density 0.5, 0.01:  masked <= the all-ones masked cell.
Information, not an assertion; the run only fails when a result is not exact.  Writes JSON (default
profiles/adc_masked_search_time.json).

usage: python tools/adc_masked_search_time.py [out.json] [n_rows]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_masked_search_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
M, K, DSUB = 15, 256, 20
N_LISTS = 1024
DENSITIES = (1.0, 0.5, 0.01)


def select(value, pos, k, ip):
    """the first k of the rows `pos` with values `value` under (key, position) -> (values, positions)"""
    kk = min(k, pos.numel())
    top = torch.topk(keys_of(-value if ip else value, pos), kk, largest=False, sorted=True)
    v = value[top.indices]
    return (v + 0.0 if ip else v), top.values & ((1 << 27) - 1)


def same(got_v, got_i, want_v, want_i):
    kk = want_i.numel()
    return (bool(torch.equal(got_i[:kk], want_i)) and bool((got_i[kk:] == -1).all())
            and bool(torch.equal(got_v[:kk].view(torch.int32), want_v.view(torch.int32))))


def expectation(row, unmasked_all, ones_ms, bytes_per_row):
    if row["density"] == 1.0:
        bound = row["unmasked_ms"] * (bytes_per_row + 0.125) / bytes_per_row + (max(unmasked_all) - min(unmasked_all))
    else:
        bound = ones_ms
    row["expected_at_most_ms"] = round(bound, 4)
    row["within"] = bool(row["masked_ms"] <= bound)


def main():
    assert N < (1 << 27)
    res = {"shape": {"n": N, "M": M, "K": K, "n_lists": N_LISTS}, "warmup": 2, "reps": 7,
           "device": torch.cuda.get_device_name(0), "densities": list(DENSITIES), "runs": []}
    rng = np.random.default_rng(11)
    pq = ra.Pq(None, rng.standard_normal((M, K, DSUB), dtype=np.float32))
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    scales = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda()
    terms = torch.from_numpy(rng.uniform(0.0, 4.0, N).astype(np.float32)).cuda()
    off_host, sizes = synthetic_lists(rng, N, N_LISTS)
    list_off = torch.from_numpy(off_host).cuda()
    ys = torch.from_numpy(rng.standard_normal((256, M * DSUB), dtype=np.float32)).cuda()
    tabs = {False: pq.adc_tables_device(ys), True: pq.adc_ip_tables_device(ys)}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    masks = {}
    for dens in DENSITIES:
        allow = torch.ones(N, dtype=torch.bool, device="cuda") if dens == 1.0 else torch.rand(N, device="cuda", generator=gen) < dens
        masks[dens] = (allow, pq.pack_row_mask_device(allow))
    res["allowed_rows"] = {str(d): int(masks[d][0].sum()) for d in DENSITIES}

    # ---- exhaustive: L2 and scaled IP ----
    for ip in (False, True):
        bytes_per_row = 19 if ip else 15
        for nq in (1, 8, 32):
            t = tabs[ip][:nq].contiguous()
            for k in (10, 100):
                def run(words, t=t, k=k, ip=ip):
                    if ip:
                        return pq.adc_ip_search_device(codes, t, k, scales=scales, allow=words)
                    return pq.adc_search_device(codes, t, k, allow=words)
                un_ms, un_all = timed(lambda: run(None))
                ones_ms = None
                for dens in DENSITIES:
                    allow, words = masks[dens]
                    ra.launch_log(reset=True)
                    v, i = run(words)
                    torch.cuda.synchronize()
                    log = ra.launch_log(reset=True)
                    pos = torch.nonzero(allow).flatten()
                    sub = codes[pos]
                    ok = True
                    for j in sorted({0, nq - 1}):
                        val = pq.adc_scan_device(sub, t[j].contiguous())
                        if ip:
                            val = val * scales[pos]
                        ok = ok and same(v[j], i[j], *select(val, pos, k, ip))
                        del val
                    del sub, pos
                    ms, all_ms = timed(lambda: run(words))
                    ones_ms = ms if dens == 1.0 else ones_ms
                    row = {"search": "exhaustive", "metric": "ip_scaled" if ip else "l2", "nq": nq, "k": k, "density": dens,
                           "masked_ms": round(ms, 4), "unmasked_ms": round(un_ms, 4), "masked_over_unmasked": round(ms / un_ms, 4),
                           "exact": ok, "launches": log, "all_ms": {"masked": all_ms, "unmasked": un_all}}
                    expectation(row, un_all, ones_ms, bytes_per_row)
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)

    # ---- lists: L2 over the codes themselves, and L2 over residual codes (probe bias + row term) ----
    k = 10
    for residual in (False, True):
        bytes_per_row = 19 if residual else 15
        for nq in (1, 8, 256):
            t = tabs[residual][:nq].contiguous()            # the residual search reads the inner-product tables
            for nprobe in (8, 64):
                probes = np.stack([rng.permutation(N_LISTS)[:nprobe] for _ in range(nq)]).astype(np.int64)
                pr = torch.from_numpy(probes).cuda()
                bias = torch.from_numpy(rng.uniform(0.0, 8.0, probes.shape).astype(np.float32)).cuda()

                def run(words, t=t, pr=pr, bias=bias, residual=residual):
                    if residual:
                        return pq.adc_search_lists_residual_device(codes, t, list_off, pr, bias, terms, k, allow=words)
                    return pq.adc_search_lists_device(codes, t, list_off, pr, k, allow=words)
                un_ms, un_all = timed(lambda: run(None))
                ones_ms = None
                for dens in DENSITIES:
                    allow, words = masks[dens]
                    ra.launch_log(reset=True)
                    v, i = run(words)
                    torch.cuda.synchronize()
                    log = ra.launch_log(reset=True)
                    ok = True
                    for j in sorted({0, nq - 1}):
                        pos = torch.cat([torch.arange(int(off_host[l]), int(off_host[l + 1]), device="cuda") for l in probes[j].tolist()])
                        b = torch.cat([bias[j, p].expand(int(sizes[l])) for p, l in enumerate(probes[j].tolist())])
                        keep = allow[pos]
                        pos, b = pos[keep], b[keep]
                        s = pq.adc_scan_device(codes[pos], t[j].contiguous())
                        val = (b + terms[pos]) - (s + s) if residual else s
                        ok = ok and same(v[j], i[j], *select(val, pos, k, False))
                    ms, all_ms = timed(lambda: run(words))
                    ones_ms = ms if dens == 1.0 else ones_ms
                    row = {"search": "lists_residual" if residual else "lists", "metric": "l2", "nq": nq, "nprobe": nprobe, "k": k,
                           "density": dens, "masked_ms": round(ms, 4), "unmasked_ms": round(un_ms, 4),
                           "masked_over_unmasked": round(ms / un_ms, 4), "exact": ok, "launches": log,
                           "all_ms": {"masked": all_ms, "unmasked": un_all}}
                    expectation(row, un_all, ones_ms, bytes_per_row)
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)

    res["outside_expectation"] = [{key: r[key] for key in ("search", "metric", "nq", "nprobe", "k", "density", "masked_ms",
                                                           "expected_at_most_ms") if key in r}
                                  for r in res["runs"] if not r["within"]]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "a masked search differs from scan + selection over the allowed rows"


if __name__ == "__main__":
    main()
