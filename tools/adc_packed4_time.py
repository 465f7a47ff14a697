"""Searches over 4-bit packed codes against the u8 searches of the same run on the unpacked codes: 100 M resident rows,
K = 16, M = 16 (d = 128, the reference's criterion shape) and M = 48 (d = 768), the synthetic 1,024 lists of
tools/adc_list_search_time.py.  Cells: exhaustive L2 and scaled IP at 1 / 8 / 32 queries and k = 10 / 100; list L2 and
residual list L2 at 1 / 8 / 256 queries, nprobe = 8 / 64, k = 10; pack and unpack of the whole matrix beside a
device-to-device copy of the same output bytes.  HIP events, median of 7 after 2 warm-up calls, packed and u8 in one
process.  The baseline of a search cell is the existing u8 search of the same shape on the unpacked codes, never the packed
code itself; before a cell is timed, the packed result of its first and last query must equal the u8 result bit for bit.

The expectation, set from the bytes before anything was measured, is recorded per cell as `within`:
  packed <= u8 + (max - min of the u8 cell's seven timings);
`ratio` = packed / u8 is recorded beside `byte_ratio` = (ceil(M / 2) + e) / (M + e), e = 4 with a scale or a row term, to
which it should tend where the u8 search is HBM-bound.  Information, not an assertion; the run only fails when a result is
not exact.  Writes JSON (default profiles/adc_packed4_time.json).

usage: python tools/adc_packed4_time.py [out.json] [n_rows] [M ...]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_packed4_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
MS = [int(a) for a in sys.argv[3:]] or [16, 48]
K = 16
DSUB = {16: 8, 48: 16}
N_LISTS = 1024


def same(got, want, rows):
    return all(bool(torch.equal(g[j], w[j])) for g, w in ((got[0].view(torch.int32), want[0].view(torch.int32)), (got[1], want[1]))
               for j in rows)


def cell(res, row, run, extra_bytes, M, nq):
    """times run(packed=False) and run(packed=True) after checking the first and the last query"""
    ra.launch_log(reset=True)
    got = run(True)
    torch.cuda.synchronize()
    log = ra.launch_log(reset=True)
    want = run(False)
    row["exact"] = same(got, want, sorted({0, nq - 1}))
    del got, want
    u8_ms, u8_all = timed(lambda: run(False))
    p4_ms, p4_all = timed(lambda: run(True))
    spread = max(u8_all) - min(u8_all)
    row.update({"packed_ms": round(p4_ms, 4), "u8_ms": round(u8_ms, 4), "ratio": round(p4_ms / u8_ms, 4),
                "byte_ratio": round(((M + 1) // 2 + extra_bytes) / (M + extra_bytes), 4), "u8_spread_ms": round(spread, 4),
                "within": bool(p4_ms <= u8_ms + spread), "launches": log, "all_ms": {"packed": p4_all, "u8": u8_all}})
    print(json.dumps(row), flush=True)
    res["runs"].append(row)


def shape(res, M):
    rng = np.random.default_rng(11 + M)
    dsub = DSUB.get(M, 8)
    pq = ra.Pq(None, rng.standard_normal((M, K, dsub), dtype=np.float32))
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda")
    packed = torch.empty((N, (M + 1) // 2), dtype=torch.uint8, device="cuda")

    # ---- pack and unpack of the whole matrix beside a copy of the same output bytes ----
    pq.pack_codes4_device(codes, out=packed, check=True)
    back = torch.empty_like(codes)
    pq.unpack_codes4_device(packed, out=back, check=True)
    exact = bool(torch.equal(back, codes))
    other = torch.empty_like(packed)
    for name, fn, copy, nbytes in (("pack", lambda: pq.pack_codes4_device(codes, out=packed), lambda: other.copy_(packed), packed.numel()),
                                   ("unpack", lambda: pq.unpack_codes4_device(packed, out=back), lambda: back.copy_(codes), codes.numel())):
        ms, all_ms = timed(fn)
        copy_ms, copy_all = timed(copy)
        row = {"step": name, "M": M, "ms": round(ms, 4), "copy_ms": round(copy_ms, 4), "over_copy": round(ms / copy_ms, 4),
               "output_bytes": nbytes, "output_GBps": round(nbytes / ms / 1e6, 1), "exact": exact,
               "all_ms": {"step": all_ms, "copy": copy_all}}
        print(json.dumps(row), flush=True)
        res["convert"].append(row)
    del back, other

    scales = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).cuda()
    terms = torch.from_numpy(rng.uniform(0.0, 4.0, N).astype(np.float32)).cuda()
    off_host, _ = synthetic_lists(rng, N, N_LISTS)
    list_off = torch.from_numpy(off_host).cuda()
    ys = torch.from_numpy(rng.standard_normal((256, M * dsub), dtype=np.float32)).cuda()
    tabs = {False: pq.adc_tables_device(ys), True: pq.adc_ip_tables_device(ys)}

    # ---- exhaustive: L2 and scaled IP ----
    for ip in (False, True):
        for nq in (1, 8, 32):
            t = tabs[ip][:nq].contiguous()
            for k in (10, 100):
                def run(p4, t=t, k=k, ip=ip):
                    c = packed if p4 else codes
                    if ip:
                        return pq.adc_ip_search_device(c, t, k, scales=scales, packed4=p4)
                    return pq.adc_search_device(c, t, k, packed4=p4)
                cell(res, {"search": "exhaustive", "metric": "ip_scaled" if ip else "l2", "M": M, "nq": nq, "k": k}, run,
                     4 if ip else 0, M, nq)

    # ---- lists: L2 over the codes themselves, and L2 over residual codes (probe bias + row term) ----
    k = 10
    for residual in (False, True):
        for nq in (1, 8, 256):
            t = tabs[residual][:nq].contiguous()            # the residual search reads the inner-product tables
            for nprobe in (8, 64):
                probes = np.stack([rng.permutation(N_LISTS)[:nprobe] for _ in range(nq)]).astype(np.int64)
                pr = torch.from_numpy(probes).cuda()
                bias = torch.from_numpy(rng.uniform(0.0, 8.0, probes.shape).astype(np.float32)).cuda()

                def run(p4, t=t, pr=pr, bias=bias, residual=residual):
                    c = packed if p4 else codes
                    if residual:
                        return pq.adc_search_lists_residual_device(c, t, list_off, pr, bias, terms, k, packed4=p4)
                    return pq.adc_search_lists_device(c, t, list_off, pr, k, packed4=p4)
                cell(res, {"search": "lists_residual" if residual else "lists", "metric": "l2", "M": M, "nq": nq,
                           "nprobe": nprobe, "k": k}, run, 4 if residual else 0, M, nq)


def main():
    assert N < (1 << 31)
    res = {"shape": {"n": N, "K": K, "M": MS, "n_lists": N_LISTS}, "warmup": 2, "reps": 7,
           "device": torch.cuda.get_device_name(0), "convert": [], "runs": []}
    for M in MS:
        shape(res, M)
        torch.cuda.empty_cache()
    res["outside_expectation"] = [{key: r[key] for key in ("search", "metric", "M", "nq", "nprobe", "k", "packed_ms", "u8_ms",
                                                           "u8_spread_ms", "ratio") if key in r}
                                  for r in res["runs"] if not r["within"]]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"] + res["convert"]), "a packed result differs from the u8 result"


if __name__ == "__main__":
    main()
