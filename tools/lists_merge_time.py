"""The list merge (Pq.merge_lists_device) against its floor and against the torch formulation it replaces: 100 M resident
rows in 1,024 lists (sizes drawn from a log-normal, as tools/adc_list_search_time.py draws them) plus a batch of 10 k,
1 M or 10 M rows spread over the same lists, for the three row widths a partitioned matrix stores: 15-byte codes, 4-byte
norms / row terms and 8-byte ids / lists.  Per cell, in one process, HIP events, 2 warm-up calls, median of 7:
  merge   pq.merge_lists_device(list_off_a, a, list_off_b, b, out=out)            (plan + mover)
  copy    a device-to-device copy of as many bytes as the merge writes: the floor -- the merge reads and writes
          every byte once
  torch   torch.cat([a, b])[perm], perm the stable argsort of the concatenated list ids: timed with perm given
          ("gather") and with the sort ("sort + gather"); its peak extra device memory beside the inputs is recorded
          (the merge allocates its output and 32 bytes per list)
Every cell's merge is compared with the torch result, bit for bit, before it is timed.  One cell (15 bytes, 1 M rows) is
also timed for forced numbers of workgroups.  Writes JSON (default profiles/lists_merge_time.json) and prints the
table of DESIGN.md.

usage: python tools/lists_merge_time.py [out.json] [n_rows]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lists_merge_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
N_LISTS = 1024
BATCHES = (10_000, 1_000_000, 10_000_000)
WIDTHS = ((15, torch.uint8, 15), (4, torch.float32, None), (8, torch.int64, None))     # row bytes, dtype, columns


def rows_of(n, dtype, cols):
    shape = (n,) if cols is None else (n, cols)
    if dtype == torch.float32:
        return torch.rand(shape, dtype=dtype, device="cuda")
    return torch.randint(0, 255, shape, dtype=dtype, device="cuda")


def main():
    rng = np.random.default_rng(21)
    pq = ra.Pq(None, rng.standard_normal((2, 16, 4), dtype=np.float32))
    off_host, sizes = synthetic_lists(rng, N, N_LISTS)
    off_a = torch.from_numpy(off_host).cuda()
    ids_a = torch.repeat_interleave(torch.arange(N_LISTS, device="cuda"), torch.from_numpy(sizes).cuda())
    res = {"shape": {"n": N, "n_lists": N_LISTS, "size_min": int(sizes.min()), "size_median": int(np.median(sizes)),
                     "size_max": int(sizes.max())},
           "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0), "runs": []}
    for nb in BATCHES:
        # the batch: list ids drawn with the lists' own weights, laid out as add() lays a batch out
        ids_b = torch.sort(torch.from_numpy(rng.choice(N_LISTS, nb, p=sizes / sizes.sum())).cuda(), stable=True).values
        off_b = torch.zeros(N_LISTS + 1, dtype=torch.int64, device="cuda")
        off_b[1:] = torch.cumsum(torch.bincount(ids_b, minlength=N_LISTS), 0)
        ids = torch.cat([ids_a, ids_b])
        sort_ms, _ = timed(lambda: torch.sort(ids, stable=True))
        perm = torch.sort(ids, stable=True).indices
        del ids
        for row_bytes, dtype, cols in WIDTHS:
            a, b = rows_of(N, dtype, cols), rows_of(nb, dtype, cols)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            want = torch.cat([a, b])[perm]
            torch.cuda.synchronize()
            torch_peak = torch.cuda.max_memory_allocated() - base
            out = torch.empty_like(want)
            ra.launch_log(reset=True)
            got, off = pq.merge_lists_device(off_a, a, off_b, b, out=out, check=True)
            log = ra.launch_log(reset=True)
            same = bool(torch.equal(got.view(torch.uint8), want.view(torch.uint8))) and bool(torch.equal(off, off_a + off_b))
            merge_ms, merge_all = timed(lambda: pq.merge_lists_device(off_a, a, off_b, b, out=out))
            copy_ms, copy_all = timed(lambda: out.copy_(want))
            del got
            gather_ms, gather_all = timed(lambda: torch.cat([a, b])[perm])
            nbytes = out.numel() * out.element_size()
            row = {"row_bytes": row_bytes, "batch_rows": nb, "out_bytes": nbytes, "same_as_torch": same,
                   "merge_ms": round(merge_ms, 4), "copy_ms": round(copy_ms, 4), "torch_gather_ms": round(gather_ms, 4),
                   "torch_sort_ms": round(sort_ms, 4), "merge_over_copy": round(merge_ms / copy_ms, 3),
                   "merge_over_torch_gather": round(merge_ms / gather_ms, 3),
                   "merge_over_torch_sort_gather": round(merge_ms / (gather_ms + sort_ms), 3),
                   "merge_gb_s_read_plus_written": round(2 * nbytes / merge_ms / 1e6, 1),
                   "torch_peak_extra_bytes": int(torch_peak), "merge_extra_bytes": int(nbytes + 32 * N_LISTS + 16),
                   "launches": log, "all_ms": {"merge": merge_all, "copy": copy_all, "torch_gather": gather_all}}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
            if row_bytes == 15 and nb == 1_000_000:
                sweep = []
                try:
                    for g in (0, 256, 512, 1024, 2048, 4096, 8192):
                        ra.set_option("lists_merge_wgs", g)
                        ms, all_ms = timed(lambda: pq.merge_lists_device(off_a, a, off_b, b, out=out))
                        sweep.append({"wgs": g or "auto", "merge_ms": round(ms, 4), "all_ms": all_ms})
                        print(json.dumps(sweep[-1]), flush=True)
                finally:
                    ra.set_option("lists_merge_wgs", 0)
                res["wgs_sweep"] = {"row_bytes": 15, "batch_rows": nb, "runs": sweep}
            del a, b, want, out
            torch.cuda.empty_cache()
        del perm
    res["slower_than_torch_gather"] = [[r["row_bytes"], r["batch_rows"]] for r in res["runs"] if r["merge_over_torch_gather"] > 1]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print("| row bytes | batch rows | merge ms | copy ms | merge / copy | torch gather ms | torch sort ms | merge / gather | torch peak extra MB |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in res["runs"]:
        print("| %d | %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %d |"
              % (r["row_bytes"], r["batch_rows"], r["merge_ms"], r["copy_ms"], r["merge_over_copy"], r["torch_gather_ms"],
                 r["torch_sort_ms"], r["merge_over_torch_gather"], r["torch_peak_extra_bytes"] >> 20))
    assert all(r["same_as_torch"] for r in res["runs"]), "the merge differs from torch.cat([a, b])[perm]"


if __name__ == "__main__":
    main()
