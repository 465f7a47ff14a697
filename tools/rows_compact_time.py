"""The row compaction (Pq.compact_rows_device; compact() of the partitioned matrices) against the route available without
it, in one process, HIP events, 2 warm-up calls, median of 7.

Arrays: what a matrix of 100 M rows stores per row -- 15-byte codes, f32 norms, int64 ids -- under four masks: 10 %, 50 %
and 90 % of the rows removed at random, and 10 % removed in runs of 4,096 consecutive rows.  Per cell
  compact   pq.compact_rows_device(words, a, capacity=count, out=out)     (count + scan + mover, and the read of the count)
  torch     a[keep], keep the bool flags on the device                    (nonzero + gather through 8-byte indices)
  copy      a device-to-device copy of the kept bytes: the box's copy rate beside the achieved one
The achieved rate counts mask + kept rows read + kept rows written.  Every cell's result is compared with torch's, bit
for bit, before it is timed.

Matrices: compact(flags) of a PartitionedMatrix and of a ResidualPartitionedMatrix of the same size over 1,024 lists, at
10 % and 50 % removed at random, against torch boolean-mask indexing of each original-order array followed by the class's
constructor (laid out on the device).  Writes JSON (default profiles/rows_compact_time.json) and prints the tables of
DESIGN.md.

usage: python tools/rows_compact_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from reductive_amd import qmatrix  # noqa: E402
from adc_search_time import timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rows_compact_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
N_LISTS, M, DSUB = 1024, 15, 4
ARRAYS = (("codes", 15, torch.uint8, 15), ("norms", 4, torch.float32, None), ("ids", 8, torch.int64, None))


def keep_flags(kind, removed):
    """bool [N] on the device: `removed` of the rows cleared, singly at random or in runs of 4,096 consecutive rows"""
    g = torch.Generator(device="cuda").manual_seed(int(removed * 100) + (7 if kind == "runs" else 0))
    if kind == "random":
        return torch.rand(N, device="cuda", generator=g) >= removed
    runs = torch.rand((N + 4095) // 4096, device="cuda", generator=g) >= removed
    return torch.repeat_interleave(runs, 4096)[:N].contiguous()


def rows_of(dtype, cols):
    shape = (N,) if cols is None else (N, cols)
    if dtype == torch.float32:
        return torch.rand(shape, dtype=dtype, device="cuda")
    return torch.randint(0, 255, shape, dtype=dtype, device="cuda")


def flat(pq, codes, norms):
    """a QuantizedMatrix around device tensors (its constructor takes host arrays)"""
    m = object.__new__(qmatrix.QuantizedMatrix)
    m.pq, m.codes, m.norms = pq, codes, norms
    return m


def same_matrix(a, b, names):
    return all(torch.equal(getattr(a, t).view(torch.uint8), getattr(b, t).view(torch.uint8)) for t in names)


def main():
    rng = np.random.default_rng(31)
    pq = ra.Pq(None, rng.standard_normal((M, 256, DSUB), dtype=np.float32))
    res = {"shape": {"n": N, "n_lists": N_LISTS}, "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0),
           "arrays": [], "matrices": []}
    for kind, removed in (("random", 0.1), ("random", 0.5), ("random", 0.9), ("runs", 0.1)):
        keep = keep_flags(kind, removed)
        words = pq.pack_row_mask_device(keep)
        for name, row_bytes, dtype, cols in ARRAYS:
            a = rows_of(dtype, cols)
            want = a[keep]
            c = want.shape[0]
            out = torch.empty_like(want)
            ra.launch_log(reset=True)
            got, _, _, count = pq.compact_rows_device(words, a, capacity=c, out=out, check=True)
            log = ra.launch_log(reset=True)
            same = count == c and bool(torch.equal(got.view(torch.uint8), want.view(torch.uint8)))
            compact_ms, compact_all = timed(lambda: pq.compact_rows_device(words, a, capacity=c, out=out))
            torch_ms, torch_all = timed(lambda: a[keep])
            copy_ms, copy_all = timed(lambda: out.copy_(want))
            kept_bytes = c * row_bytes
            moved = words.numel() * 4 + 2 * kept_bytes
            row = {"array": name, "row_bytes": row_bytes, "mask": kind, "removed": removed, "kept_rows": c, "same_as_torch": same,
                   "compact_ms": round(compact_ms, 4), "torch_ms": round(torch_ms, 4), "copy_ms": round(copy_ms, 4),
                   "compact_over_torch": round(compact_ms / torch_ms, 3),
                   "compact_gb_s": round(moved / compact_ms / 1e6, 1), "copy_gb_s": round(2 * kept_bytes / copy_ms / 1e6, 1),
                   "launches": log, "all_ms": {"compact": compact_all, "torch": torch_all, "copy": copy_all}}
            print(json.dumps(row), flush=True)
            res["arrays"].append(row)
            del a, want, out, got
            torch.cuda.empty_cache()
        del keep, words

    # the matrices: original-order arrays, a random assignment to 1,024 lists, the layout on the device
    rpq = ra.Pq(None, rng.standard_normal((M, 256, DSUB), dtype=np.float32) * np.float32(0.7))
    centroids = rng.standard_normal((N_LISTS, M * DSUB), dtype=np.float32)
    codes, norms, terms = rows_of(torch.uint8, M), rows_of(torch.float32, None), rows_of(torch.float32, None)
    assign = torch.randint(0, N_LISTS, (N,), dtype=torch.int64, device="cuda")
    builders = {
        "PartitionedMatrix": (lambda sel: qmatrix.PartitionedMatrix(flat(pq, codes[sel], norms[sel]), centroids, assign[sel]),
                              ("ids", "list_off", "positions", "codes", "norms")),
        "ResidualPartitionedMatrix": (lambda sel: qmatrix.ResidualPartitionedMatrix(rpq, codes[sel], norms[sel], terms[sel], centroids,
                                                                                   assign[sel]),
                                      ("ids", "list_off", "positions", "codes", "norms", "row_terms", "lists"))}
    for cls, (build, names) in builders.items():
        m = build(slice(None))
        for removed in (0.1, 0.5):
            keep = keep_flags("random", removed)
            want = build(keep)
            got, kept = m.compact(keep)
            same = same_matrix(got, want, names) and bool(torch.equal(kept, torch.nonzero(keep)[:, 0]))
            del got, want, kept
            torch.cuda.empty_cache()
            compact_ms, compact_all = timed(lambda: m.compact(keep))
            torch_ms, torch_all = timed(lambda: build(keep))
            row = {"class": cls, "removed": removed, "same_as_constructor": same, "compact_ms": round(compact_ms, 3),
                   "torch_index_and_constructor_ms": round(torch_ms, 3), "compact_over_torch": round(compact_ms / torch_ms, 3),
                   "all_ms": {"compact": compact_all, "torch": torch_all}}
            print(json.dumps(row), flush=True)
            res["matrices"].append(row)
            del keep
        del m
        torch.cuda.empty_cache()
    res["slower_than_torch"] = [[r["array"], r["mask"], r["removed"]] for r in res["arrays"] if r["compact_over_torch"] > 1] + \
                               [[r["class"], r["removed"]] for r in res["matrices"] if r["compact_over_torch"] > 1]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print("| array | mask | removed | compact ms | torch ms | compact / torch | compact GB/s | copy GB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in res["arrays"]:
        print("| %s (%d B) | %s | %d %% | %.3f | %.3f | %.2f | %.0f | %.0f |"
              % (r["array"], r["row_bytes"], r["mask"], round(100 * r["removed"]), r["compact_ms"], r["torch_ms"],
                 r["compact_over_torch"], r["compact_gb_s"], r["copy_gb_s"]))
    print("| class | removed | compact() ms | torch index + constructor ms | ratio |")
    print("|---|---|---|---|---|")
    for r in res["matrices"]:
        print("| %s | %d %% | %.2f | %.2f | %.2f |" % (r["class"], round(100 * r["removed"]), r["compact_ms"],
                                                    r["torch_index_and_constructor_ms"], r["compact_over_torch"]))
    assert all(r["same_as_torch"] for r in res["arrays"]), "the compaction differs from a[keep]"
    assert all(r["same_as_constructor"] for r in res["matrices"]), "compact() differs from the constructor on the kept rows"


if __name__ == "__main__":
    main()
