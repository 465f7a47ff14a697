"""Exact range search over resident vectors (pqhip_flat_range_f32_dev, pqhip_flat_range_lists_f32_dev) against what
bounds it, in one process on the same buffers, on one MI355X.

10 M standard-normal rows of d = 300, f32 and f16.  Per cell of nq in {1, 8, 64} x radius in {none, ~10, ~1,000, all},
squared L2: the radii are the query's own 10th / 1,000th smallest distance (from flat_search_device, k = 1,024), half its
smallest distance (no row) and +Inf (every row).  HIP events around the call, median of 5 after 2 warm-up calls, outputs
allocated before the timing, for
    count      the raw call with capacity = 0: the count pass (one stream of the matrix per pass of 4 queries) + scans
    full       the raw call with capacity = the result's size: count + scan + fill from the hit bitmap
    search     baseline (i): flat_search_device at k = 10 -- one stream of the matrix per pass of 4 queries.  A selective
               full call should cost about this, the admit-everything call about twice this.
    torch      baseline (ii): norms - 2 q @ x.T (+ the query norms), compare, nonzero; the row norms are computed before
               the timing.  ANOTHER ROUNDING: its distances are not the library's, so rows at the radius may differ; it is
               timed, not compared.  Skipped where its intermediates would not fit beside the outputs (nq = 64, all).
Reported per cell: the medians, all five times of each, the spread (max - min) of full and search, full / search, and the
matrix bytes over the count time as a fraction of 8 TB/s.  A selective cell (none, ~10, ~1,000) whose full call is slower
than the search by more than the larger of the two spreads is listed under "findings", as is an admit-everything cell
slower than twice the search by more than that.

List form: the same rows in 1,024 lists of random lengths, nprobe in {8, 64}, nq in {1, 8, 64}, radius ~10 (of the probed
rows' own distances this is wider than the query's 10th over all rows: the threshold is the exhaustive one, the lists
return a subset) and all.  `lists` = flat_range_lists_device against `masked` = flat_range_device with the mask of the
query's probed lists, one call per query, masks packed before the timing; the results are compared as sets per query.

Writes JSON (default profiles/flat_range_time.json).

usage: python tools/flat_range_time.py [out.json]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402
from reductive_amd import _lib  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_range_time.json")
N, D, LISTS = 10_000_000, 300, 1024
FORMS = ((torch.float32, "f32"), (torch.float16, "f16"))
NQS, NPROBES = (1, 8, 64), (8, 64)
RADII = ("none", "10", "1000", "all")
WARM, REPS = 2, 5
HBM_BYTES_PER_S = 8e12


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


def raw_range(pq, q, x, thr, lims, val, idx, capacity):
    """pqhip_flat_range_f32_dev on contiguous tensors, squared L2, no mask; capacity 0: null outputs"""
    nq = q.shape[0]
    rc = _lib.lib().pqhip_flat_range_f32_dev(
        pq._cb(), pq._slot_for(x), q.data_ptr(), nq, D, x.data_ptr(), x.element_size(), N, D, D, None, 0, thr.data_ptr(),
        lims.data_ptr(), val.data_ptr() if capacity else None, idx.data_ptr() if capacity else None, capacity,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK, rc


def thresholds(pq, q, x):
    """per radius class one threshold per query, from the query's own nearest distances"""
    v, _ = pq.flat_search_device(q, x, 1024)
    inf = torch.full_like(v[:, 0], float("inf"))
    return {"none": (v[:, 0] * 0.5).contiguous(), "10": v[:, 9].contiguous(), "1000": v[:, 999].contiguous(), "all": inf}


def masks_of(pq, off, probes):
    words = []
    for row in probes.tolist():
        flags = torch.zeros(N, dtype=torch.bool, device="cuda")
        for l in row:
            flags[off[l]:off[l + 1]] = True
        words.append(pq.pack_row_mask_device(flags.view(torch.uint8)))
    return words


def main():
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "d": D, "n_lists": LISTS, "warmup": WARM, "reps": REPS,
           "baseline_search": "flat_search_device, k = 10: one stream of the matrix per pass of 4 queries",
           "baseline_torch": "row norms (precomputed) - 2 q @ x.T + query norms, <= radius, nonzero: another rounding, timed only",
           "runs": [], "findings": [], "lists": [], "lists_findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    pq = ra.Pq(None, np.zeros((1, 1, D), np.float32))
    rng = np.random.default_rng(43)
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
        norms = torch.cat([(x[r0:r0 + 1_000_000].float() ** 2).sum(1) for r0 in range(0, N, 1_000_000)])
        for nq in NQS:
            q = ys[:nq].contiguous()
            qt = q.to(dtype)
            thr = thresholds(pq, q, x)
            ms_s, all_s = timed(lambda: pq.flat_search_device(q, x, 10))
            lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
            for radius in RADII:
                t = thr[radius]
                raw_range(pq, q, x, t, lims, None, None, 0)
                total = int(lims[-1])
                cap = max(total, 1)
                val = torch.empty(cap, dtype=torch.float32, device="cuda")
                idx = torch.empty(cap, dtype=torch.int64, device="cuda")
                ra.launch_log(reset=True)
                raw_range(pq, q, x, t, lims, val, idx, cap)
                log = ra.launch_log(reset=True)
                ms_c, all_c = timed(lambda: raw_range(pq, q, x, t, lims, None, None, 0))
                ms_f, all_f = timed(lambda: raw_range(pq, q, x, t, lims, val, idx, cap))
                ms_t, all_t = None, None
                if not (nq == 64 and radius == "all"):
                    qn = (q * q).sum(1)
                    ms_t, all_t = timed(lambda: torch.nonzero((norms[None] - 2.0 * (qt @ x.T).float() + qn[:, None]) <= t[:, None]))
                spread = max(max(all_f) - min(all_f), max(all_s) - min(all_s))
                row = {"vectors": name, "nq": nq, "radius": radius, "rows_returned": total,
                       "ms": {"count": round(ms_c, 4), "full": round(ms_f, 4), "search_k10": round(ms_s, 4),
                              "torch": None if ms_t is None else round(ms_t, 4)},
                       "full_over_search": round(ms_f / ms_s, 4), "spread_ms": round(spread, 4),
                       "count_fraction_of_8TBps": round(matrix_bytes * -(-nq // 4) / (ms_c * 1e-3) / HBM_BYTES_PER_S, 5),
                       "launches": log, "all_ms": {"count": all_c, "full": all_f, "search_k10": all_s, "torch": all_t}}
                print(json.dumps(row), flush=True)
                res["runs"].append(row)
                budget = 2.0 * ms_s if radius == "all" else ms_s
                if ms_f > budget + spread:
                    res["findings"].append({key: row[key] for key in ("vectors", "nq", "radius", "ms", "spread_ms", "full_over_search")})
                del val, idx
                with open(OUT, "w") as f:
                    json.dump(res, f, indent=1)
            for p in NPROBES:
                pr = probes[(nq, p)]
                pd = torch.from_numpy(pr).cuda()
                words = masks_of(pq, off, pr)
                for radius in ("10", "all"):
                    t = thr[radius]
                    tl = t.tolist()                          # host copies: no read of the device inside the timing
                    ra.launch_log(reset=True)
                    l, v, i = pq.flat_range_lists_device(q, x, od, pd, t, check=True)
                    log = ra.launch_log(reset=True)
                    total = int(l[-1])
                    for j in range(nq):
                        ml, mv, mi = pq.flat_range_device(q[j], x, tl[j], allow=words[j], capacity=total + 1)
                        seg = slice(int(l[j]), int(l[j + 1]))
                        order = torch.sort(i[seg]).indices
                        assert torch.equal(i[seg][order], mi) and torch.equal(v[seg][order].view(torch.int32), mv.view(torch.int32))
                    ms_l, all_l = timed(lambda: pq.flat_range_lists_device(q, x, od, pd, t, capacity=total + 1))
                    ms_m, all_m = timed(lambda: [pq.flat_range_device(q[j], x, tl[j], allow=words[j], capacity=total + 1)
                                                 for j in range(nq)])
                    spread = max(max(all_l) - min(all_l), max(all_m) - min(all_m))
                    row = {"vectors": name, "nq": nq, "nprobe": p, "radius": radius, "rows_returned": total,
                           "ms": {"lists": round(ms_l, 4), "masked": round(ms_m, 4)}, "lists_over_masked": round(ms_l / ms_m, 4),
                           "spread_ms": round(spread, 4), "launches": log, "all_ms": {"lists": all_l, "masked": all_m}}
                    print(json.dumps(row), flush=True)
                    res["lists"].append(row)
                    if ms_l > ms_m + spread:
                        res["lists_findings"].append({key: row[key] for key in ("vectors", "nq", "nprobe", "radius", "ms", "spread_ms")})
                    with open(OUT, "w") as f:
                        json.dump(res, f, indent=1)
        del x, norms
        torch.cuda.empty_cache()
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
