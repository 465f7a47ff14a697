"""Exact search among given rows (pqhip_flat_among_f32_dev, pqhip_flat_range_among_f32_dev) against what the library
offered for the same answer before, in one process on the same buffers, on one MI355X.

10 M standard-normal rows of d = 300, f32 and f16; nq in {1, 8, 64} queries, each with its own m in {1,000, 100,000,
1,000,000} random distinct ids (a CSR: lims + ids).  HIP events around the call, median of 5 after 2 warm-up calls.  Every
cell is compared bit for bit with its baseline before it is timed.
    top-k   k in {10, 100}: flat_among_device against
            masked   flat_search_device with the mask of the query's candidates, one call per query, the masks packed
                     outside the timing -- it walks the mask words of all 10 M rows and loads the allowed ones
            rerank   (m = 1,000 only) rerank_device on the same candidates as a [nq, 1000] matrix
    range   flat_range_among_device's two raw calls (count, then fill at the result's size) at a selective threshold (the
            query's 10th best candidate) and at +Inf (every candidate), against
            masked   flat_range_device with the same mask and radius, one call per query (capacity given, so one call)
            The ids are sorted ascending per query for the range cells, so that both return the same sequence.
The top-k cells name each query's ids in random order.  Reported per cell: the medians, all five times, the spread
(max - min), ours / baseline, the workgroups per query the host rule gives (recomputed here by the rule's formula), and the
NAMED bytes (nq m d element bytes) over time as a fraction of 8 TB/s.  A cell slower than a baseline by more than the
larger spread is listed under "findings".  A last sweep (one query, k = 10, m up to all rows) brackets the fraction of
the rows at which the masked exhaustive call becomes as fast as the gather.

Writes JSON (default profiles/flat_among_time.json).

usage: python tools/flat_among_time.py [out.json]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_among_time.json")
N, D = 10_000_000, 300
FORMS = ((torch.float32, "f32"), (torch.float16, "f16"))
NQS, MS, KS = (1, 8, 64), (1_000, 100_000, 1_000_000), (10, 100)
SWEEP = (2_000_000, 5_000_000, 10_000_000)
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


def spread(*alls):
    return max(max(a) - min(a) for a in alls)


def same(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def raw_range(pq, q, x, lims, ids, thr, out_lims, val, idx, capacity):
    """pqhip_flat_range_among_f32_dev on contiguous tensors, squared L2; capacity 0: null outputs"""
    nq = q.shape[0]
    rc = _lib.lib().pqhip_flat_range_among_f32_dev(
        pq._cb(), pq._slot_for(x), q.data_ptr(), nq, D, x.data_ptr(), x.element_size(), N, D, D, lims.data_ptr(), ids.data_ptr(),
        ids.shape[0], 0, thr.data_ptr(), out_lims.data_ptr(), val.data_ptr() if capacity else None,
        idx.data_ptr() if capacity else None, capacity, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK, rc


def rule_wgs(mean_ids, nq, row_bytes, n_cus):
    """flat_among_wgs_per_query of pqhip_flat_among.hip"""
    by_bytes = int((mean_ids * row_bytes + 262143.0) / 262144.0)
    by_tiles = (mean_ids + 255) // 256
    return max(1, min(by_bytes, by_tiles, max(1, n_cus // max(nq, 1))))


def candidates(nq, m, gen):
    """nq sorted lists of m distinct rows -> (lims, ids) on the device"""
    if m == N:
        parts = [torch.arange(N, dtype=torch.int64, device="cuda") for _ in range(nq)]
    else:
        parts = [torch.sort(torch.randperm(N, device="cuda", generator=gen)[:m]).values for _ in range(nq)]
    lims = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * m
    return lims, torch.cat(parts)


def masks_of(pq, lims, ids, nq):
    words = []
    for j in range(nq):
        flags = torch.zeros(N, dtype=torch.bool, device="cuda")
        flags[ids[int(lims[j]):int(lims[j + 1])]] = True
        words.append(pq.pack_row_mask_device(flags.view(torch.uint8)))
    return words


def main():
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "d": D, "warmup": WARM, "reps": REPS,
           "baseline_masked": "flat_search_device / flat_range_device with the mask of the query's candidates, one call per query, "
                              "masks packed outside the timing",
           "baseline_rerank": "rerank_device on the same candidates (m = 1,000)",
           "topk": [], "range": [], "sweep": [], "findings": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    pq = ra.Pq(None, np.zeros((1, 1, D), np.float32))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(47)
    rng = np.random.default_rng(47)
    ys = torch.from_numpy(rng.standard_normal((max(NQS), D), dtype=np.float32)).cuda()

    def save():
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)

    def finding(kind, row, ours, base, sp):
        if ours > base + sp:
            res["findings"].append({"cell": kind, **{key: row[key] for key in row if key not in ("all_ms", "launches")}})

    for dtype, name in FORMS:
        x = torch.empty((N, D), dtype=dtype, device="cuda")
        for r0 in range(0, N, 2_000_000):
            x[r0:r0 + 2_000_000].normal_()
        row_bytes = D * x.element_size()
        for nq in NQS:
            q = ys[:nq].contiguous()
            for m in MS:
                lims, ids = candidates(nq, m, gen)
                shuffled = torch.cat([ids[j * m:(j + 1) * m][torch.randperm(m, device="cuda", generator=gen)] for j in range(nq)])
                words = masks_of(pq, lims, ids, nq)
                named = nq * m * row_bytes
                G = rule_wgs(m, nq, row_bytes, n_cus)
                for k in KS:
                    ra.launch_log(reset=True)
                    v, i = pq.flat_among_device(q, x, shuffled, k, lims=lims, check=True)
                    log = ra.launch_log(reset=True)
                    for j in range(nq):
                        mv, mi = pq.flat_search_device(q[j], x, k, allow=words[j])
                        assert same(mv, v[j]) and same(mi, i[j]), (name, nq, m, k, j)
                    ms_a, all_a = timed(lambda: pq.flat_among_device(q, x, shuffled, k, lims=lims))
                    ms_m, all_m = timed(lambda: [pq.flat_search_device(q[j], x, k, allow=words[j]) for j in range(nq)])
                    row = {"vectors": name, "nq": nq, "ids_per_query": m, "k": k, "wgs_per_query": G,
                           "ms": {"among": round(ms_a, 4), "masked": round(ms_m, 4)}, "among_over_masked": round(ms_a / ms_m, 4),
                           "named_fraction_of_8TBps": round(named / (ms_a * 1e-3) / HBM_BYTES_PER_S, 5),
                           "spread_ms": round(spread(all_a, all_m), 4), "launches": log, "all_ms": {"among": all_a, "masked": all_m}}
                    finding("topk vs masked", row, ms_a, ms_m, row["spread_ms"])
                    if m <= 1024:
                        cand = shuffled.view(nq, m)
                        cv, ci = pq.rerank_device(q, x, cand, k)
                        assert same(cv, v) and same(ci, i), (name, nq, m, k)
                        ms_r, all_r = timed(lambda: pq.rerank_device(q, x, cand, k))
                        row["ms"]["rerank"] = round(ms_r, 4)
                        row["among_over_rerank"] = round(ms_a / ms_r, 4)
                        row["all_ms"]["rerank"] = all_r
                        row["spread_rerank_ms"] = round(spread(all_a, all_r), 4)
                        finding("topk vs rerank", row, ms_a, ms_r, row["spread_rerank_ms"])
                    print(json.dumps(row), flush=True)
                    res["topk"].append(row)
                    save()
                # range: the ascending ids, a selective threshold (the 10th best candidate) and +Inf
                best, _ = pq.flat_among_device(q, x, ids, 10, lims=lims)
                out_lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
                for kind, thr in (("10", best[:, 9].contiguous()), ("all", torch.full((nq,), float("inf"), device="cuda"))):
                    tl = thr.tolist()                        # host copies: no read of the device inside the timing
                    ra.launch_log(reset=True)
                    l, v, i = pq.flat_range_among_device(q, x, ids, thr, lims=lims, check=True)
                    log = ra.launch_log(reset=True)
                    total = int(l[-1])
                    for j in range(nq):
                        ml, mv, mi = pq.flat_range_device(q[j], x, tl[j], allow=words[j], capacity=total + 1)
                        seg = slice(int(l[j]), int(l[j + 1]))
                        assert same(i[seg], mi) and same(v[seg], mv), (name, nq, m, kind, j)
                    val = torch.empty(max(total, 1), dtype=torch.float32, device="cuda")
                    idx = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")

                    def both():
                        raw_range(pq, q, x, lims, ids, thr, out_lims, None, None, 0)
                        raw_range(pq, q, x, lims, ids, thr, out_lims, val, idx, max(total, 1))
                    ms_c, all_c = timed(lambda: raw_range(pq, q, x, lims, ids, thr, out_lims, None, None, 0))
                    ms_f, all_f = timed(lambda: raw_range(pq, q, x, lims, ids, thr, out_lims, val, idx, max(total, 1)))
                    ms_b, all_b = timed(both)
                    ms_m, all_m = timed(lambda: [pq.flat_range_device(q[j], x, tl[j], allow=words[j], capacity=total + 1)
                                                 for j in range(nq)])
                    row = {"vectors": name, "nq": nq, "ids_per_query": m, "radius": kind, "rows_returned": total, "wgs_per_query": G,
                           "ms": {"count": round(ms_c, 4), "full": round(ms_f, 4), "count_then_full": round(ms_b, 4),
                                  "masked": round(ms_m, 4)},
                           "full_over_masked": round(ms_f / ms_m, 4),
                           "named_fraction_of_8TBps_count": round(named / (ms_c * 1e-3) / HBM_BYTES_PER_S, 5),
                           "spread_ms": round(spread(all_f, all_m), 4), "launches": log,
                           "all_ms": {"count": all_c, "full": all_f, "count_then_full": all_b, "masked": all_m}}
                    finding("range vs masked", row, ms_f, ms_m, row["spread_ms"])
                    print(json.dumps(row), flush=True)
                    res["range"].append(row)
                    save()
                    del val, idx, l, v, i
                del lims, ids, shuffled, words
                torch.cuda.empty_cache()
        # where the gather loses to the stream: one query, k = 10, ever larger fractions of the rows
        q = ys[:1].contiguous()
        for m in SWEEP:
            lims, ids = candidates(1, m, gen)
            words = masks_of(pq, lims, ids, 1)
            v, i = pq.flat_among_device(q, x, ids, 10, lims=lims, check=True)
            mv, mi = pq.flat_search_device(q[0], x, 10, allow=words[0])
            assert same(mv, v[0]) and same(mi, i[0]), (name, m)
            ms_a, all_a = timed(lambda: pq.flat_among_device(q, x, ids, 10, lims=lims))
            ms_m, all_m = timed(lambda: pq.flat_search_device(q[0], x, 10, allow=words[0]))
            ms_u, all_u = timed(lambda: pq.flat_search_device(q[0], x, 10))
            row = {"vectors": name, "nq": 1, "ids_per_query": m, "fraction_of_rows": m / N, "k": 10,
                   "ms": {"among": round(ms_a, 4), "masked": round(ms_m, 4), "unmasked": round(ms_u, 4)},
                   "among_over_masked": round(ms_a / ms_m, 4),
                   "named_fraction_of_8TBps": round(m * row_bytes / (ms_a * 1e-3) / HBM_BYTES_PER_S, 5),
                   "all_ms": {"among": all_a, "masked": all_m, "unmasked": all_u}}
            print(json.dumps(row), flush=True)
            res["sweep"].append(row)
            save()
            del lims, ids, words
        del x
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
