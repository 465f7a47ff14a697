"""Exact search over resident vectors (Pq.flat_search_device, pqhip_flat_search_f32_dev) against what a user writes in
torch otherwise, in one process on the same buffers, on one MI355X; and the first recall numbers of the quantized
searches, measured against the flat truth.

Timing.  Standard-normal rows; per cell of N in {1 M, 10 M} x (d = 300 f32, d = 300 f16, d = 768 f16) x nq in {1, 8, 64} x
k in {10, 100, 1024}, squared L2: HIP events around the call, median of 5 after 2 warm-up calls, for
    kernel   flat_search_device: k_flat_search (+ merge) per pass of 4 queries (k <= 128) or 1
    torch    xn - 2 (q @ x.T) with the row norms xn precomputed outside the timing, then topk -- not bit-equal, no gate
both in the same run, plus rows x queries per second and the vector bytes N d vec_bytes (read once per PASS by the
kernel, but counted once: what one stream of the matrix costs) over the time as a fraction of 8 TB/s.  One masked row per
N: d = 300 f32, k = 10, 10 % of the rows allowed.  The share of the kernel's ids that torch's top-k also holds is
recorded per cell (rounding differs; not asserted).

Recall.  A trained index, d = 300, M = 15, K = 256 over 200,000 rows of a mixture of 2,000 Gaussians (sigma 0.3 around
unit-normal centres), 256 queries drawn the same way: recall@10 and recall@100 against exact_nearest of
QuantizedMatrix.nearest and PartitionedMatrix.nearest (1,024 lists) at nprobe 8 and 64, each plain and with refine=100.

Writes JSON (default profiles/flat_search_time.json).

usage: python tools/flat_search_time.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import reductive_amd as ra  # noqa: E402
from reductive_amd import qmatrix  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flat_search_time.json")
NS = (1_000_000, 10_000_000)
FORMS = ((300, torch.float32, "f32"), (300, torch.float16, "f16"), (768, torch.float16, "f16"))
NQS, KS = (1, 8, 64), (10, 100, 1024)
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


def composition(q, x, xn, k, flags=None):
    """what a caller without the kernel writes: |x|^2 - 2 q.x (the query's own norm does not change the order)"""
    d2 = xn[None, :] - 2.0 * (q.to(x.dtype) @ x.T).float()
    if flags is not None:
        d2 = d2.masked_fill(~flags[None, :], float("inf"))
    top = torch.topk(d2, k, dim=1, largest=False, sorted=True)
    return top.values, top.indices


def cell(res, pq, x, xn, q, k, name, words=None, flags=None):
    n, d = x.shape
    nq = q.shape[0]
    ra.launch_log(reset=True)
    v, i = pq.flat_search_device(q, x, k, allow=words, check=True)
    log = ra.launch_log(reset=True)
    tv, ti = composition(q, x, xn, k, flags)
    agree = float(np.mean([len(set(i[j].tolist()) & set(ti[j].tolist())) / k for j in sorted({0, nq - 1})]))
    ms_k, all_k = timed(lambda: pq.flat_search_device(q, x, k, allow=words))
    ms_t, all_t = timed(lambda: composition(q, x, xn, k, flags))
    vec_bytes = n * d * x.element_size()
    row = {"rows": n, "d": d, "vectors": name, "nq": nq, "k": k, "allowed_fraction": None if flags is None else 0.1,
           "ms": {"kernel": round(ms_k, 4), "torch": round(ms_t, 4)}, "kernel_over_torch": round(ms_k / ms_t, 4),
           "rows_x_queries_per_s": round(n * nq / (ms_k * 1e-3), 1), "vector_bytes": vec_bytes,
           "fraction_of_8TBps": round(vec_bytes / (ms_k * 1e-3) / HBM_BYTES_PER_S, 5),
           "ids_shared_with_torch": round(agree, 4), "launches": log, "all_ms": {"kernel": all_k, "torch": all_t}}
    print(json.dumps(row), flush=True)
    res["runs"].append(row)


def timing(res):
    pq = ra.Pq(None, np.zeros((1, 1, 300), np.float32))
    rng = np.random.default_rng(31)
    for n in NS:
        for d, dtype, name in FORMS:
            x = torch.empty((n, d), dtype=dtype, device="cuda")
            for r0 in range(0, n, 2_000_000):
                x[r0:r0 + 2_000_000].normal_()
            xn = torch.cat([(x[r0:r0 + 1_000_000].float() ** 2).sum(1) for r0 in range(0, n, 1_000_000)])
            ys = torch.from_numpy(rng.standard_normal((max(NQS), d), dtype=np.float32)).cuda()
            for nq in NQS:
                for k in KS:
                    cell(res, pq, x, xn, ys[:nq].contiguous(), k, name)
            if d == 300 and dtype == torch.float32:
                flags = torch.rand(n, device="cuda") < 0.1
                words = pq.pack_row_mask_device(flags)
                for nq in (1, 8):
                    cell(res, pq, x, xn, ys[:nq].contiguous(), 10, name, words=words, flags=flags)
            del x, xn
            torch.cuda.empty_cache()


def recall_numbers(res):
    n, d, m, bits, n_lists, nq, centres = 200_000, 300, 15, 8, 1024, 256, 2000
    rng = np.random.default_rng(32)
    c = rng.standard_normal((centres, d), dtype=np.float32)
    x = c[rng.integers(0, centres, n)] + np.float32(0.3) * rng.standard_normal((n, d), dtype=np.float32)
    ys = c[rng.integers(0, centres, nq)] + np.float32(0.3) * rng.standard_normal((nq, d), dtype=np.float32)
    pq = ra.train_pq(m, bits, 8, 1, x[:50_000], rng=np.random.default_rng(33))
    xd = torch.from_numpy(x).cuda()
    qm = qmatrix.QuantizedMatrix(pq, pq.quantize_batch_device(xd).cpu().numpy()).attach_vectors(xd)
    pm = qm.partition(n_lists, n_iterations=5, vectors=xd, train_rows=50_000, rng=np.random.default_rng(34),
                      on_device=True).attach_vectors(xd)
    yd = torch.from_numpy(ys).cuda()
    truth = qm.exact_nearest(yd, 100)[1].cpu().numpy()

    def recall(found, k):
        f = found.cpu().numpy()
        return round(float(np.mean([len(set(f[j, :k].tolist()) & set(truth[j, :k].tolist())) / k for j in range(nq)])), 4)
    runs = []
    for name, fn, kw in (("QuantizedMatrix", qm.nearest, {}), ("PartitionedMatrix nprobe=8", pm.nearest, {"nprobe": 8}),
                         ("PartitionedMatrix nprobe=64", pm.nearest, {"nprobe": 64})):
        runs.append({"search": name,
                     "recall_at_10": recall(fn(yd, 10, **kw)[1], 10),
                     "recall_at_10_refine_100": recall(fn(yd, 10, refine=100, **kw)[1], 10),
                     "recall_at_100": recall(fn(yd, 100, **kw)[1], 100),
                     "recall_at_100_refine_100": recall(fn(yd, 100, refine=100, **kw)[1], 100)})
        print(json.dumps(runs[-1]), flush=True)
    res["recall"] = {"n": n, "d": d, "M": m, "K": 1 << bits, "n_lists": n_lists, "queries": nq,
                     "data": "mixture of %d Gaussians, sigma 0.3" % centres,
                     "truth": "exact_nearest (pqhip_flat_search_f32_dev) over the attached f32 vectors", "runs": runs}


def main():
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS,
           "torch_baseline": "xn - 2 (q @ x.T) in the vectors' dtype, row norms precomputed, then topk; not bit-equal",
           "runs": []}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    for stage in (timing, recall_numbers):
        stage(res)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
