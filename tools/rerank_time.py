"""Exact re-ranking (Pq.rerank_device, pqhip_rerank_f32_dev) against the torch composition of the same stage, in one
process on the same data: a resident matrix of d = 300 columns with as many rows as asked for (default 100 M: 60 GB as
f16, 120 GB as f32; halved until it fits, the size used is recorded), standard-normal entries, candidates random
DISTINCT rows per query -- the unfavourable case for the gather, no two candidates share a cache line.  Per cell of
nq in {1, 8, 256} x R in {10, 100, 1024} x k in {10, min(100, R)} x {f32, f16} x {L2, IP}: HIP events around the call,
median of 7 after 2 warm-up calls, for
    kernel      rerank_device: k_rerank_dist + k_rerank_select
    torch       vectors[cand] -> (difference -> square | product) -> sum -> topk -> gather of the row ids
and the bytes the kernel must read, nq R d vec_bytes, over its time as a fraction of 8 TB/s (HBM peak; a share of peak
of the whole call, selection included).  Every cell is checked on the device for its first and last query against a
float64 torch evaluation: returned values within the f32 bound of tests/rerank_ref.py of the float64 values of the
returned rows, ascending order, and no candidate left out that is better than the k-th by more than that bound.

One end-to-end pair per vector type: ResidualPartitionedMatrix.nearest at nprobe = 8, k = 10 over the same number of
rows (M = 15, K = 256, 1,024 synthetic lists, random codes and terms: timing needs no trained quantizer), 1 and 8
queries, with and without refine=100.

Expectation recorded per cell (not asserted): the kernel reads every gathered element once in at most two launches,
the composition moves the gathered block at least three times over five or more launches, so kernel <= torch in every
cell.  The trained fixture of tests/test_gpu_refine.py gives recall@10 with and without refine=100 per nprobe.
Writes JSON (default profiles/rerank_time.json).

usage: python tools/rerank_time.py [out.json] [n_rows]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reductive_amd as ra  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rerank_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
D = 300
NQS, RS = (1, 8, 256), (10, 100, 1024)
WARM, REPS = 2, 7
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


def composition(q, x, cand, k, ip):
    """what a caller without the kernel writes"""
    g = x[cand].float()                                    # [nq, R, d]
    if ip:
        v = (g * q[:, None, :]).sum(2)
    else:
        t = g - q[:, None, :]
        v = (t * t).sum(2)
    top = torch.topk(v, k, dim=1, largest=ip, sorted=True)
    return top.values, torch.gather(cand, 1, top.indices)


def f32_bound(d, ip):
    """tests/rerank_ref.py f32_bound: (3 | 1) + ceil(d / 64) + 6 roundings of 2^-24"""
    u = 2.0 ** -24
    r = (1 if ip else 3) + -(-d // 64) + 6
    return r * u / (1.0 - r * u)


def exact(q, x, cand, got_v, got_i, k, ip):
    """one query against float64 on the device"""
    g = x[cand].double()
    term = g * q.double() if ip else (g - q.double()) ** 2
    v64, scale = term.sum(1), term.abs().sum(1)
    bound = f32_bound(x.shape[1], ip) * scale
    hit = cand[None, :] == got_i[:, None]                  # [k, R]: where each returned row sits among the candidates
    pos = hit.int().argmax(1)
    ok = bool(hit.any(1).all()) and got_i.unique().numel() == k
    ok = ok and bool(((got_v.double() - v64[pos]).abs() <= bound[pos]).all())
    key = -got_v if ip else got_v
    ok = ok and bool((key[1:] >= key[:-1]).all())
    kth = torch.topk(-v64 if ip else v64, k, largest=False).values[-1]
    worst = (-v64[pos] if ip else v64[pos]).max()
    return ok and bool(worst <= kth + 2.0 * bound.max())


def allocate(rows, dtype):
    """standard-normal [rows, D], filled in place; halves the rows until the allocation succeeds"""
    while True:
        try:
            x = torch.empty((rows, D), dtype=dtype, device="cuda")
            break
        except torch.OutOfMemoryError:
            rows //= 2
    step = 4_000_000
    for r0 in range(0, rows, step):
        x[r0:r0 + step].normal_()
    return x


def distinct_rows(n, count):
    """`count` distinct random rows of n, in random order, on the device"""
    if n < 8 * count:
        return torch.randperm(n, device="cuda")[:count]
    while True:
        u = torch.unique(torch.randint(0, n, (2 * count + 16,), device="cuda"))
        if u.numel() >= count:
            return u[torch.randperm(u.numel(), device="cuda")[:count]]


def cells(res, pq, x, name):
    rng = np.random.default_rng(21)
    n = x.shape[0]
    ys = torch.from_numpy(rng.standard_normal((max(NQS), D), dtype=np.float32)).cuda()
    for nq in NQS:
        q = ys[:nq].contiguous()
        for R in RS:
            cand = torch.stack([distinct_rows(n, R) for _ in range(nq)])
            for k in sorted({10, min(100, R)}):
                for ip in (False, True):
                    ra.launch_log(reset=True)
                    v, i = pq.rerank_device(q, x, cand, k, ip=ip, check=True)
                    log = ra.launch_log(reset=True)
                    ok = all(exact(q[j], x, cand[j], v[j], i[j], k, ip) for j in sorted({0, nq - 1}))
                    ms_k, all_k = timed(lambda: pq.rerank_device(q, x, cand, k, ip=ip))
                    ms_t, all_t = timed(lambda: composition(q, x, cand, k, ip))
                    must_read = nq * R * D * x.element_size()
                    row = {"vectors": name, "metric": "ip" if ip else "l2", "nq": nq, "R": R, "k": k,
                           "ms": {"kernel": round(ms_k, 4), "torch": round(ms_t, 4)},
                           "kernel_over_torch": round(ms_k / ms_t, 4), "kernel_within_expectation": bool(ms_k <= ms_t),
                           "bytes_must_read": must_read,
                           "fraction_of_8TBps": round(must_read / (ms_k * 1e-3) / HBM_BYTES_PER_S, 5),
                           "exact": ok, "launches": log, "all_ms": {"kernel": all_k, "torch": all_t}}
                    print(json.dumps(row), flush=True)
                    res["runs"].append(row)


def synthetic_matrix(n):
    """a ResidualPartitionedMatrix of n rows for timing: 1,024 lists of log-normal sizes, rows assigned at random"""
    from reductive_amd import qmatrix
    m, kk, dsub, n_lists = 15, 256, 20, 1024
    rng = np.random.default_rng(22)
    pq = ra.Pq(None, rng.standard_normal((m, kk, dsub), dtype=np.float32))
    sizes = rng.lognormal(0.0, 0.5, n_lists)
    assign = np.repeat(np.arange(n_lists), np.floor(sizes / sizes.sum() * n).astype(np.int64))
    assign = np.concatenate([assign, np.zeros(n - assign.size, np.int64)])
    rng.shuffle(assign)
    codes = torch.randint(0, kk, (n, m), dtype=torch.uint8, device="cuda")
    terms = torch.from_numpy(rng.uniform(0.0, 40.0, n).astype(np.float32)).cuda()
    return qmatrix.ResidualPartitionedMatrix(pq, codes, None, terms, rng.standard_normal((n_lists, D), dtype=np.float32), assign)


def end_to_end(res, rm, x, name):
    """ResidualPartitionedMatrix.nearest with and without refine=100 over as many rows as x has"""
    n, nprobe, k, R = x.shape[0], 8, 10, 100
    rng = np.random.default_rng(23)
    rm.vectors = x
    for nq in (1, 8):
        q = torch.from_numpy(rng.standard_normal((nq, D), dtype=np.float32)).cuda()
        ms_p, all_p = timed(lambda: rm.nearest(q, k, nprobe))
        ms_c, all_c = timed(lambda: rm.nearest(q, R, nprobe))
        ms_r, all_r = timed(lambda: rm.nearest(q, k, nprobe, refine=R))
        row = {"vectors": name, "rows": n, "nq": nq, "nprobe": nprobe, "k": k, "refine": R,
               "ms": {"nearest_k10": round(ms_p, 4), "nearest_k100": round(ms_c, 4), "nearest_k10_refine100": round(ms_r, 4)},
               "refine_over_plain": round(ms_r / ms_p, 4), "all_ms": {"plain": all_p, "k100": all_c, "refined": all_r}}
        print(json.dumps(row), flush=True)
        res["end_to_end"].append(row)


def trained(res):
    """recall@10 of the trained fixture (tests/test_gpu_refine.py) with and without refine=100"""
    from reductive_amd import qmatrix
    from test_gpu_refine import trained_fixture
    m, bits, n_lists, k, R = 8, 4, 64, 10, 100
    x, ys, d2 = trained_fixture()
    nq = ys.shape[0]
    flat = ra.train_pq(m, bits, 10, 1, x, rng=np.random.default_rng(9831))
    qm = qmatrix.QuantizedMatrix(flat, flat.quantize_batch(x)).attach_vectors(x)
    pm = qm.partition(n_lists, vectors=x, rng=np.random.default_rng(9832))
    rm = qm.partition_residual(n_lists, vectors=x, rng=np.random.default_rng(9832))
    truth = np.argsort(d2, axis=1, kind="stable")[:, :k]
    yd = torch.from_numpy(ys).cuda()

    def recall(found):
        f = found.cpu().numpy()
        return float(np.mean([len(set(f[q].tolist()) & set(truth[q].tolist())) / k for q in range(nq)]))
    runs = []
    for nprobe in (1, 8, 64):
        runs.append({"nprobe": nprobe, "refine": R,
                     "recall_at_10_flat": round(recall(pm.nearest(yd, k, nprobe)[1]), 4),
                     "recall_at_10_flat_refined": round(recall(pm.nearest(yd, k, nprobe, refine=R)[1]), 4),
                     "recall_at_10_residual": round(recall(rm.nearest(yd, k, nprobe)[1]), 4),
                     "recall_at_10_residual_refined": round(recall(rm.nearest(yd, k, nprobe, refine=R)[1]), 4)})
        print(json.dumps(runs[-1]), flush=True)
    res["trained_case"] = {"n": x.shape[0], "d": x.shape[1], "M": m, "K": 1 << bits, "n_lists": n_lists, "queries": nq,
                           "k": k, "note": "recall@10 against the true float64 neighbours", "runs": runs}


def main():
    res = {"shape": {"n_asked": N, "d": D}, "warmup": WARM, "reps": REPS, "device": torch.cuda.get_device_name(0),
           "expectation": "kernel <= torch in every cell, the margin growing with nq * R",
           "rows_used": {}, "runs": [], "end_to_end": []}
    trained(res)
    pq = ra.Pq(None, np.random.default_rng(20).standard_normal((15, 256, 20), dtype=np.float32))
    rm = None
    for name, dtype in (("f16", torch.float16), ("f32", torch.float32)):
        x = allocate(N, dtype)
        res["rows_used"][name] = {"rows": x.shape[0], "bytes": x.numel() * x.element_size()}
        cells(res, pq, x, name)
        if rm is None or len(rm) != x.shape[0]:
            rm = None
            rm = synthetic_matrix(x.shape[0])
        end_to_end(res, rm, x, name)
        rm.vectors = None
        del x
        torch.cuda.empty_cache()
    res["misses"] = [{key: r[key] for key in ("vectors", "metric", "nq", "R", "k", "kernel_over_torch")}
                     for r in res["runs"] if not r["kernel_within_expectation"]]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "re-ranking differs from the float64 evaluation"


if __name__ == "__main__":
    main()
