"""Building a partitioned index with the project's own builder: the device route (on_device=True) against the host route
of the same call in the same run -- which is the code of the parent commit, unchanged.  d = 300, M = 15, K = 256, 1,024
lists; the code matrix is random and is partitioned from its own reconstructions (vectors=None), so nothing but 15 bytes
per row is generated.  One process; wall clock around synchronised calls for the end-to-end cells (one call each: they
take seconds), HIP events (2 warm-up calls, median of 7) for the kernels.
  (a) partition and partition_residual end to end at N_SMALL rows (default 10 M), both routes
  (b) the same at N_BIG rows (default 100 M), training on TRAIN_ROWS rows so that the training, which both routes share,
      does not drown the difference; the host route is run at N_BIG too unless `--no-host-big` (say so in the file)
  (c) the layout kernel against the torch form _Lists._piece uses: stable sort, bincount, cumsum, scatter
  (d) the residual kernel against rows - centroids[assign] on one chunk of 2^20 rows
  (e) the term kernel against the tail of _residual_codes_terms (reconstruct, widen, ten passes) on one chunk
  (f) each kernel beside a device-to-device copy of its output bytes
Before a cell is timed its device result is compared with the host route's: exactly, except the row terms, which are
compared within 2^-23 |t| + 2^-40 sum_j (r^2 + |2 c r|).  Writes JSON (default profiles/index_build_time.json) and prints
the table of DESIGN.md.

usage: python tools/index_build_time.py [out.json] [n_small] [n_big] [--no-host-big]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_search_time import timed  # noqa: E402
from reductive_amd import qmatrix  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "index_build_time.json")
N_SMALL = int(ARGS[1]) if len(ARGS) > 1 else 10_000_000
N_BIG = int(ARGS[2]) if len(ARGS) > 2 else 100_000_000
HOST_BIG = "--no-host-big" not in sys.argv
M, K, DS, N_LISTS, TRAIN_ROWS, ITERS = 15, 256, 20, 1024, 1_000_000, 4
D = M * DS
LIST_TENSORS = ("ids", "list_off", "positions", "codes", "norms")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def same(a, b, names):
    for t in names:
        x, y = getattr(a, t), getattr(b, t)
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            return False
    return bool(np.array_equal(a.centroids, b.centroids))


def terms_within_bound(dev, host, rpq):
    """the device-built residual matrix against the host-built one: row terms within the derived bound, chunk by chunk"""
    cd = dev._centroids_dev
    worst = 0.0
    for r0 in range(0, len(dev), 1 << 20):
        sl = slice(r0, min(len(dev), r0 + (1 << 20)))
        r = rpq.reconstruct_batch_device(dev.codes[sl]).double()
        c2 = 2.0 * cd[dev.lists[sl]].double() * r
        S = (r * r + c2.abs()).sum(1)
        th = host.row_terms[sl].double()
        err = (dev.row_terms[sl].double() - th).abs()
        bound = 2.0 ** -23 * th.abs() + 2.0 ** -40 * S
        worst = max(worst, float((err / bound).max()))
    return worst


def end_to_end(pq, rpq, n, host, res, label):
    codes = torch.randint(0, K, (n, M), dtype=torch.uint8, device="cuda")
    qm = qmatrix.QuantizedMatrix.__new__(qmatrix.QuantizedMatrix)
    qm.pq, qm.codes, qm.norms = pq, codes, None
    kw = dict(n_iterations=ITERS, train_rows=min(TRAIN_ROWS, n))
    for call in ("partition", "partition_residual"):
        extra = dict(residual_pq=rpq) if call == "partition_residual" else {}
        fn = getattr(qm, call)
        dev, dev_s = wall(lambda: fn(N_LISTS, rng=np.random.default_rng(5), on_device=True, **kw, **extra))
        row = {"cell": label, "call": call, "rows": n, "device_s": round(dev_s, 3)}
        if host:
            hst, host_s = wall(lambda: fn(N_LISTS, rng=np.random.default_rng(5), **kw, **extra))
            names = LIST_TENSORS + (("lists",) if call == "partition_residual" else ())
            row.update(host_s=round(host_s, 3), host_over_device=round(host_s / dev_s, 2), same_as_host=same(dev, hst, names))
            if call == "partition_residual":
                row["terms_err_over_bound_max"] = terms_within_bound(dev, hst, rpq)
            del hst
        else:
            row["host_s"] = None
        print(json.dumps(row), flush=True)
        res["runs"].append(row)
        del dev
        torch.cuda.empty_cache()
    del codes, qm


def copy_ms(nbytes):
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a))[0]


def kernels(pq, rpq, res):
    rng = np.random.default_rng(9)
    cd = torch.from_numpy(rng.standard_normal((N_LISTS, D), dtype=np.float32)).cuda()
    for n in (N_SMALL, N_BIG):                                              # (c) the layout
        assign = torch.randint(0, N_LISTS, (n,), dtype=torch.int64, device="cuda")

        def torch_form():
            ids = torch.sort(assign, stable=True).indices
            off = torch.zeros(N_LISTS + 1, dtype=torch.int64, device="cuda")
            off[1:] = torch.cumsum(torch.bincount(assign, minlength=N_LISTS), 0)
            pos = torch.empty_like(ids)
            pos[ids] = torch.arange(n, dtype=torch.int64, device="cuda")
            return ids, off, pos

        got, want = pq.lists_layout_device(assign, N_LISTS, check=True), torch_form()
        ok = all(bool(torch.equal(g, w)) for g, w in zip(got, want))
        del got, want
        k_ms, _ = timed(lambda: pq.lists_layout_device(assign, N_LISTS))
        a32 = assign.int()
        k32_ms, _ = timed(lambda: pq.lists_layout_device(a32, N_LISTS))
        t_ms, _ = timed(torch_form)
        c_ms = copy_ms(16 * n)
        row = {"cell": "c", "kernel": "layout", "rows": n, "same_as_torch": ok, "kernel_ms": round(k_ms, 3),
               "kernel_int32_ids_ms": round(k32_ms, 3), "torch_ms": round(t_ms, 3), "torch_over_kernel": round(t_ms / k_ms, 2),
               "copy_of_output_ms": round(c_ms, 3), "kernel_over_copy": round(k_ms / c_ms, 2)}
        print(json.dumps(row), flush=True)
        res["runs"].append(row)
        del assign, a32
        torch.cuda.empty_cache()
    n = 1 << 20                                                             # (d), (e): one chunk of the build loop
    assign = torch.randint(0, N_LISTS, (n,), dtype=torch.int64, device="cuda")
    x = torch.randn((n, D), device="cuda")
    out = torch.empty_like(x)
    ok = bool(torch.equal(pq.residuals_device(x, assign, cd, out=out, check=True), x - cd[assign]))
    k_ms, _ = timed(lambda: pq.residuals_device(x, assign, cd, out=out))
    t_ms, _ = timed(lambda: x - cd[assign])
    c_ms = copy_ms(4 * n * D)
    row = {"cell": "d", "kernel": "residuals", "rows": n, "same_as_torch": ok, "kernel_ms": round(k_ms, 3), "torch_ms": round(t_ms, 3),
           "torch_over_kernel": round(t_ms / k_ms, 2), "copy_of_output_ms": round(c_ms, 3), "kernel_over_copy": round(k_ms / c_ms, 2)}
    print(json.dumps(row), flush=True)
    res["runs"].append(row)
    codes = rpq.quantize_batch_device(out)
    c = cd[assign]

    def tail():
        r = rpq.reconstruct_batch_device(codes).double()
        return (r * r + 2.0 * c.double() * r).sum(1).float()

    th = tail().double()
    r = rpq.reconstruct_batch_device(codes).double()
    S = (r * r + (2.0 * c.double() * r).abs()).sum(1)
    td = rpq.residual_terms_device(codes, assign, cd, check=True).double()
    worst = float(((td - th).abs() / (2.0 ** -23 * th.abs() + 2.0 ** -40 * S)).max())
    del r, S
    terms = torch.empty(n, device="cuda")
    k_ms, _ = timed(lambda: rpq.residual_terms_device(codes, assign, cd, out=terms))
    t_ms, _ = timed(tail)
    c_ms = copy_ms(4 * n)
    row = {"cell": "e", "kernel": "terms", "rows": n, "err_over_bound_max": worst, "kernel_ms": round(k_ms, 3), "torch_ms": round(t_ms, 3),
           "torch_over_kernel": round(t_ms / k_ms, 2), "copy_of_output_ms": round(c_ms, 3), "kernel_over_copy": round(k_ms / c_ms, 2)}
    print(json.dumps(row), flush=True)
    res["runs"].append(row)


def main():
    rng = np.random.default_rng(31)
    pq = ra.Pq(None, rng.standard_normal((M, K, DS), dtype=np.float32))
    rpq = ra.Pq(None, rng.standard_normal((M, K, DS), dtype=np.float32) * np.float32(0.5))
    res = {"shape": {"d": D, "M": M, "K": K, "n_lists": N_LISTS, "train_rows": TRAIN_ROWS, "kmeans_iterations": ITERS,
                     "n_small": N_SMALL, "n_big": N_BIG},
           "baseline": "the on_device=False route of the same call in the same run (unchanged from the parent commit)",
           "host_route_at_n_big": HOST_BIG, "device": torch.cuda.get_device_name(0), "runs": []}
    end_to_end(pq, rpq, 200_000, True, {"runs": []}, "warm-up")            # handles, pinned staging, the first launches
    end_to_end(pq, rpq, N_SMALL, True, res, "a")
    end_to_end(pq, rpq, N_BIG, HOST_BIG, res, "b")
    kernels(pq, rpq, res)
    res["slower_than_baseline"] = [[r["cell"], r.get("call", r.get("kernel")), r["rows"]] for r in res["runs"]
                                   if (r.get("host_over_device") or r.get("torch_over_kernel") or 2) < 1]
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print("| cell | what | rows | device route / kernel | host route / torch | ratio |")
    print("|---|---|---|---|---|---|")
    for r in res["runs"]:
        if "call" in r:
            print("| %s | %s | %d | %.2f s | %s | %s |" % (r["cell"], r["call"], r["rows"], r["device_s"],
                                                         "%.2f s" % r["host_s"] if r["host_s"] else "-", r.get("host_over_device", "-")))
        else:
            print("| %s | %s | %d | %.3f ms | %.3f ms | %.2f (%.2f x a copy of the output) |"
                  % (r["cell"], r["kernel"], r["rows"], r["kernel_ms"], r["torch_ms"], r["torch_over_kernel"], r["kernel_over_copy"]))
    assert all(r.get("same_as_host", True) and r.get("same_as_torch", True) for r in res["runs"]), "the device route differs"
    assert all(r.get("terms_err_over_bound_max", 0) <= 1 and r.get("err_over_bound_max", 0) <= 1 for r in res["runs"])


if __name__ == "__main__":
    main()
