"""The searches among given rows against what a caller does today: 100 M resident rows, K = 256, M = 15 and 48, k = 10.

Shared list (lims None): the allowed rows of a filter of density 10 %, 1 %, 0.1 % and 0.01 %, as sorted and as shuffled
ids, 1 / 8 / 32 queries; baseline: the existing masked exhaustive search with the mask of the same set.
CSR: 256 queries x {1,024, 100 k} ids each; baseline: one mask packed and one masked search run per query.
HIP events, median of 7 after 2 warm-up calls, both sides in one process on the same data; before a cell is timed, the
first and the last query of the candidate search must equal the baseline's bit for bit.

Recorded beside the timings, as information and not as an assertion: per (M, order, nq) the pair of adjacent densities
between which the candidate search overtakes the masked one (`crossover`), and the shared-list cells with nq >= 8 that
the single-query producer loses to the eight-queries-per-pass masked search (`lost_to_multi_query`): the case for a
later multi-query producer.  The run only fails when a result is not exact.  Writes JSON (default
profiles/adc_among_time.json).

usage: python tools/adc_among_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from adc_search_time import timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_among_time.json")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
MS = [int(a) for a in sys.argv[3:]] or [15, 48]
K, KTOP = 256, 10
DENSITIES = (0.1, 0.01, 0.001, 0.0001)


def same(got, want, rows):
    return all(bool(torch.equal(g[j], w[j])) for g, w in ((got[0].view(torch.int32), want[0].view(torch.int32)), (got[1], want[1]))
               for j in rows)


def shape(res, M):
    g = torch.Generator(device="cuda").manual_seed(17 + M)
    pq = ra.Pq(None, np.random.default_rng(17 + M).standard_normal((M, K, 4), dtype=np.float32))
    codes = torch.randint(0, K, (N, M), dtype=torch.uint8, device="cuda", generator=g)
    ys = torch.randn((256, M * 4), device="cuda", generator=g)
    tables = pq.adc_tables_device(ys)

    # ---- shared list against the masked exhaustive search of the same set ----
    for density in DENSITIES:
        flags = torch.rand(N, device="cuda", generator=g) < density
        words = pq.pack_row_mask_device(flags)
        rows = torch.nonzero(flags)[:, 0].contiguous()
        del flags
        for order in ("sorted", "shuffled"):
            ids = rows if order == "sorted" else rows[torch.randperm(rows.shape[0], device="cuda", generator=g)].contiguous()
            for nq in (1, 8, 32):
                t = tables[:nq].contiguous()
                among = lambda: pq.adc_among_device(codes, t, ids, KTOP)
                masked = lambda: pq.adc_search_device(codes, t, KTOP, allow=words)
                ra.launch_log(reset=True)
                got = among()
                torch.cuda.synchronize()
                log = ra.launch_log(reset=True)
                exact = same(got, masked(), sorted({0, nq - 1}))
                a_ms, a_all = timed(among)
                m_ms, m_all = timed(masked)
                row = {"cell": "shared", "M": M, "density": density, "n_ids": int(ids.shape[0]), "order": order, "nq": nq,
                       "among_ms": round(a_ms, 4), "masked_ms": round(m_ms, 4), "ratio": round(a_ms / m_ms, 4), "exact": exact,
                       "launches": log, "all_ms": {"among": a_all, "masked": m_all}}
                print(json.dumps(row), flush=True)
                res["runs"].append(row)
        del words, rows

    # ---- CSR against one packed mask and one masked search per query ----
    nq = 256
    t = tables[:nq].contiguous()
    for per_query in (1024, 100_000):
        ids = torch.randint(0, N, (nq * per_query,), dtype=torch.int64, device="cuda", generator=g)
        lims = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * per_query
        among = lambda: pq.adc_among_device(codes, t, ids, KTOP, lims=lims)

        def today(queries=range(nq)):
            out = []
            for q in queries:
                flags = torch.zeros(N, dtype=torch.uint8, device="cuda")
                flags[ids[q * per_query:(q + 1) * per_query]] = 1
                out.append(pq.adc_search_device(codes, t[q], KTOP, allow=pq.pack_row_mask_device(flags)))
            return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
        got = among()
        ends = [0, nq - 1]
        want = today(ends)
        # random ids may repeat inside a query: a repeated row comes back twice from the candidate search only
        distinct = all(int(torch.unique(ids[q * per_query:(q + 1) * per_query]).shape[0]) == per_query for q in ends)
        exact = (not distinct) or same((got[0][ends], got[1][ends]), want, [0, 1])
        a_ms, a_all = timed(among)
        m_ms, m_all = timed(today)
        row = {"cell": "csr", "M": M, "nq": nq, "ids_per_query": per_query, "among_ms": round(a_ms, 4),
               "mask_and_search_per_query_ms": round(m_ms, 4), "ratio": round(a_ms / m_ms, 4), "exact": exact,
               "compared": distinct, "all_ms": {"among": a_all, "today": m_all}}
        print(json.dumps(row), flush=True)
        res["runs"].append(row)
        del ids, lims


def summarise(res):
    shared = [r for r in res["runs"] if r["cell"] == "shared"]
    cross = []
    for M in MS:
        for order in ("sorted", "shuffled"):
            for nq in (1, 8, 32):
                cells = {r["density"]: r["ratio"] for r in shared if (r["M"], r["order"], r["nq"]) == (M, order, nq)}
                pair = None
                for hi, lo in zip(DENSITIES, DENSITIES[1:]):
                    if hi in cells and lo in cells and cells[hi] > 1.0 >= cells[lo]:
                        pair = [hi, lo]
                where = pair if pair else ("above %g" % DENSITIES[0] if cells and cells[DENSITIES[0]] <= 1.0 else "below %g" % DENSITIES[-1])
                cross.append({"M": M, "order": order, "nq": nq, "among_overtakes_between": where})
    res["crossover"] = cross
    res["lost_to_multi_query"] = [{key: r[key] for key in ("M", "density", "order", "nq", "among_ms", "masked_ms", "ratio")}
                                  for r in shared if r["nq"] >= 8 and r["ratio"] > 1.0]


def main():
    assert N < (1 << 31)
    res = {"shape": {"n": N, "K": K, "M": MS, "k": KTOP}, "warmup": 2, "reps": 7, "device": torch.cuda.get_device_name(0), "runs": []}
    for M in MS:
        shape(res, M)
        torch.cuda.empty_cache()
    summarise(res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    assert all(r["exact"] for r in res["runs"]), "a candidate search differs from its baseline"


if __name__ == "__main__":
    main()
