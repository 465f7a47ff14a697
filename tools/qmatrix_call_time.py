"""Wall time of one search call on the three resident matrices, Python included: the A/B of a change to
reductive_amd/qmatrix.py that leaves the device work as it is (profiles/qmatrix_refactor_ab.json).

Series: nearest(q, 10) for one query on the flat, partitioned and residual matrix of the fixture `world` of
tests/test_gpu_qmatrix_packed4.py (M = 4; 3,000 rows, 16 lists, all lists probed), and within(q, radius) on the flat
matrix with the radius of the 10th neighbour.  Each call is timed from before the call to after torch.cuda.synchronize();
the figure is the median of 300 calls after 30 warm-up calls, in microseconds.

usage (on a GPU):  python tools/qmatrix_call_time.py run LABEL [DIRECTORY HOLDING THE reductive_amd TO TIME] > RUN.json
                   python tools/qmatrix_call_time.py combine PARENT_1.json PARENT_2.json CHANGE.json > AB.json
Each run is a fresh process; PQHIP_LIB lets a second Python package use the library of the first."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, WARMUP = 300, 30


def run(label, package_dir=None):
    sys.path.insert(0, os.path.abspath(package_dir or ROOT))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import reductive_amd as ra
    import test_gpu_qmatrix_packed4 as fixture
    ra.lib()
    w = fixture.world(ra, 4)
    q = torch.from_numpy(w.queries[0]).cuda()
    radius = float(w.m["flat"].nearest(q, 10)[0][9])
    series = {"flat.nearest": lambda: w.m["flat"].nearest(q, 10),
              "lists.nearest": lambda: w.m["lists"].nearest(q, 10, fixture.N_LISTS),
              "residual.nearest": lambda: w.m["residual"].nearest(q, 10, fixture.N_LISTS),
              "flat.within": lambda: w.m["flat"].within(q, radius)}
    out = {"label": label, "calls": CALLS, "warmup": WARMUP, "median_us": {}, "p10_us": {}, "p90_us": {}}
    for name, call in series.items():
        times = []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
        times = sorted(times[WARMUP:])
        out["median_us"][name] = round(statistics.median(times), 2)
        out["p10_us"][name] = round(times[CALLS // 10], 2)
        out["p90_us"][name] = round(times[CALLS * 9 // 10], 2)
    print(json.dumps(out))


def combine(parent_1, parent_2, change):
    runs = [json.load(open(p)) for p in (parent_1, parent_2, change)]
    rows = []
    for name in runs[0]["median_us"]:
        a, b, c = (r["median_us"][name] for r in runs)
        spread = abs(a - b)
        low, high = min(a, b) - spread, max(a, b) + spread
        rows.append({"series": name, "parent_us": [a, b], "change_us": c, "spread_us": round(spread, 2),
                     "allowed_us": [round(low, 2), round(high, 2)],
                     "verdict": "within" if low <= c <= high else "faster" if c < low else "slower"})
    method = ("one GPU call, three fresh processes in the order parent, change, parent; per series the median wall time of "
              "%d synchronised calls after %d warm-up calls; spread = the difference of the two parent medians; allowed = "
              "[min - spread, max + spread] of the parent medians" % (CALLS, WARMUP))
    one_per_line = lambda items: ",\n  ".join(json.dumps(item) for item in items)
    print('{"method": %s,\n "rows": [\n  %s],\n "runs": [\n  %s]}' % (json.dumps(method), one_per_line(rows), one_per_line(runs)))


if __name__ == "__main__":
    {"run": run, "combine": combine}[sys.argv[1]](*sys.argv[2:])
