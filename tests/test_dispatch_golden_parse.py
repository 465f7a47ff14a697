"""The encode dispatch golden file as data (tests/dispatch_golden.py): every line parses, formats back to itself, and is
either replayed on the device by test_gpu_dispatch_replay.py or one of the named exclusions; the replay's centroids are the
ones the golden's dispatch was decided on (san_driver centroids)."""
import os
import subprocess

import numpy as np
import pytest

import dispatch_golden as dg

MOCK = os.path.join(dg.ROOT, "tests", "mock_hip")


def test_every_golden_line_parses_and_formats_back():
    with open(dg.GOLDEN) as f:
        lines = [t for t in f.read().splitlines() if not (t.startswith("    ") and t.strip())]
    calls = dg.parse()
    assert len(calls) == len(lines)
    for c, text in zip(calls, lines):
        assert c.format() == text, c.line
    kinds = {k: sum(c.kind == k for c in calls) for k in ("variant", "pq", "opq", "kmeans")}
    assert kinds["variant"] == 14 and kinds["kmeans"] == 16 and kinds["pq"] > 700 and kinds["opq"] > 200, kinds


def test_unknown_line_is_an_error():
    for bad in ("pq M=2 K=16 dsub=2 v=0 cb=1 n=4096 x_pad=3: 0 \"k\" [k]", "pq M=2 K=16 dsub=2 v=0 cb=1 n=4096: 0 [k]",
                "kmeans M=2 K=8 dsub=1 n=5 iterations=1: 0 []", "something else", ""):
        with pytest.raises(ValueError):
            dg.parse_line(bad, 1)


def test_replay_covers_every_call_but_the_named_exclusions():
    calls = dg.parse()
    plan = dg.replay_plan(calls)
    left = [c.header() for c in calls if c not in plan]
    assert sorted(left) == sorted(dg.EXCLUDED), left
    assert all(c.n == 1 << 46 for c in calls if c.header() in dg.EXCLUDED)
    assert max(c.n for c in plan) <= 3_000_000
    ids = dg.case_ids(plan)
    assert len(set(ids)) == len(ids) == len(calls) - 2
    print("golden: %d calls, %d replayed on the device, %d excluded (%s)"
          % (len(calls), len(plan), len(left), "; ".join(dg.EXCLUDED)))


def test_centroids_match_san_driver():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    build = subprocess.run(["make", "-C", MOCK, "-s", "-j8"], capture_output=True, text=True, timeout=1500)
    assert build.returncode == 0, build.stderr[-3000:]
    for M, K, dsub in ((1, 4, 2), (2, 128, 2), (15, 256, 20), (3, 1000, 8), (2, 16, 1100), (72, 64, 2)):
        run = subprocess.run([os.path.join(MOCK, "build", "san_driver"), "centroids", str(M), str(K), str(dsub)],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        want = np.array([int(t, 16) for t in run.stdout.split()], dtype=np.uint32)
        got = dg.centroids(M, K, dsub)
        assert got.shape == (M, K, dsub) and got.dtype == np.float32
        assert np.array_equal(got.reshape(-1).view(np.uint32), want), (M, K, dsub)
