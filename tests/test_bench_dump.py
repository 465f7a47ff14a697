"""bench.py --dump-outputs: what the timed path computed in its last step, as float32 .npy files of at most 64 MB in all.
CPU: the row sample of large outputs.  GPU: the dumped codes of a timed encode run are the oracle's codes of the bench's own
seeded input, and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_sample_is_fixed_bounded_and_keeps_head_and_tail():
    x = np.arange(3_000_000 * 5, dtype=np.int64).reshape(3_000_000, 5) % 251
    a = bench.dump_sample(x.astype(np.uint8), 1_000_000)
    assert a.dtype == np.float32 and a.nbytes <= 1_000_000 and a.shape == (50_000, 5)
    assert (a[:256] == x[:256]).all() and (a[-256:] == x[-256:]).all()
    assert a.tobytes() == bench.dump_sample(x.astype(np.uint8), 1_000_000).tobytes()
    d = np.arange(4 * 1000, dtype=np.float32).reshape(4, 1000)
    s = bench.dump_sample(d, 4 * 4 * 100, axis=1)
    assert s.shape == (4, 100) and (s[:, :25] == d[:, :25]).all() and (s[:, -25:] == d[:, -25:]).all()
    assert bench.dump_sample(d, 1 << 20).tobytes() == d.tobytes()             # small outputs: whole


@pytest.mark.gpu
def test_dumped_codes_are_the_oracle_codes_of_the_timed_input(tmp_path):
    import torch
    from oracle import pq_oracle as orc
    rows, steps = 1_100_000, 3                    # 66 MB of float32 codes: sampled to the budget
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--rows", str(rows), "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == steps and len(rec["roofline"]["launch_ms"]) == steps
    assert sorted(os.listdir(tmp_path)) == ["codes.npy"]
    assert os.path.getsize(tmp_path / "codes.npy") <= 64_000_000
    got = np.load(tmp_path / "codes.npy")
    assert got.dtype == np.float32
    x = bench.Bench.normal_rows(types.SimpleNamespace(torch=torch, dev=torch.device("cuda", 0)), rows, 300, 42).cpu().numpy()
    want = orc.quantize_batch(synth.normalish(43, (15, 256, 20)), x, n_threads=bench.host_cores())
    assert got.tobytes() == bench.dump_sample(want, bench.DUMP_BYTES).tobytes()
