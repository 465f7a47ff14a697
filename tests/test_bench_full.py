"""bench.py --full: a plain run times its steps and prints the line; the CPU baseline and the oracle parity check of the
timed path come with --full alone."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--rows", "200000", *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_cpu_baseline_and_parity_only_with_full():
    plain = bench_line()
    assert plain["steps"] == 2 and len(plain["roofline"]["launch_ms"]) == 2
    assert "cpu_baseline" not in plain and "configs" not in plain
    full = bench_line("--full")
    assert full["metric"] == plain["metric"] and full["unit"] == plain["unit"]
    assert full["cpu_baseline"]["gpu_codes_identical_on_sample"] is True
    assert full["cpu_baseline"]["host_resident_api_identical"] is True
