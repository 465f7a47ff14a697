"""The encode dispatch, on the CPU: which kernel (with its template arguments), grid, block and dynamic LDS serve each call
of a fixed list that covers every border of the dispatch rules, with the call's status, pqhip_last_encode_kernel and the
launch log.  tests/mock_hip/ builds every translation unit of libpqhip against a mock HIP runtime that records each launch;
`san_driver dispatch` walks the calls and prints what was launched.  The output must equal tests/golden/encode_dispatch.txt:
a dispatch change shows up here as a diff, not only on a GPU.  (After an intended dispatch change, regenerate the golden
file with `tests/mock_hip/build/san_driver dispatch > tests/golden/encode_dispatch.txt` and review the diff.)"""
import difflib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock_hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "encode_dispatch.txt")


def test_encode_dispatch_trace_matches_golden():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    build = subprocess.run(["make", "-C", MOCK, "-s", "-j8"], capture_output=True, text=True, timeout=1500)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(MOCK, "build", "san_driver"), "dispatch"], capture_output=True, text=True, env=env,
                         timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    with open(GOLDEN) as f:
        want = f.read()
    if run.stdout != want:
        diff = difflib.unified_diff(want.splitlines(), run.stdout.splitlines(), "golden", "now", lineterm="", n=1)
        pytest.fail("encode dispatch differs from %s:\n%s" % (os.path.relpath(GOLDEN, ROOT), "\n".join(list(diff)[:200])))
