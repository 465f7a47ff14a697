"""The encode dispatch golden file (tests/golden/encode_dispatch.txt, written by `tests/mock_hip/build/san_driver dispatch`) as
call records, shared by the CPU test of the file itself (test_dispatch_golden_parse.py) and its replay on the device
(test_gpu_dispatch_replay.py).

Each non-indented line of the file is one call:
    pqhip_set_encode_variant(<v>): status <s>
    <pq | opq | opq(opq_fused=0)> M=.. K=.. dsub=.. v=.. cb=.. n=..[ x_rs=d+..][ x_off=..][ o_rs=M+..][ c_off=..]
        [ candidate_tables=0]: <status> "<pqhip_last_encode_kernel>" [<launch log>]
    kmeans M=.. K=.. dsub=.. n=.. iterations=.. kmeans_no_graph=..: <status> [<launch log>]
The indented lines under a call are the mock's launch geometry (grids, LDS bytes): specific to the mock, not parsed.  A line
that matches none of the forms is an error."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "encode_dispatch.txt")

# Calls of the golden file that are never replayed on a device: 2^46 rows, which the mock runs over a one-row buffer (its
# kernels do not run) and a device would read far outside any allocation.  Their status and kernel are checked on the CPU
# only (test_encode_dispatch.py).
EXCLUDED = (
    "pq M=4 K=64 dsub=2 v=0 cb=1 n=70368744177664",
    "pq M=64 K=64 dsub=2 v=0 cb=1 n=70368744177664",
)


@dataclass(frozen=True)
class Call:
    kind: str                        # "variant", "pq", "opq", "kmeans"
    status: int
    M: int = 0
    K: int = 0
    dsub: int = 0
    variant: int = 0
    code_bytes: int = 1
    n: int = 0
    x_pad: int = 0                   # row stride d + x_pad floats
    x_off: int = 0                   # rows start x_off floats into the buffer
    o_pad: int = 0                   # code row stride M + o_pad elements
    c_off: int = 0                   # codes start c_off bytes into the buffer
    tables: int = 1                  # context option candidate_tables
    fused: int = 1                   # context option opq_fused
    iterations: int = 0              # kmeans only
    no_graph: int = 0                # kmeans only: context option kmeans_no_graph
    kernel: str = ""                 # pqhip_last_encode_kernel (pq / opq)
    log: str = ""                    # pqhip_launch_log
    line: int = field(default=0, compare=False)   # 1-based line number in the golden file

    @property
    def d(self):
        return self.M * self.dsub

    def header(self):
        """The call's line up to the colon (what san_driver prints before the status)."""
        if self.kind == "variant":
            return "pqhip_set_encode_variant(%d)" % self.variant
        if self.kind == "kmeans":
            return "kmeans M=%d K=%d dsub=%d n=%d iterations=%d kmeans_no_graph=%d" % (
                self.M, self.K, self.dsub, self.n, self.iterations, self.no_graph)
        name = "pq" if self.kind == "pq" else ("opq" if self.fused else "opq(opq_fused=0)")
        s = "%s M=%d K=%d dsub=%d v=%d cb=%d n=%d" % (name, self.M, self.K, self.dsub, self.variant, self.code_bytes, self.n)
        for tag, v in (("x_rs=d+", self.x_pad), ("x_off=", self.x_off), ("o_rs=M+", self.o_pad), ("c_off=", self.c_off)):
            if v:
                s += " %s%d" % (tag, v)
        if not self.tables:
            s += " candidate_tables=0"
        return s

    def format(self):
        """The whole line as san_driver prints it."""
        if self.kind == "variant":
            return "%s: status %d" % (self.header(), self.status)
        if self.kind == "kmeans":
            return "%s: %d [%s]" % (self.header(), self.status, self.log)
        return '%s: %d "%s" [%s]' % (self.header(), self.status, self.kernel, self.log)


_VARIANT = re.compile(r"pqhip_set_encode_variant\((-?\d+)\): status (\d+)")
_ENCODE = re.compile(r"(pq|opq|opq\(opq_fused=0\)) M=(\d+) K=(\d+) dsub=(\d+) v=(\d+) cb=(\d+) n=(\d+)"
                     r"(?: x_rs=d\+(\d+))?(?: x_off=(\d+))?(?: o_rs=M\+(\d+))?(?: c_off=(\d+))?( candidate_tables=0)?"
                     r': (\d+) "([^"]*)" \[([^\]]*)\]')
_KMEANS = re.compile(r"kmeans M=(\d+) K=(\d+) dsub=(\d+) n=(\d+) iterations=(\d+) kmeans_no_graph=(\d+): (\d+) \[([^\]]*)\]")


def parse_line(text, line=0):
    m = _VARIANT.fullmatch(text)
    if m:
        return Call("variant", int(m[2]), variant=int(m[1]), line=line)
    m = _ENCODE.fullmatch(text)
    if m:
        opt = [int(g) if g else 0 for g in m.groups()[7:11]]
        return Call("pq" if m[1] == "pq" else "opq", int(m[13]), M=int(m[2]), K=int(m[3]), dsub=int(m[4]), variant=int(m[5]),
                    code_bytes=int(m[6]), n=int(m[7]), x_pad=opt[0], x_off=opt[1], o_pad=opt[2], c_off=opt[3],
                    tables=0 if m[12] else 1, fused=0 if m[1] == "opq(opq_fused=0)" else 1, kernel=m[14], log=m[15], line=line)
    m = _KMEANS.fullmatch(text)
    if m:
        return Call("kmeans", int(m[7]), M=int(m[1]), K=int(m[2]), dsub=int(m[3]), n=int(m[4]), iterations=int(m[5]),
                    no_graph=int(m[6]), log=m[8], line=line)
    raise ValueError("%s:%d: not a golden call line: %r" % (os.path.relpath(GOLDEN, ROOT), line, text))


def parse(path=GOLDEN):
    """Every call of the golden file, in file order (ValueError on a line of no known form)."""
    calls = []
    with open(path) as f:
        for i, text in enumerate(f.read().splitlines(), 1):
            if text.startswith("    ") and text.strip():
                continue                                         # the mock's launch geometry
            calls.append(parse_line(text, i))
    return calls


def case_ids(calls):
    """pytest ids: the header, with "#2", "#3", .. on repeated headers (the list visits some calls twice)."""
    seen, ids = {}, []
    for c in calls:
        h = c.header()
        seen[h] = seen.get(h, 0) + 1
        ids.append(h if seen[h] == 1 else "%s#%d" % (h, seen[h]))
    return ids


def replay_plan(calls):
    """The calls the device replays: all but EXCLUDED."""
    return [c for c in calls if c.header() not in EXCLUDED]


def centroids(M, K, dsub):
    """san_driver's dispatch::centroids(): centroid i of the flat [M][K][dsub] array is ((i * 2654435761 mod 2^64) >> 8 & 0xffff)
    / 65536 as float32 -- multiples of 2^-16 in [0, 1)."""
    i = np.arange(M * K * dsub, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (i * np.uint64(2654435761)) >> np.uint64(8)
    return ((h & np.uint64(0xFFFF)).astype(np.float32) / np.float32(65536)).reshape(M, K, dsub)
