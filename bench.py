#!/usr/bin/env python3
"""bench.py -- headline measurement: vectors/s of Pq::quantize_batch (d=300, M=15, K=256) on
MI355X, inputs resident in HBM, through the C ABI of libpqhip.so.

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one batch: rows_per_gpu synthetic fp32 vectors already
in HBM -> u8 codes in HBM.  With N > 1 every rank owns an independent row shard (the path has no
exchange step: no collective on the data path, "weak" scaling); the only collectives are the
barrier and the max-reduction of the elapsed time.  Rank 0 prints ONE JSON line.

A plain run times the headline (BASELINE.json configs[1]) and prints its line, with the roofline
figures of its own timed steps; nothing else runs.  `--full` adds what takes work of its own: the
CPU baseline and oracle parity check of every timed path, the store-ceiling runs of the reconstruct
and lookup workloads and, in the default single-GPU run, in the same process and the same JSON
line (key "configs"), the other single-GPU BASELINE configs with their own roofline / cpu_baseline
/ parity records, and after them the reference's own shapes (key "reference_shapes").  The configs:
    configs[2]  Opq rotate+encode 10 M x 300          (--workload opq_encode)
    configs[3]  Pq::reconstruct_batch 100 M codes      (--workload reconstruct --rows 100000000)
    configs[4]  one GPU's shard (12.5 M rows) of the 100 M x 768, M=48 encode  (--workload encode_d768)
`--no-sub-configs` skips them; `--workload X` runs X alone as the top-level record.  `--dump-outputs`
writes the outputs of every timed path of the default run, so it times the other configs as well.
`--in-process N` instead drives the LIBRARY's own sharder (pqhip_ctx_create(devices) +
pqhip_quantize_batch_f32 over one host batch, codes concatenated host-side: north_star's form).
"""
import argparse
import hashlib
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: FP32 matrix peak (dense)
PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec peak

# workload -> (label, default shape (d, M, K), default rows per GPU)
WORKLOADS = {
    "encode": ("Pq::quantize_batch {rows} x d={d} fp32 per GPU, M={m}, K={k} (BASELINE configs[1]: 10M on 1 MI355X)", (300, 15, 256), 10_000_000),
    "opq_encode": ("Opq rotate+encode {rows} x d={d} per GPU, M={m}, K={k} (BASELINE configs[2])", (300, 15, 256), 10_000_000),
    "reconstruct": ("Pq::reconstruct_batch {rows} u8 codes -> d={d} fp32 per GPU (BASELINE configs[3]: 100M codes on 1 MI355X)", (300, 15, 256), 10_000_000),
    "opq_reconstruct": ("Opq reconstruct_batch {rows} u8 codes -> gather -> x P^T -> d={d} fp32 per GPU (SURVEY 8a row a8 with a projection)", (300, 15, 256), 10_000_000),
    "encode_d768": ("Pq encode {rows} x d={d} per GPU, M={m}, K={k}: one GPU's shard of BASELINE configs[4] (100M x d=768, M=48 batch-sharded across 8 MI355X = 12.5M rows per GPU)", (768, 48, 256), 12_500_000),
    "lookup": ("embedding lookup: {rows} random rows of a resident 10M x {m} u8 code matrix -> select + reconstruct + per-row rescale, d={d} fp32 (SURVEY 8f rank 2)", (300, 15, 256), 10_000_000),
    "adc_scan": ("asymmetric-distance scan: {rows} resident u8 code rows (M={m}) against the K={k}-entry lookup tables of one query, d={d} (SURVEY 8f rank 4)", (300, 15, 256), 100_000_000),
    "opq_train": ("device part of Opq::train_iteration (rotate, k-means update, quantize->reconstruct, X^T.R), {rows} x d={d} per GPU, M={m}, K={k}", (300, 15, 256), 10_000_000),
    "kmeans": ("kmeans_iteration on all {m} subquantizers (training step; SURVEY 8f rank 1), {rows} x d={d} per GPU, K={k}", (300, 15, 256), 10_000_000),
}

# the default one-GPU run: the other single-GPU BASELINE configs (key, workload, rows) ...
SUB_CONFIGS = (("configs[2]", "opq_encode", 10_000_000),
               ("configs[3]", "reconstruct", 100_000_000),
               ("configs[4]_one_gpu_shard", "encode_d768", 12_500_000))
# ... and the reference's OWN shapes (not BASELINE configs): its criterion bench (benches/pq.rs:9-10) and its statistical
# test (pq.rs:431-440), 10 M rows each, same record form.  (Third: M = d / 2 two-float sub-vectors at the headline dimension
# -- the shape finalfusion's own quantizer front end is remembered to default to; nothing in the reference's sources pins it.)
REFERENCE_SHAPES = (("benches_pq_rs_d128_M16_K16", (128, 16, 16)), ("pq_rs_test_d20_M10_K128", (20, 10, 128)),
                    ("half_dim_d300_M150_K256", (300, 150, 256)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=None, help="rows per GPU (default: the workload's BASELINE size)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="encode")
    ap.add_argument("--d", type=int, default=None)
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--k", type=int, default=None, help="centroids per subquantizer (u8 codes up to 256, 32-bit codes beyond)")
    ap.add_argument("--variant", type=int, default=0, help="0 auto, 1 anchor kernel, 2 MFMA kernel")
    ap.add_argument("--cpu-rows", type=int, default=2_000_000, help="rows of the CPU-baseline sample")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline figure: CPU baselines and oracle parity checks, store-ceiling runs, and the "
                         "configs[2..4] and reference-shape records of the default run")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baselines, parity checks and store ceilings")
    ap.add_argument("--no-sub-configs", action="store_true",
                    help="headline only: skip the configs[2..4] and reference-shape records of a --full or --dump-outputs run")
    ap.add_argument("--sub-steps", type=int, default=10, help="timed steps of every sub-config (after 2 warm-up steps)")
    ap.add_argument("--in-process", type=int, default=0, metavar="N",
                    help="drive the library's own row sharder over N device slots from ONE process and one host batch")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend for the barrier / max-reduction (gloo: rehearsals)")
    ap.add_argument("--single-device", action="store_true",
                    help="rehearsal on a one-GPU box: every rank / slot uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--queries", type=int, default=1, help="adc_scan workload: queries scanned per step (8 share one pass over the codes)")
    ap.add_argument("--record-bytes", type=int, default=None, help="lookup workload: interleaved records of this many bytes (codes + scale of a row together) instead of a code matrix and a scale vector")
    ap.add_argument("--lookup-codes", type=int, default=10_000_000, help="lookup workload: rows of the resident code matrix")
    ap.add_argument("--fast-cross", action="store_true",
                    help="opq_train workload: X^T.R as a plain split-K product (context option cross_product_exact = 0: float tolerance, no per-block partials)")
    ap.add_argument("--dry-run", action="store_true",
                    help="exercise sharding/reduction/printing only (CPU, gloo); no GPU work")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what every timed path of the run computed in its last step to DIR/<name>.npy "
                         "(float32, at most 64 MB in all; larger outputs are sampled: see dump_sample)")
    return ap.parse_args()


def host_cores():
    """CPU cores this process may actually use: the cgroup CPU quota (cgroup v2 `cpu.max`, v1 `cpu.cfs_quota_us`)
    and the scheduler affinity, whichever is smaller -- NOT os.cpu_count(), which reports the host's logical CPUs
    (256 on the GPU boxes, of which a one-GPU job is granted 16: `cpu.max = 1600000 100000`)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(quota + 0.5)))
    return max(1, n)


def per_step(log, steps):
    """'k_a x20 + k_b x60' over 20 timed steps -> 'k_a + k_b x3' (counts that are not whole multiples stay as logged)."""
    out = []
    for part in [p for p in log.split(" + ") if p]:
        name, _, cnt = part.rpartition(" x")
        if not name or not cnt.isdigit():
            name, cnt = part, "1"
        c = int(cnt)
        if steps > 0 and c % steps == 0:
            c //= steps
            out.append(name if c == 1 else "%s x%d" % (name, c))
        else:
            out.append("%s x%d/%d steps" % (name, c, steps))
    return " + ".join(out)


def shard_ranges(world, rows):
    """weak scaling: rank r owns global rows [r*rows, (r+1)*rows)."""
    return [[r * rows, (r + 1) * rows] for r in range(world)]


def source_hash():
    """sha256 over the kernel / C-ABI sources: identifies the build a PMC pass was taken on
    (.git does not travel to the GPU box, so a commit id is not available there)."""
    h = hashlib.sha256()
    base = os.path.join(ROOT, "reductive_amd", "csrc")
    for name in sorted(os.listdir(base)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(base, name), "rb").read())
    return h.hexdigest()[:16]


DUMP_BYTES = 60_000_000           # --dump-outputs: array bytes of all files together (64 MB with room for the .npy headers)
OUTPUT_NAMES = {"encode": "codes", "encode_d768": "codes", "opq_encode": "codes", "reconstruct": "reconstruction",
                "opq_reconstruct": "reconstruction", "lookup": "reconstruction", "adc_scan": "distances"}


def dump_sample(t, budget, axis=0):
    """float32 host copy of the tensor / array t, or, when that exceeds `budget` bytes, of a fixed sample of its rows along
    `axis`: the first and last 256 (ragged last tiles live there) and a draw of numpy's default_rng(0) from the rest, in row
    order.  The sample depends on the shape alone, so two runs with the same arguments dump the same rows."""
    import numpy as np
    n = t.shape[axis]
    keep = max(1, budget // max(1, 4 * (int(np.prod(t.shape)) // max(1, n))))
    if n > keep:
        e = min(256, keep // 4)
        rest = np.random.default_rng(0).choice(n - 2 * e, keep - 2 * e, replace=False) + e
        idx = np.sort(np.concatenate([np.arange(e), rest, np.arange(n - e, n)]))
        if hasattr(t, "index_select"):           # torch tensor: sampled on its device, only the sample is copied
            import torch
            t = t.index_select(axis, torch.from_numpy(idx).to(t.device))
        else:
            t = np.take(t, idx, axis=axis)
    if hasattr(t, "cpu"):
        t = t.cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def write_outputs(path, outputs):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), a)


def load_pmc_traffic(workload, rows, d, m, k, suffix=""):
    """HBM bytes per launch of the workload's dominant kernel from the committed rocprofv3 --pmc
    passes (profiles/pmc_traffic.json, written by tools/pmc_summarize.py).  Refused (None + reason)
    unless the record was taken for exactly this workload size AND on the kernel sources of this build."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        rec = json.load(open(p))["entries"].get("%s@%d@d%d_m%d_k%d%s" % (workload, rows, d, m, k, suffix))
    except Exception:
        return None, "no profiles/pmc_traffic.json"
    if not rec:
        return None, "no PMC pass for this workload size"
    if rec.get("source_hash") != source_hash():
        return None, "stale: PMC pass taken on kernel sources %s, this build is %s" % (rec.get("source_hash"), source_hash())
    return rec, None


class Bench:
    """One GPU's view of the benchmark: the workloads share the context, the clock helpers and the
    barrier; every workload returns a self-contained record (value, roofline, cpu_baseline, parity)."""

    def __init__(self, args, rank, world, local_rank, barrier):
        import torch
        import reductive_amd
        from reductive_amd.pq import _Ctx
        self.args, self.rank, self.world, self.barrier = args, rank, world, barrier
        self.torch = torch
        self.ra = reductive_amd
        torch.cuda.set_device(local_rank)
        self.dev = torch.device("cuda", local_rank)
        reductive_amd.lib()                       # fails loudly if the HIP library is missing
        self.ctx = _Ctx(devices=[local_rank])     # one process per GPU

    # ---- timing: K steps between barrier + synchronize pairs; HIP events per step on the launch stream
    def timed(self, step, steps, warmup):
        torch = self.torch
        for _ in range(warmup):
            step()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize()
        self.barrier()
        torch.cuda.synchronize()
        self.ra.launch_log(reset=True)               # from here on: the launches of the K timed steps only
        t0 = time.perf_counter()
        for a, b in evs:
            a.record()                            # torch's current stream = the stream passed to the C ABI
            step()
            b.record()
        torch.cuda.synchronize()
        self.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        per = [a.elapsed_time(b) for a, b in evs]
        self.last_launch_ms = [round(v, 3) for v in per]
        return elapsed, sum(per) / len(per), min(per), max(per)

    def normal_rows(self, rows, d, seed):
        torch = self.torch
        g = torch.Generator(device=self.dev).manual_seed(seed)
        src = torch.empty((rows, d), device=self.dev, dtype=torch.float32)
        for r0 in range(0, rows, 1 << 20):        # N(0,1) like benches/pq.rs:9, generated in HBM
            src[r0:r0 + (1 << 20)].normal_(generator=g)
        return src

    def run(self, workload, rows, d, m, k, steps, warmup, cpu=True, dump=0):
        """dump > 0: the record carries "outputs", what the last timed step computed, in at most `dump` bytes (dump_sample)."""
        import numpy as np
        import synth
        torch, args = self.torch, self.args
        dsub = d // m
        flop_enc = 2 * k * d                      # distance GEMM only
        bytes_vec = 4 * d + m                     # algorithmic HBM bytes per vector
        q = synth.normalish(43, (m, k, dsub))     # same codebook on every rank (replicated)
        P = synth.orthonormal(44, d) if workload in ("opq_encode", "opq_reconstruct") else None
        pq = self.ra.Pq(P, q, ctx=self.ctx)
        if args.variant:
            pq.set_encode_variant(args.variant)
        g = torch.Generator(device=self.dev).manual_seed(42 + self.rank)
        extra, cpu_rec, q0 = {}, None, None
        kernel = None
        if workload in ("reconstruct", "opq_reconstruct"):
            src = torch.randint(0, k, (rows, m), device=self.dev, dtype=torch.uint8, generator=g)
            dst = torch.empty((rows, d), device=self.dev, dtype=torch.float32)
            step = lambda: pq.reconstruct_batch_device(src, out=dst, check=False)
        elif workload == "lookup":
            n_codes = args.lookup_codes
            src = torch.randint(0, k, (n_codes, m), device=self.dev, dtype=torch.uint8, generator=g)
            sel = torch.randint(0, n_codes, (rows,), device=self.dev, dtype=torch.int64, generator=g)
            scl = torch.rand((n_codes,), device=self.dev, dtype=torch.float32, generator=g) + 0.5
            dst = torch.empty((rows, d), device=self.dev, dtype=torch.float32)
            if not args.record_bytes:
                step = lambda: pq.reconstruct_rows_device(src, sel, scales=scl, out=dst, check=False)
            else:                                 # interleaved records: codes + scale of a row share one line (A/B: tools/lookup_ab.sh)
                rec, rec_off = self.ra.Pq.interleave_records(src, scl, record_bytes=args.record_bytes)
                step = lambda: pq.reconstruct_records_device(rec, rec_off, sel, out=dst, check=False)
                extra["layout"] = "interleaved %d-byte records (codes at 0, f32 scale at %d)" % (rec.shape[1], rec_off)
        elif workload == "adc_scan":
            src = torch.randint(0, k, (rows, m), device=self.dev, dtype=torch.uint8 if k <= 256 else torch.int32, generator=g)
            nq = max(1, args.queries)
            query = torch.from_numpy(synth.normalish(45, (d,) if nq == 1 else (nq, d))).to(self.dev)
            dst = torch.empty((rows,) if nq == 1 else (nq, rows), device=self.dev, dtype=torch.float32)
            lut = pq.adc_tables_device(query)
            extra["queries_per_scan"] = nq
            step = lambda: pq.adc_scan_device(src, lut, out=dst)
        else:
            src = self.normal_rows(rows, d, 42 + self.rank)
            dst = torch.empty((rows, m), device=self.dev, dtype=torch.uint8 if k <= 256 else torch.int32)
            step = lambda: pq.quantize_batch_device(src, out=dst)
        if workload in ("opq_train", "kmeans"):
            # initial centroids = K distinct instances per subquantizer (RandomInstanceCentroids, pq.rs:166-172)
            pick = torch.arange(k, device=self.dev) * (rows // k)
            q0 = np.stack([src[(pick + 7 * mm) % rows, mm * dsub:(mm + 1) * dsub].cpu().numpy() for mm in range(m)])
        if workload == "opq_train":
            from reductive_amd.pq import opq_train_step
            P0 = synth.orthonormal(44, d)
            state = {"q": q0}
            self.ctx.set_option("cross_product_exact", 0 if args.fast_cross else 1)
            extra["cross_product"] = "float tolerance (split-K)" if args.fast_cross else "exact (rule 2: 256-row blocks added in row order)"

            def step():
                state["q"], state["cross"] = opq_train_step(state["q"], P0, src, ctx=self.ctx)
        if workload == "kmeans":
            # one step = one kmeans_iteration (assign + update) of all M subquantizers over the resident
            # instances; the K timed steps are ONE library call with n_iterations = K, exactly how
            # pq.rs:176 drives it (centroids carried from step to step)
            from reductive_amd.pq import kmeans_iterations
            state = {}

            def run_steps(n_it):
                if n_it > 0:
                    state["q"] = kmeans_iterations(q0, src, n_iterations=n_it, want_loss=False, ctx=self.ctx)[0]
            run_steps(warmup)
            torch.cuda.synchronize()
            self.barrier()
            torch.cuda.synchronize()
            self.ra.launch_log(reset=True)
            t0 = time.perf_counter()
            run_steps(steps)
            torch.cuda.synchronize()
            self.barrier()
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            kernel_ms = kmin = kmax = 1e3 * elapsed / steps
        else:
            elapsed, kernel_ms, kmin, kmax = self.timed(step, steps, warmup)
        # what the timed steps actually launched (the library's launch log of this thread: distinct kernel names with
        # counts over the K timed steps) -- never a string table
        kernel = per_step(self.ra.launch_log(reset=True), steps)
        extra["kernels_launched_per_step"] = kernel
        if workload in ("encode", "encode_d768", "opq_encode", "opq_train"):
            extra["encode_kernel"] = pq.last_encode_kernel()
        outputs = {}                              # taken before the CPU baseline and the store-ceiling fill below overwrite dst
        if dump and workload in ("opq_train", "kmeans"):
            outputs = {"quantizers": dump_sample(state["q"], dump // 2)}
            if workload == "opq_train":
                outputs["cross"] = dump_sample(state["cross"], dump // 2)
        elif dump:
            outputs = {OUTPUT_NAMES[workload]: dump_sample(dst, dump, axis=dst.dim() - 1 if workload == "adc_scan" else 0)}

        sec = kernel_ms * 1e-3
        suffix = ""
        if workload == "adc_scan" and args.queries > 1:
            suffix = "_q%d" % args.queries
        if workload == "lookup" and args.lookup_codes != 10_000_000:
            suffix = "_codes%d" % args.lookup_codes
        if workload == "opq_train" and args.fast_cross:
            suffix = "_fastcross"
        traffic_rec, why = load_pmc_traffic(workload, rows, d, m, k, suffix)
        traffic = traffic_rec["hbm_bytes_per_launch"] if traffic_rec else None
        if workload in ("reconstruct", "lookup", "adc_scan"):
            if workload == "lookup":
                bytes_vec = 4 * d + m + 8 + 4     # output row + code row + row index + scale
            if workload == "adc_scan":
                bytes_vec = m * (1 if k <= 256 else 4) + 4 * max(1, args.queries)   # code row in, one f32 distance out per query
            ach = bytes_vec * rows / sec / 1e9
            roof = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS,
                    "traffic": traffic, "kernel": kernel, "avg_launch_ms": kernel_ms, "min_launch_ms": kmin,
                    "max_launch_ms": kmax, "worst_launch_frac": bytes_vec * rows / (kmax * 1e-3) / 1e9 / PEAK_HBM_GBS,
                    "algorithmic_bytes_per_vector": bytes_vec}
        else:
            flop = flop_enc + (2 * d * d if workload == "opq_encode" else 0)
            if workload == "opq_train":           # rotation + 2 assignments + cross product
                flop = 2 * d * d + 2 * flop_enc + 2 * d * d
            if workload == "opq_reconstruct":     # the inverse rotation only (+ 2 d^2 per vector)
                flop = 2 * d * d
            ach = flop * rows / sec / 1e12
            roof = {"bound": "mfma", "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / PEAK_F32_MFMA_TFLOPS, "traffic": traffic,
                    "kernel": kernel,
                    "avg_launch_ms": kernel_ms, "min_launch_ms": kmin, "max_launch_ms": kmax,
                    "algorithmic_flop_per_vector": flop, "algorithmic_bytes_per_vector": bytes_vec,
                    "hbm_gbs": bytes_vec * rows / sec / 1e9, "hbm_frac": bytes_vec * rows / sec / 1e9 / PEAK_HBM_GBS,
                    "mfma_frac": ach / PEAK_F32_MFMA_TFLOPS}
            # The candidate-list kernel evaluates a handful of the K distances per sub-vector and issues no matrix instruction: the
            # flop of the full distance matrix is an equivalent, not work it does.  Its governing roofline is HBM (rows in, codes
            # out); the equivalent stays in the record under its own name.
            if workload == "encode" and isinstance(kernel, str) and "k_encode_vor2" in kernel:
                roof.update({"bound": "hbm", "achieved": roof["hbm_gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": roof["hbm_frac"],
                             "full_distance_matrix_tflops_equivalent": ach})
            # small codebooks (K = 16: 32 flop per byte): the HBM roofline is the nearer one -- it governs, the matrix fraction stays beside it
            elif workload == "encode" and roof["hbm_frac"] > roof["frac"]:
                roof.update({"bound": "hbm", "achieved": roof["hbm_gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": roof["hbm_frac"],
                             "mfma_tflops": ach})
        if workload != "kmeans":
            roof["launch_ms"] = list(getattr(self, "last_launch_ms", []))[:32]     # every timed step, in order
        if traffic_rec:
            roof["traffic_kernel"] = traffic_rec.get("kernel")
            roof["traffic_over_algorithmic"] = traffic / float(bytes_vec * rows)
        else:
            roof["traffic_note"] = why

        checks = args.full and not args.no_cpu_baseline
        if cpu and self.world == 1 and checks:
            if workload in ("encode", "opq_encode", "encode_d768"):
                cpu_rec = cpu_baseline(args, q, P, src, dst, pq, full=(workload == "encode"))
            elif workload == "reconstruct":
                cpu_rec = cpu_baseline_reconstruct(q, src, dst)
            elif workload == "opq_reconstruct":
                cpu_rec = cpu_baseline_reconstruct(q, src, dst, P)
            elif workload == "kmeans":
                cpu_rec = cpu_baseline_kmeans(args, q0, src, self.ctx)
            elif workload == "adc_scan":
                cpu_rec = cpu_baseline_adc(q, query, src, dst, lut)
        if workload in ("reconstruct", "lookup") and checks:
            # what plain streaming stores reach on THIS output allocation of THIS box (torch fill_, no reads): the
            # write rate moves 5-9 % with the physical placement of the buffer for every store pattern
            # (tools/store_patterns.hip), so the kernel is also quoted against it.  After the parity
            # check above, which reads the output.
            flat = dst.view(-1)
            parts = [flat[i:i + (1 << 30)] for i in range(0, flat.numel(), 1 << 30)]

            def fill():
                for part in parts:
                    part.fill_(1.0)
            _, _, fmin, _ = self.timed(fill, 3, 1)
            ceil_gbs = flat.numel() * 4 / (fmin * 1e-3) / 1e9
            roof["store_ceiling"] = {"gbs": ceil_gbs, "kernel_over_ceiling": 4 * d * rows / sec / 1e9 / ceil_gbs,
                                     "what": "torch fill_ of the same output buffer, best of 3, measured after the timed region (output bytes only on both sides of the ratio)"}
            del flat, parts
        del src, dst
        pq.close()
        torch.cuda.empty_cache()
        return {"elapsed": elapsed, "rows": rows, "steps": steps, "warmup": warmup, "extra": extra,
                "roofline": roof, "cpu_baseline": cpu_rec, "shape": (d, m, k), "outputs": outputs}


METRIC_NAMES = {"encode": "vectors/sec PQ encode", "encode_d768": "vectors/sec PQ encode",
                "opq_encode": "vectors/sec OPQ rotate+encode", "reconstruct": "vectors/sec PQ reconstruct",
                "opq_reconstruct": "vectors/sec OPQ reconstruct (gather + inverse rotation)",
                "lookup": "vectors/sec select+reconstruct+rescale lookup",
                "adc_scan": "codes/sec asymmetric-distance scan",
                "opq_train": "vectors/sec per OPQ training iteration (device part)",
                "kmeans": "vectors/sec per k-means iteration, all subquantizers"}


def record(workload, r, world, shards=None):
    d, m, k = r["shape"]
    total_rows = world * r["rows"]
    rec = {"metric": "%s (d=%d, M=%d, K=%d)" % (METRIC_NAMES[workload], d, m, k),
           "value": total_rows * r["steps"] / r["elapsed"], "unit": "vectors/s",
           "n_gpus": world, "steps": r["steps"], "warmup": r["warmup"],
           "ms_per_step": 1e3 * r["elapsed"] / r["steps"], "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": WORKLOADS[workload][0].format(rows=r["rows"], d=d, m=m, k=k),
                      "rows_per_gpu": r["rows"], "rows_total": total_rows, "d": d, "M": m, "K": k,
                      "placement": "inputs and outputs resident in HBM; C ABI device entry point"}}
    if shards is not None:
        rec["config"]["shards"] = shards
    rec.update(r["extra"])
    rec["roofline"] = r["roofline"]
    if r["cpu_baseline"] is not None:
        rec["cpu_baseline"] = r["cpu_baseline"]
    return rec


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = not args.dry_run
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=args.backend if use_gpu else "gloo", rank=rank, world_size=world)
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run" % (args.gpus, world))
    label, (d0, m0, k0), rows0 = WORKLOADS[args.workload]
    d, m, k = args.d or d0, args.m or m0, args.k or k0
    rows = args.rows or rows0
    shards = shard_ranges(world, rows)

    def barrier():
        if world > 1:
            dist.barrier()

    if args.in_process:
        if world != 1:
            raise SystemExit("--in-process drives all device slots from ONE process")
        print(json.dumps(in_process(args, d, m, k, rows)), flush=True)
        return

    # with --full the default one-GPU run also times SUB_CONFIGS and REFERENCE_SHAPES after the headline, in the same
    # process; so does --dump-outputs, whose files are what every one of these paths computed.  The dump shares its byte
    # budget equally between the timed paths of the run (or of all ranks)
    default_headline = (args.workload == "encode" and (d, m, k) == (300, 15, 256) and rows == 10_000_000)
    with_subs = (use_gpu and world == 1 and default_headline and not args.no_sub_configs
                 and (args.full or bool(args.dump_outputs)))
    n_paths = 1 + len(SUB_CONFIGS) + len(REFERENCE_SHAPES) if with_subs else world
    dump = DUMP_BYTES // n_paths if args.dump_outputs else 0
    outputs = {}
    if use_gpu:
        if args.single_device:
            local_rank = 0
        b = Bench(args, rank, world, local_rank, barrier)
        main_r = b.run(args.workload, rows, d, m, k, args.steps, args.warmup, dump=dump)
        elapsed = main_r["elapsed"]
        outputs.update((("rank%d." % rank if world > 1 else "") + n, a) for n, a in main_r.pop("outputs").items())
    else:
        main_r = None
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            time.sleep(0.001)
        barrier()
        elapsed = time.perf_counter() - t0

    tmax = torch.tensor([elapsed], dtype=torch.float64,
                        device="cuda" if (use_gpu and world > 1 and args.backend == "nccl") else "cpu")
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax.item())

    if rank == 0:
        if main_r is None:
            main_r = {"elapsed": elapsed, "rows": rows, "steps": args.steps, "warmup": args.warmup, "extra": {},
                      "roofline": None, "cpu_baseline": None, "shape": (d, m, k)}
        main_r["elapsed"] = elapsed               # max over ranks
        rec = record(args.workload, main_r, world, shards)
        if not use_gpu:
            rec.pop("roofline", None)
        # the other single-GPU BASELINE configs, each with its own roofline / cpu_baseline / parity record
        if with_subs:
            subs = {}
            for key, wl, srows in SUB_CONFIGS:
                sd, sm, sk = WORKLOADS[wl][1]
                try:
                    r = b.run(wl, srows, sd, sm, sk, max(1, min(args.steps, args.sub_steps)), min(2, max(1, args.warmup)), dump=dump)
                    subs[key] = record(wl, r, 1)
                    outputs.update((re.sub(r"\W", "", key) + "." + n, a) for n, a in r["outputs"].items())
                except Exception as e:            # a sub-config must never take the headline line down
                    subs[key] = {"error": "%s: %s" % (type(e).__name__, e)}
            rec["configs"] = subs
            refs = {}
            for key, (sd, sm, sk) in REFERENCE_SHAPES:
                try:
                    r = b.run("encode", 10_000_000, sd, sm, sk, max(1, min(args.steps, args.sub_steps)), min(2, max(1, args.warmup)), dump=dump)
                    refs[key] = record("encode", r, 1)
                    outputs.update((key + "." + n, a) for n, a in r["outputs"].items())
                except Exception as e:
                    refs[key] = {"error": "%s: %s" % (type(e).__name__, e)}
            rec["reference_shapes"] = refs
        if use_gpu:
            rec["summary"] = summarize(rec)       # LAST key: the tail of the line always shows every BASELINE config
        print(json.dumps(rec), flush=True)
    if args.dump_outputs:
        write_outputs(args.dump_outputs, outputs)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def summarize(rec):
    """Compact per-config digest (<= 800 characters), emitted as the last key of the JSON line: value, roofline
    fraction, measured-over-algorithmic HBM traffic and the parity flag of the headline and of every sub-config."""
    def parity(r):
        cb = r.get("cpu_baseline") or {}
        flags = [v for k_, v in cb.items() if k_.startswith("gpu_") and isinstance(v, bool)]
        return all(flags) if flags else None

    def one(r):
        if "error" in r:
            return {"error": r["error"][:60]}
        roof = r.get("roofline") or {}
        tr = roof.get("traffic_over_algorithmic")
        return {"v": float("%.4g" % r["value"]), "frac": round(roof.get("frac", 0.0), 3), "bound": roof.get("bound"),
                "traffic_ratio": None if tr is None else round(tr, 2), "parity": parity(r)}
    out = {"configs[1]": one(rec)}
    for key, sub in (rec.get("configs") or {}).items():
        out[key.replace("_one_gpu_shard", "")] = one(sub)
    for key, sub in (rec.get("reference_shapes") or {}).items():
        o = one(sub)
        if "error" not in o:                      # small-codebook shapes: the HBM fraction is the one that says something
            o["hbm_frac"] = round((sub.get("roofline") or {}).get("hbm_frac", 0.0), 3)
            o.pop("traffic_ratio", None)
        out[key.split("_d")[0]] = o
    return out


def in_process(args, d, m, k, rows):
    """north_star's multi-GPU form, measured through the LIBRARY's sharder: one process, one host batch,
    pqhip_ctx_create(devices) + pqhip_quantize_batch_f32 (contiguous row shards, one host thread per
    device, codebook replicated, no collective, codes land in one host array).  PCIe-inclusive by
    construction, so this is reported beside -- never as -- the HBM-resident `value` of the default run."""
    import numpy as np
    import reductive_amd
    import synth
    from reductive_amd.pq import _Ctx
    n_slots = args.in_process
    devices = [0] * n_slots if args.single_device else list(range(n_slots))
    reductive_amd.lib()
    ctx = _Ctx(devices=devices)
    q = synth.normalish(43, (m, k, d // m))
    pq = reductive_amd.Pq(None, q, ctx=ctx)
    rng = np.random.default_rng(42)
    x = rng.standard_normal((rows, d), dtype=np.float32)
    out = np.empty((rows, m), np.uint8 if k <= 256 else np.uint32)
    # warm-up on the WHOLE batch: the pinned staging buffers of a device slot grow with the shard they serve, and a warm-up on
    # 262,144 rows (rounds 2-3) sized them for 131 k-row shards when two slots shared the batch -- the first timed step then
    # paid four 256 MB hipHostMalloc calls (50-60 ms, varying from box to box): the "two slots are slower than one" of
    # VERDICT r3 weak #14 was this, not the link (gpurun_out/r4e/sweep.jsonl: a constant +41..59 ms per call at 2 M, 8 M and
    # 16 M rows; tools/mb_h2d_concurrent.py: 56.5 GB/s aggregate for 1, 2 and 4 concurrent H2D streams)
    for _ in range(max(1, args.warmup)):
        pq.quantize_batch_into(x, out)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pq.quantize_batch_into(x, out)
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        write_outputs(args.dump_outputs, {"codes": dump_sample(out, DUMP_BYTES)})
    per = (rows + n_slots - 1) // n_slots
    rec = {"metric": "vectors/sec PQ encode, host-resident batch through the library's device sharder (d=%d, M=%d, K=%d)" % (d, m, k),
           "value": rows * args.steps / elapsed, "unit": "vectors/s", "n_gpus": n_slots, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "pqhip_quantize_batch_f32 over ONE host batch of %d x %d, rows sharded contiguously over %d device slot(s) %s, codes concatenated host-side (PCIe-inclusive)"
                                  % (rows, d, n_slots, devices), "rows_total": rows, "d": d, "M": m, "K": k,
                      "shards": [[i * per, min(rows, (i + 1) * per)] for i in range(n_slots)],
                      "placement": "inputs and outputs in pageable host memory"},
           "host_gbs": rows * (4 * d + m) * args.steps / elapsed / 1e9}
    if args.full and not args.no_cpu_baseline:
        from oracle import pq_oracle as orc
        n_s = min(rows, 200_000)
        tail = slice(rows - n_s, rows)
        rec["codes_identical_to_oracle_head_and_tail"] = bool(
            (orc.quantize_batch(q, x[:n_s], n_threads=host_cores()) == out[:n_s]).all()
            and (orc.quantize_batch(q, x[tail], n_threads=host_cores()) == out[tail]).all())
    return rec


def cpu_baseline(args, q, P, src, dst, pq, full=True):
    """The oracle (a C port of the reference's path, CANON-F32) timed on this box's host cores on
    a bounded sample of the SAME workload, plus a parity check of the GPU codes on that sample.
    The oracle is used here only as the thing timed/checked -- never as the product."""
    from oracle import pq_oracle as orc
    import numpy as np
    cores = host_cores()                          # the CPU quota of this job = the threads the oracle is given
    d = src.shape[1]
    scale = max(1, (d * (2 if P is not None else 1)) // 300)      # keep the sample's CPU work bounded for wide / OPQ shapes
    n_mt = min(args.cpu_rows // scale, src.shape[0])
    n_st = min(max(n_mt // 8, 1), 250_000 // scale)
    x = src[:n_mt].cpu().numpy()
    t = time.perf_counter()
    c_mt = orc.quantize_batch(q, x, projection=P, n_threads=cores, dtype=np.uint8 if dst.dtype.itemsize == 1 else np.uint32)
    t_mt = time.perf_counter() - t
    t = time.perf_counter()
    orc.quantize_batch(q, x[:n_st], projection=P, n_threads=1)
    t_st = time.perf_counter() - t
    same = bool((dst[:n_mt].cpu().numpy().astype(np.int64) == c_mt.astype(np.int64)).all())
    # the sample's tail of the batch as well (last rows of the launch: ragged row groups, clamped tiles)
    n_tail = min(200_000 // scale, src.shape[0])
    xt = src[-n_tail:].cpu().numpy()
    same_tail = bool((dst[-n_tail:].cpu().numpy().astype(np.int64) ==
                      orc.quantize_batch(q, xt, projection=P, n_threads=cores, dtype=np.uint32).astype(np.int64)).all())
    rec = {"value": n_mt / t_mt, "unit": "vectors/s", "cores": cores, "logical_cpus": os.cpu_count(), "kind": "port",
           "sample": "first %d rows of the bench batch, oracle sharded over %d threads (%.1f s); "
                     "single-thread: %d rows; parity also on the last %d rows" % (n_mt, cores, t_mt, n_st, n_tail),
           "single_thread_value": n_st / t_st, "simd": "avx2+fma" if orc.lib().pqo_uses_fma_simd() else "scalar",
           "gpu_codes_identical_on_sample": same and same_tail}
    if not full:
        return rec
    # PCIe-inclusive rate of the host-buffer entry point on the same sample (never `value`)
    n_h = min(n_mt, 2_000_000)
    pq.quantize_batch(x[:n_h])                    # first call sizes the pinned staging buffers (kept by the context)
    t = time.perf_counter()
    c_h = pq.quantize_batch(x[:n_h])
    t_h = time.perf_counter() - t
    # the same path written as BLAS sgemm + argmin (numpy / OpenBLAS, all cores) -- a
    # stand-in for a reference linked against an optimised BLAS; not bit-comparable (its own rounding order)
    blas = None
    if P is None:
        try:
            n_b = min(n_mt, 200_000)
            xb = x[:n_b]
            cc = (q.astype(np.float32) ** 2).sum(-1)
            t = time.perf_counter()
            codes_b = np.empty((n_b, q.shape[0]), np.uint8)
            for m_ in range(q.shape[0]):
                xs = xb[:, m_ * q.shape[2]:(m_ + 1) * q.shape[2]]
                dist = (xs * xs).sum(1, keepdims=True) + cc[m_][None, :] - 2.0 * (xs @ q[m_].T)
                codes_b[:, m_] = dist.argmin(1)
            blas = {"value": n_b / (time.perf_counter() - t), "rows": n_b,
                    "agreement_with_canon": float((codes_b == c_mt[:n_b]).mean())}
        except Exception:
            blas = None
    rec.update({"blas_formulation": blas, "host_resident_api_value": n_h / t_h,
                "host_resident_api_gbs": n_h * (4 * d + q.shape[0]) / t_h / 1e9,
                "host_resident_api_identical": bool((c_h == c_mt[:n_h]).all())})
    return rec


def cpu_baseline_reconstruct(q, src, dst, P=None):
    """BASELINE.md B-rec: the oracle's gather (primitives.rs:110-173 semantics, single thread as in the
    reference) on head, middle and TAIL row ranges of the launch -- for the 100 M-code config the tail
    rows sit beyond element offset 2^32 of the output and beyond the Infinity Cache's reach of the code
    matrix -- and the GPU rows checked against it byte for byte.  With a projection (pq.rs:323-326) the
    oracle also un-rotates, and the comparison is SURVEY.md 8c rule 6: 1e-5 of the largest magnitude."""
    import numpy as np
    from oracle import pq_oracle as orc
    rows = src.shape[0]
    n_s = min(250_000 if P is None else 50_000, rows)
    starts = sorted({0, max(0, rows // 2 - n_s // 2), max(0, rows - n_s)})
    t_cpu, ok, n_tot, worst = 0.0, True, 0, 0.0
    for s0 in starts:
        c_host = src[s0:s0 + n_s].cpu().numpy()
        t = time.perf_counter()
        want = orc.reconstruct_batch(q, c_host) if P is None else orc.reconstruct_batch(q, c_host, projection=P)
        t_cpu += time.perf_counter() - t
        n_tot += c_host.shape[0]
        got = dst[s0:s0 + n_s].cpu().numpy()
        if P is None:
            ok = ok and bool(got.tobytes() == want.tobytes())
        else:
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            worst = max(worst, rel)
            ok = ok and rel <= 1e-5
    rec = {"value": n_tot / t_cpu, "unit": "vectors/s", "cores": 1, "kind": "port",
           "sample": "%d code rows at row offsets %s of the bench batch (head, middle, tail; last output element offset %d), "
                     "oracle %s on one thread (%.1f s)" % (n_s, starts, rows * q.shape[0] * q.shape[2] - 1,
                                                           "gather" if P is None else "gather + inverse rotation", t_cpu)}
    if P is None:
        rec["gpu_rows_identical_on_sample"] = ok
    else:
        rec["gpu_rows_within_1e-5_on_sample"] = ok
        rec["max_rel_error"] = worst
    return rec


def cpu_baseline_kmeans(args, q0, src, ctx):
    """One kmeans_iteration of the oracle (assignment sharded over the host cores, update and loss
    sequential as in the reference) on a bounded sample, and the GPU result on the same sample
    checked bit for bit (centroids and losses)."""
    from oracle import pq_oracle as orc
    from reductive_amd.pq import kmeans_iterations
    cores = host_cores()
    n_s = min(args.cpu_rows // 2, src.shape[0])
    x = src[:n_s].cpu().numpy()
    t = time.perf_counter()
    want_q, want_loss = orc.kmeans_iterations(q0, x, n_iterations=1, n_threads=cores)
    t_cpu = time.perf_counter() - t
    got_q, got_loss = kmeans_iterations(q0, src[:n_s], n_iterations=1, want_loss=True, ctx=ctx)
    return {"value": n_s / t_cpu, "unit": "vectors/s", "cores": cores, "logical_cpus": os.cpu_count(), "kind": "port",
            "sample": "one iteration over the first %d rows of the bench batch; oracle assignment on %d "
                      "threads, update + loss sequential (%.1f s)" % (n_s, cores, t_cpu),
            "gpu_centroids_identical_on_sample": bool(got_q.tobytes() == want_q.tobytes()),
            "gpu_loss_identical_on_sample": bool(got_loss.tobytes() == want_loss.tobytes())}


def cpu_baseline_adc(q, query, src, dst, lut):
    """The oracle's table build + scan (declared f32 order: tables by CANON-F32 rules 1-3, row sums
    sequentially over m) on head and tail samples of the code matrix; GPU distances checked bit for bit."""
    from oracle import pq_oracle as orc
    import numpy as np
    rows = src.shape[0]
    nq = 1 if query.dim() == 1 else query.shape[0]
    n_s = min(2_000_000 // nq, rows)
    qh = query.cpu().numpy()
    want_lut = orc.adc_tables(q, qh)
    ok = bool(lut.cpu().numpy().tobytes() == want_lut.tobytes())
    t_cpu, n_tot = 0.0, 0
    for s0 in sorted({0, rows - n_s}):
        c_host = src[s0:s0 + n_s].cpu().numpy()
        t = time.perf_counter()
        want = orc.adc_scan(want_lut, c_host)
        t_cpu += time.perf_counter() - t
        n_tot += c_host.shape[0]
        ok = ok and bool(np.ascontiguousarray(dst[..., s0:s0 + n_s].cpu().numpy()).tobytes() == want.tobytes())
    return {"value": n_tot / t_cpu, "unit": "vectors/s", "cores": 1, "kind": "port",
            "sample": "%d code rows x %d queries (head and tail of the resident matrix), oracle scan on one thread (%.1f s)" % (n_tot, nq, t_cpu),
            "gpu_distances_identical_on_sample": ok}


if __name__ == "__main__":
    main()
