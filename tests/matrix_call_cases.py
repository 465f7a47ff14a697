"""What the three resident matrices of reductive_amd/qmatrix.py ask of `Pq`: the case list and a recorder.

Each case calls one public method of a QuantizedMatrix, PartitionedMatrix or ResidualPartitionedMatrix over small
synthetic inputs (tests/synth.py; no training outside the build cases).  A recorder wraps every attribute of `Pq` whose
name ends in `_device` -- and, for the build cases, reductive_amd.pq.kmeans_iterations, cluster_assignments and train_pq
-- forwards each call and notes what qmatrix.py itself asked for (calls a wrapper makes of another wrapper are pq.py's
own business and are left out): the method without its `_device`, after the number of subquantizers of the Pq it was
called on (M1 = the coarse quantizer), and every argument that is not at its default, by parameter name: scalars as they
are, a tensor as dtype, shape, strides (left out for a contiguous tensor) and a digest of its bytes, an `out=` tensor without the digest (its bytes are uninitialised), a numpy
Generator as a digest of its state.  Per case the record holds the calls, launch_log(reset=True), the returned tensors
-- for a returned matrix every tensor it stores -- and the type and text of a raised exception.

tests/golden/matrix_call_trace.json was written by this module's main from the commit BEFORE the searches of the three
classes were moved onto one driver per search kind (`written_from` in the file names it), and is never rewritten from
later code: tests/test_gpu_matrix_call_trace.py replays the cases against it.  A record does not depend on the cases
run before it: the fixture runs every case once unrecorded, so that what a Pq prepares on its first use is done, and a
range flag left up by an unchecked call is taken down before each case.  main runs every case twice and refuses a case
whose two records differ; the build cases (partition*, which train on the GPU) agreed as well, so their records hold
the digests of the built matrices like every other case.
usage (on a GPU): python tests/matrix_call_cases.py OUT.json COMMIT [DIRECTORY HOLDING THE reductive_amd OF THAT COMMIT]"""
import hashlib
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "matrix_call_trace.json")

M, K, DSUB = 5, 16, 4            # odd M: packed rows of 3 bytes
D = M * DSUB
N, N_LISTS = 37, 4
LIST_SIZES = [10, 0, 15, 12]     # LIST_OFF[37] of device_call_cases: list 1 is empty
NQ = 3
BIG_N, BIG_LISTS = 1100, 1030    # more than 1,024 lists: the all-lists route of the probe selection
KINDS = ("flat", "lists", "residual")
STORED = ("ids", "list_off", "positions", "codes", "norms", "row_terms", "lists", "vectors")
BUILD_FUNCTIONS = ("kmeans_iterations", "cluster_assignments", "train_pq")


DTYPES = {"float32": "f32", "float16": "f16", "float64": "f64", "int64": "i64", "int32": "i32", "uint8": "u8", "bool": "b"}


def _digest(b):
    return hashlib.sha256(b).hexdigest()[:6]


def _shape(a):
    return ",".join(str(int(n)) for n in a)


def _tensor(t, digest=True):
    """dtype[shape], then /strides where they are not those of a contiguous tensor, then #digest of the bytes"""
    name = str(t.dtype).replace("torch.", "")
    s = "%s[%s]" % (DTYPES.get(name, name), _shape(t.shape))
    if not t.is_contiguous() or t.stride() != t.contiguous().stride():
        s += "/" + _shape(t.stride())
    return s + "#" + _digest(t.detach().cpu().contiguous().reshape(-1).numpy().tobytes()) if digest else s


def _value(v, digest=True):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return "np.%s[%s]#%s" % (v.dtype, _shape(v.shape), _digest(np.ascontiguousarray(v).tobytes()))
    if hasattr(v, "untyped_storage"):
        return _tensor(v, digest)
    if isinstance(v, np.random.Generator):
        return "rng#" + _digest(repr(v.bit_generator.state).encode())
    if isinstance(v, (tuple, list)):
        return [_value(e, digest) for e in v]
    if isinstance(v, slice):
        return "slice(%s, %s, %s)" % (v.start, v.stop, v.step)
    return type(v).__name__


def _result(out):
    """what a case returned: tensors as _tensor gives them, a matrix by every tensor it stores, a RowFilter by its words"""
    if isinstance(out, (tuple, list)):
        return [_result(e) for e in out]
    if hasattr(out, "words") and hasattr(out, "n_allowed"):
        return {"RowFilter": _tensor(out.words), "n_allowed": out.n_allowed}
    if hasattr(out, "codes") and hasattr(out, "pq"):
        rec = {"type": type(out).__name__, "packed4": out.packed4, "device_terms": getattr(out, "device_terms", None),
               "pq": _value(np.asarray(out.pq.subquantizers()))}
        if hasattr(out, "centroids"):
            rec["centroids"] = _value(out.centroids)
        for name in STORED:
            if getattr(out, name, None) is not None:
                rec[name] = _tensor(getattr(out, name))
        return rec
    return _value(out)


class Recorder:
    """Puts recording wrappers in the place of the Pq device methods (and of the build functions of reductive_amd.pq)
    through `setattr_(object, name, value)`; leave() puts the originals back."""

    def __init__(self, ra, setattr_):
        self.calls, self.depth, self.saved, self.setattr = [], 0, [], setattr_
        for name in sorted(vars(ra.Pq)):
            if name.endswith("_device") and callable(getattr(ra.Pq, name)):
                self._wrap(ra.Pq, name, True)
        for name in BUILD_FUNCTIONS:
            self._wrap(ra.pq, name, False)

    def _wrap(self, owner, name, method):
        fn = getattr(owner, name)
        sig = inspect.signature(fn)

        def call(*args, **kw):
            if self.depth == 0:
                bound = sig.bind(*args, **kw)
                rec = {p: _value(v, digest=p != "out") for p, v in bound.arguments.items()
                       if p not in ("self", "ctx") and v is not sig.parameters[p].default}
                who = "M%d." % args[0].quantized_len() if method else ""
                self.calls.append([who + name.replace("_device", ""), rec])
            self.depth += 1
            try:
                return fn(*args, **kw)
            finally:
                self.depth -= 1
        self.saved.append((owner, name, fn))
        self.setattr(owner, name, call)

    def leave(self):
        for owner, name, fn in self.saved:
            self.setattr(owner, name, fn)


# ---- inputs: platform-independent bits (synth.py), small shapes; everything a case reads is made here, once ------------
def _assignment(seed, sizes):
    """list ids with the given list sizes, in a fixed shuffled order"""
    import synth
    ids = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    return np.ascontiguousarray(ids[np.argsort(synth._hash(seed, ids.size), kind="stable")])


class Env:
    def __init__(self, ra):
        import synth
        import torch
        from reductive_amd import qmatrix
        self.ra, self.torch = ra, torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.dev = dev
        self.pq = ra.Pq(None, synth.normalish(7100, (M, K, DSUB)))
        self.rpq = ra.Pq(None, synth.normalish(7103, (M, K, DSUB)) * np.float32(0.5))      # the quantizer of the residuals
        self.x = synth.normalish(7101, (N, D))
        self.norms = synth.uniform01(7106, (N,)) + np.float32(0.5)
        self.centroids = synth.normalish(7105, (N_LISTS, D))
        self.assign = _assignment(7104, LIST_SIZES)
        self.queries = dev(synth.normalish(7107, (NQ, D)))
        self.xb, self.nb = synth.normalish(7110, (6, D)), synth.uniform01(7111, (6,)) + np.float32(0.5)
        self.assign_b = _assignment(7112, [2, 1, 0, 3])
        self.flags = synth.codes_u8(7113, (N,), 3) > 0
        self.m, self.filters, self.piece = {}, {}, {}

        def three(n_rows, norms, centroids, assign, seed):
            codes = synth.codes_u8(seed, (n_rows, M), K)
            flat = qmatrix.QuantizedMatrix(self.pq, codes, norms)
            lists = qmatrix.PartitionedMatrix(flat, centroids, assign)
            residual = qmatrix.ResidualPartitionedMatrix(self.rpq, dev(synth.codes_u8(seed + 1, (n_rows, M), K)),
                                                         None if norms is None else dev(norms),
                                                         dev(synth.normalish(seed + 2, (n_rows,))), centroids, assign)
            return {"flat": flat, "lists": lists, "residual": residual}

        for with_norms in (True, False):
            ms = three(N, self.norms if with_norms else None, self.centroids, self.assign, 7120)
            for kind, m in ms.items():
                m.attach_vectors(self.x, torch.float32 if with_norms else torch.float16)
                for packed in (False, True):
                    mm = m.pack4() if packed else m
                    self.m[kind, with_norms, packed] = mm
                    self.filters[kind, with_norms, packed] = mm.row_filter(self.flags)
            for kind, p in three(6, self.nb if with_norms else None, self.centroids, self.assign_b, 7130).items():
                self.piece[kind, with_norms] = p                                           # what extend() is given
        self.bare = qmatrix.QuantizedMatrix(self.pq, synth.codes_u8(7120, (N, M), K))      # no vectors attached
        self.other_lists = qmatrix.PartitionedMatrix(self.piece["flat", True], self.centroids * np.float32(2.0), self.assign_b)
        dt = qmatrix.ResidualPartitionedMatrix(self.rpq, dev(synth.codes_u8(7121, (N, M), K)), dev(self.norms),
                                               dev(synth.normalish(7122, (N,))), self.centroids, dev(self.assign))
        dt.device_terms = True              # as partition_residual(on_device=True) leaves it
        self.device_terms = dt.attach_vectors(self.x)
        self.big = three(BIG_N, synth.uniform01(7140, (BIG_N,)) + np.float32(0.5), synth.normalish(7141, (BIG_LISTS, D)),
                         _assignment(7142, [2] * (BIG_N - BIG_LISTS) + [1] * (2 * BIG_LISTS - BIG_N)), 7143)
        self.ropq = ra.Pq(np.ascontiguousarray(np.eye(D, dtype=np.float32)[::-1]), synth.normalish(7150, (M, K, DSUB)))
        self.one_row = dev(np.zeros((1, M), np.uint8))
        for run in CASES.values():      # once unrecorded: what a Pq prepares on its first use stays out of the records
            try:
                run(self)
            except Exception:
                pass
        torch.cuda.synchronize()

    def settle(self):
        """A range flag that an unchecked call of an earlier case left up (a row number out of range) would be raised by
        this case's first checked call: a checked call per quantizer takes it down, so that a record does not depend
        on the cases before it."""
        for p in (self.pq, self.rpq, self.ropq):
            try:
                p.reconstruct_batch_device(self.one_row)
            except self.ra.PanicError:
                pass

    def q(self, multi):
        return self.queries if multi else self.queries[0]

    def allow(self, form, key):
        return {"none": None, "bool": self.flags, "filter": self.filters[key]}[form]


def _cases():
    cases = {}

    def add(name, run):
        assert name not in cases, name
        cases[name] = run

    rng = np.random.RandomState(20251)
    pick = lambda *options: options[rng.randint(len(options))]
    probe = lambda kind, nprobe: {} if kind == "flat" else {"nprobe": nprobe}
    drawn = lambda: dict(with_norms=pick(True, False), multi=pick(True, False), nprobe=pick(1, 2, 4))

    # ---- nearest / most_similar: use_norms x refine x allow x packed; norms, queries, k and nprobe drawn per case -----------
    def topk(method, kind, with_norms, packed, multi, k, nprobe, refine, allow, use_norms=None):
        def run(E):
            key = (kind, with_norms, packed)
            kw = dict(probe(kind, nprobe), refine=refine, allow=E.allow(allow, key))
            if use_norms is not None:
                kw["use_norms"] = use_norms
            return getattr(E.m[key], method)(E.q(multi), k, **kw)
        return run

    for kind in KINDS:
        for method, use_norms in (("nearest", None), ("most_similar", True), ("most_similar", False)):
            for refine in (None, 8):
                for allow in ("none", "bool", "filter"):
                    for packed in (False, True):
                        add("%s-%s-%s-r%s-%s-p%d" % (kind, method, {None: "l2", True: "scaled", False: "plain"}[use_norms], refine or 0, allow, packed),
                            topk(method, kind, packed=packed, refine=refine, allow=allow, use_norms=use_norms,
                                 k=pick(1, 5) if refine else pick(1, 5, 40), **drawn()))
        fixed = dict(with_norms=True, packed=False, multi=True, k=5, nprobe=2, refine=None, allow="none")
        add(kind + "-nearest-refine-below-k", topk("nearest", kind, **dict(fixed, k=40, refine=8)))
        if kind != "flat":
            add(kind + "-most_similar-refine-then-nprobe", topk("most_similar", kind, **dict(fixed, nprobe=0, refine=2)))
    add("flat-nearest-refine-without-vectors", lambda E: E.bare.nearest(E.q(True), 5, refine=8))

    # ---- within / similar_above: threshold form x sort x allow; a packed matrix refuses ------------------------------------
    def in_range(method, kind, with_norms, packed, multi, per_query, sort, allow, nprobe, use_norms=None):
        def run(E):
            key = (kind, with_norms, packed)
            values = ([30.0, 45.0, 1e9] if method == "within" else [-1.0, 0.5, -1e9])[:NQ if multi else 1]
            thr = np.array(values, np.float32) if per_query else values[-1 if multi else 0]
            kw = dict(probe(kind, nprobe), sort=sort, allow=E.allow(allow, key))
            if use_norms is not None:
                kw["use_norms"] = use_norms
            return getattr(E.m[key], method)(E.q(multi), thr, **kw)
        return run

    for kind in KINDS:
        for method in ("within", "similar_above"):
            for per_query in (False, True):
                for sort in (False, True):
                    for allow in ("none", pick("bool", "filter")):
                        add("%s-%s-perquery%d-sort%d-%s" % (kind, method, per_query, sort, allow),
                            in_range(method, kind, packed=False, per_query=per_query, sort=sort, allow=allow,
                                     use_norms=None if method == "within" else pick(True, False), **drawn()))
            add("%s-%s-packed-then-filter" % (kind, method), lambda E, kind=kind, method=method: getattr(E.m[kind, True, True], method)(
                E.q(True), 1.0, allow=E.filters[kind, True, False], **probe(kind, 0)))

    # ---- nearest_among / most_similar_among ---------------------------------------------------------------------------------
    SHARED = np.array([3, -1, 36, 0, 99, 17, 17, 5], np.int64)           # a -1 and a number out of range
    LIMS = np.array([0, 3, 3, 8], np.int64)

    def among(method, kind, with_norms=True, packed=False, multi=True, pair=False, k=5, refine=None, check=False, rows=None):
        def run(E):
            r = rows
            if r is None:
                r = (LIMS if multi else LIMS[[0, -1]], E.dev(SHARED)) if pair else SHARED
            kw = {} if method == "nearest_among" else {"use_norms": with_norms}
            return getattr(E.m[kind, with_norms, packed], method)(E.q(multi), r, k, refine=refine, check=check, **kw)
        return run

    for kind in KINDS:
        for method in ("nearest_among", "most_similar_among"):
            for pair in (False, True):
                for refine in (None, 8):
                    add("%s-%s-pair%d-refine%s" % (kind, method, pair, refine),
                        among(method, kind, with_norms=pick(True, False), multi=pick(True, False), pair=pair, k=pick(1, 5), refine=refine))
            add("%s-%s-packed-then-refine" % (kind, method), among(method, kind, packed=True, k=40, refine=8))
        add(kind + "-nearest_among-check", among("nearest_among", kind, check=True))
        add(kind + "-nearest_among-k40", among("nearest_among", kind, k=40))
        add(kind + "-most_similar_among-refine-then-rows", among("most_similar_among", kind, k=40, refine=8, rows=np.zeros(3, np.float32)))
        add(kind + "-most_similar_among-rows-triple", among("most_similar_among", kind, rows=(LIMS, SHARED, SHARED)))

    # ---- row filters, embeddings, packing, growth -----------------------------------------------------------------------------
    for kind in KINDS:
        m = lambda E, kind=kind: E.m[kind, True, False]
        p = lambda E, kind=kind: E.m[kind, False, True]
        add("row_filter-allow-" + kind, lambda E, m=m: m(E).row_filter(E.flags))
        add("row_filter-rows-" + kind, lambda E, p=p: p(E).row_filter(rows=[5, 36, 5, 0]))
        add("row_filter-excluded-" + kind, lambda E, m=m: m(E).row_filter(rows=E.dev(np.array([5, 36], np.int64)), allowed=False))
        add("row_filter-out-of-range-" + kind, lambda E, m=m: m(E).row_filter(rows=[0, N]))
        add("row_filter-of-another-matrix-" + kind, lambda E, kind=kind: E.m[kind, True, False].nearest(
            E.q(True), 5, allow=E.filters[kind, True, True], **probe(kind, 2)))
        add("embeddings-" + kind, lambda E, m=m: m(E).embeddings([36, 0, 7, 7]))
        add("embeddings-packed-" + kind, lambda E, p=p: p(E).embeddings(np.array([1, 35])))
        add("pack4-" + kind, lambda E, m=m: m(E).pack4())
        add("unpack4-" + kind, lambda E, p=p: p(E).unpack4())
        add("attach_vectors-f16-" + kind, lambda E, m=m: m(E).pack4().attach_vectors(E.dev(E.x), E.torch.float16))
        add("add-" + kind, lambda E, m=m: m(E).add(E.xb, norms=E.nb))
        add("add-packed-" + kind, lambda E, p=p: p(E).add(E.dev(E.xb)))
        add("add-none-" + kind, lambda E, m=m: m(E).add(E.xb[:0], norms=E.nb[:0]))
        add("add-missing-norms-" + kind, lambda E, m=m: m(E).add(E.xb))
    for kind in KINDS[1:]:
        add("extend-" + kind, lambda E, kind=kind: E.m[kind, True, False].extend(E.piece[kind, True]))
        add("extend-packed-" + kind, lambda E, kind=kind: E.m[kind, False, True].extend(E.piece[kind, False].pack4()))
        add("extend-packed-mismatch-" + kind, lambda E, kind=kind: E.m[kind, True, True].extend(E.piece[kind, True]))
        add("extend-norms-mismatch-" + kind, lambda E, kind=kind: E.m[kind, True, False].extend(E.piece[kind, False]))
        add("assign-" + kind, lambda E, kind=kind: E.m[kind, True, False].assign(E.xb))
    add("extend-another-class", lambda E: E.m["lists", True, False].extend(E.piece["residual", True]))
    add("extend-other-centroids", lambda E: E.m["lists", True, False].extend(E.other_lists))
    add("extend-terms-route", lambda E: E.device_terms.extend(E.piece["residual", True]))
    add("encode-torch-terms", lambda E: E.m["residual", True, False].encode(E.xb))
    add("encode-device-terms", lambda E: E.device_terms.encode(E.dev(E.xb)))
    add("encode-device-terms-none", lambda E: E.device_terms.encode(E.xb[:0]))
    add("add-device-terms-packed", lambda E: E.device_terms.pack4().add(E.xb, norms=E.nb))

    # ---- probe selection, and the route beyond 1,024 probes -----------------------------------------------------------------
    for kind in KINDS[1:]:
        for nprobe in (1, 2, 4, 0):
            add("probes-%s-%d" % (kind, nprobe), lambda E, kind=kind, nprobe=nprobe: E.m[kind, True, False].probes(E.q(nprobe != 2), nprobe))
        big = lambda E, kind=kind: E.big[kind]
        add("big-%s-probes" % kind, lambda E, big=big: big(E).probes(E.q(True), BIG_LISTS))
        add("big-%s-nearest" % kind, lambda E, big=big: big(E).nearest(E.q(True), 5, BIG_LISTS))
        add("big-%s-most_similar-one-query" % kind, lambda E, big=big: big(E).most_similar(E.q(False), 40, 5000, use_norms=False))
        add("big-%s-within" % kind, lambda E, big=big: big(E).within(E.q(False), 30.0, BIG_LISTS, sort=True))
        add("big-%s-similar_above" % kind, lambda E, big=big: big(E).similar_above(E.q(True), 0.5, BIG_LISTS))
        add("big-%s-nearest-1025" % kind, lambda E, big=big: big(E).nearest(E.q(True), 5, 1025))
        add("big-%s-similar_above-1025" % kind, lambda E, big=big: big(E).similar_above(E.q(True), 0.5, 1025))

    # ---- the build steps: partition / partition_residual ----------------------------------------------------------------------
    def build(method, with_norms=True, vectors=False, seed=1, given_pq=None, **kw):
        def run(E):
            more = dict(kw, rng=np.random.default_rng(seed), n_iterations=2)
            if vectors:
                more["vectors"] = E.dev(E.x) if vectors == "device" else E.x
            if method == "partition_residual":
                more["pq_iterations"] = 2
                if given_pq:
                    more["residual_pq"] = getattr(E, given_pq)
            return getattr(E.m["flat", with_norms, False], method)(N_LISTS, **more)
        return run

    for method in ("partition", "partition_residual"):
        for on_device in (False, True):
            add("%s-device%d" % (method, on_device), build(method, on_device=on_device))
            add("%s-device%d-train-rows" % (method, on_device),
                build(method, with_norms=False, vectors="device" if on_device else "host", train_rows=20, seed=3, on_device=on_device))
        add(method + "-packed", lambda E, method=method: getattr(E.m["flat", True, True], method)(N_LISTS))
        add(method + "-too-many-lists", build(method, train_rows=3))
    for on_device in (False, True):
        add("partition_residual-device%d-given-pq" % on_device, build("partition_residual", given_pq="rpq", seed=4, on_device=on_device))
    add("partition_residual-device1-given-opq", build("partition_residual", given_pq="ropq", vectors="host", seed=5, on_device=True))
    return cases


CASES = _cases()


def run_case(E, run, setattr_):
    """One case -> its record.  `setattr_(object, name, value)` puts the wrappers in (monkeypatch.setattr in the test)."""
    torch = E.torch
    E.settle()
    torch.cuda.synchronize()
    E.ra.launch_log(reset=True)
    rec = Recorder(E.ra, setattr_)
    out, error = None, None
    try:
        out = run(E)
    except Exception as e:      # the record is what the method raised
        error = [type(e).__name__, str(e)]
    finally:
        rec.leave()
    torch.cuda.synchronize()
    log = E.ra.launch_log(reset=True)
    return json.loads(json.dumps({"calls": rec.calls, "log": log, "error": error, "returns": _result(out)}))


def main(out_path, commit, package_dir=None):
    sys.path.insert(0, os.path.abspath(package_dir or os.path.dirname(HERE)))
    sys.path.insert(0, HERE)
    import reductive_amd
    E = Env(reductive_amd)
    with open(out_path, "w") as f:
        f.write('{"written_from": %s,\n "cases": {\n' % json.dumps(commit))
        unstable = []
        for i, (name, run) in enumerate(CASES.items()):
            record = run_case(E, run, setattr)
            if record != run_case(E, run, setattr):
                unstable.append(name)
            f.write('%s  %s: %s' % (",\n" if i else "", json.dumps(name), json.dumps(record, separators=(",", ":"))))
        f.write("\n }}\n")
    print("%d cases -> %s" % (len(CASES), out_path))
    assert not unstable, "two runs differ: %s" % unstable


if __name__ == "__main__":
    main(*sys.argv[1:4])
