"""What the `*_device` wrappers of reductive_amd/pq.py hand to the C library: the case list and a recording proxy.

Each case calls one wrapper with small tensors.  A Recorder stands in the place of the loaded library
(reductive_amd._lib.lib), forwards every call and notes the symbol and its arguments: integers as they are, pointers as
None, "cb", "stream", [input name, byte offset into its storage] or "fresh" (an address the wrapper made itself: an
output, a contiguous copy, a stand-in).  Per case the record holds the calls, shape / dtype / strides and a digest of
every returned tensor, and the type and text of a raised exception.

tests/golden/device_call_trace.json was written by this module's main from the commit BEFORE the wrappers were moved
onto reductive_amd/_marshal.py, and is never rewritten from later code: tests/test_gpu_device_call_trace.py replays the
cases against it.
usage (on a GPU): python tests/device_call_cases.py OUT.json COMMIT [DIRECTORY HOLDING THE reductive_amd OF THAT COMMIT]"""
import ctypes
import hashlib
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "device_call_trace.json")

QUANTIZERS = {"A": (5, 16, 4),       # odd M: packed rows of 3 bytes; packed4 and every u8 path
              "B": (2, 300, 2)}      # K > 256: int32 codes
N_LISTS = 4
LIST_OFF = {0: [0, 0, 0, 0, 0], 1: [0, 1, 1, 1, 1], 37: [0, 10, 10, 25, 37]}        # list 1 is empty
NQ = 3


class Recorder:
    """In the place of the loaded library: forwards every call and records it."""

    def __init__(self, real):
        self._real = real
        self.calls = []
        self.inputs = {}        # name -> (storage address, bytes)
        self.cb = None
        self.stream = 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("pqhip_"):
            return fn

        def call(*args):
            self.calls.append([name] + [self._classify(a, t) for a, t in zip(args, fn.argtypes or ())])
            return fn(*args)
        return call

    def _classify(self, a, argtype):
        if argtype is not ctypes.c_void_p:
            return int(a) if isinstance(a, (int, np.integer)) else repr(a)
        if isinstance(a, ctypes.c_void_p):
            if a.value == self.cb:
                return "cb"
            return "stream" if (a.value or 0) == self.stream else "another stream"
        if not a:
            return None
        for name, (base, size) in self.inputs.items():
            if base <= a < base + size:
                return [name, a - base]
        return "fresh"


# ---- inputs: platform-independent bits (synth.py), small shapes ---------------------------------------------------------
class Env:
    def __init__(self, ra):
        import synth
        import torch
        self.ra, self.torch, self.synth = ra, torch, synth
        self.pq = {q: ra.Pq(None, synth.normalish(7000 + i, (M, K, d))) for i, (q, (M, K, d)) in enumerate(QUANTIZERS.items())}
        M, K, d = QUANTIZERS["A"]
        self.pq["P"] = ra.Pq(np.eye(M * d, dtype=np.float32), synth.normalish(7000, (M, K, d)))     # with a projection
        for p in self.pq.values():
            p._cb()
        self.side_stream = torch.cuda.Stream()

    def dev(self, a):
        a = np.ascontiguousarray(a)
        if a.size == 0:         # numpy gives an empty array strides of 0; keep the strides of its shape
            return self.torch.empty(a.shape, dtype=self.torch.from_numpy(a).dtype, device="cuda")
        return self.torch.from_numpy(a).cuda()

    def laid_out(self, a, layout):
        """a 2-D array on the device: contiguous, as the first columns of a wider matrix, or column-major"""
        if layout == "contig":
            return self.dev(a)
        if layout == "rows":
            wide = np.zeros((a.shape[0], a.shape[1] + 3), a.dtype)
            wide[:, :a.shape[1]] = a
            return self.dev(wide)[:, :a.shape[1]]
        assert layout == "cols"
        return self.dev(a.T).t()

    def f32(self, seed, shape):
        return self.synth.normalish(seed, shape)

    def ints(self, seed, shape, k, dtype):
        h = self.synth._hash(seed, int(np.prod(shape)))
        return ((h >> np.uint64(33)) % np.uint64(k)).astype(dtype).reshape(shape)

    def codes(self, q, n, layout="contig", packed4=False, seed=100):
        M, K, _ = QUANTIZERS[q]
        c = self.ints(seed + n, (n, M), K, np.uint8 if K <= 256 else np.int32)
        if packed4:     # a quantizer that 4-bit rows do not serve is refused before they are read
            c = self.ra.pack_codes4(c, K).reshape(n, (M + 1) // 2) if K <= 16 else np.zeros((n, (M + 1) // 2), np.uint8)
        return self.laid_out(c, layout)

    def tables(self, q, multi, seed=200):
        M, K, _ = QUANTIZERS[q]
        return self.dev(self.f32(seed, (NQ, M, K) if multi else (M, K)))

    def mask(self, n, seed=300):
        bits = self.ints(seed + n, (n,), 3, np.uint8) > 0
        words = np.zeros((n + 31) // 32, np.uint32)
        for p in np.nonzero(bits)[0]:
            words[p >> 5] |= np.uint32(1) << np.uint32(p & 31)
        return self.dev(words.view(np.int32))

    def probes(self, multi, layout):
        p = np.array([[0, 2], [3, -1], [1, 0]] if multi else [[2, -1]], np.int64)
        t = self.laid_out(p, layout)
        return t if multi else t[0]

    def bias(self, multi, layout):
        t = self.laid_out(self.f32(400, (NQ if multi else 1, 2)), layout)
        return t if multi else t[0]

    def threshold(self, form, multi):
        if form == "float":
            return 0.5
        if form in ("numpy-scalar", "tensor-scalar"):
            return np.float32(0.5) if form == "numpy-scalar" else self.torch.tensor(0.5)
        per_query = np.array([0.5, -1.0, 2.0] if multi else [0.5], np.float32)
        return per_query if form == "numpy" else self.dev(per_query)


def search_call(fn, q="A", n=37, layout="contig", multi=True, allow=False, scales=False, packed4=False, k=5, check=False,
                stream=False, probes="contig", bias="contig", capacity="default", thr="float", edit=None):
    """A case of one of the 12 search and range wrappers: the arguments the wrapper's signature names, from the options."""
    def make(E):
        pq = E.pq[q]
        names = inspect.signature(getattr(pq, fn)).parameters
        kw = {"codes": E.codes(q, n, layout, packed4), "check": check}
        kw["ip_tables" if "ip_tables" in names else "tables"] = E.tables(q, multi)
        if "list_off" in names:
            kw["list_off"] = E.dev(np.array(LIST_OFF[n], np.int64))
            kw["probes"] = E.probes(multi, probes)
        if "probe_bias" in names:
            kw["probe_bias"] = E.bias(multi, bias)
        if "row_terms" in names:
            kw["row_terms"] = E.dev(E.f32(500 + n, (n,)))
        if "scales" in names and scales:
            kw["scales"] = E.dev(E.f32(600 + n, (n,)))
        if allow:
            kw["allow"] = E.mask(n)
        if packed4:
            kw["packed4"] = True
        if "k" in names:
            kw["k"] = k
        else:
            kw["threshold"] = E.threshold(thr, multi)
            if capacity != "default":
                kw["capacity"] = capacity
        if stream:
            kw["stream"] = E.side_stream.cuda_stream
        if edit:
            edit(E, kw)
        return pq, fn, kw
    return make


def call(fn, make_kw, q="A"):
    return lambda E: (E.pq[q], fn, make_kw(E))


SEARCHES = ["adc_search_device", "adc_ip_search_device", "adc_search_lists_device", "adc_ip_search_lists_device",
            "adc_search_lists_residual_device", "adc_ip_search_lists_residual_device"]
RANGES = [s.replace("search", "range") for s in SEARCHES]
LAYOUTS = ["contig", "rows", "cols"]


def _cases():
    cases = {}

    def add(name, make):
        assert name not in cases, name
        cases[name] = make

    # ---- the 12 search and range wrappers: rows x code layouts, the other options drawn per case ----------------------
    rng = np.random.RandomState(20250)
    pick = lambda *options: options[rng.randint(len(options))]
    for fn in SEARCHES + RANGES:
        for n in (0, 1, 37):
            for layout in LAYOUTS:
                o = dict(n=n, layout=layout, multi=pick(False, True), allow=pick(False, True), scales=pick(False, True),
                         check=pick(False, True), stream=pick(False, True), probes=pick(*LAYOUTS), bias=pick(*LAYOUTS))
                if fn in SEARCHES:
                    o.update(packed4=pick(False, True), k=pick(1, 5))
                else:
                    o.update(capacity=pick("default", 0, 1), thr=pick("float", "numpy", "tensor"))
                add("%s-n%d-%s" % (fn, n, layout), search_call(fn, **o))
        # each option once more against a fixed background, so that none depends on the draw
        for key, value in (("multi", False), ("allow", True), ("scales", True), ("check", True), ("stream", True),
                           ("probes", "rows"), ("probes", "cols"), ("bias", "rows"), ("bias", "cols")):
            add("%s-%s-%s" % (fn, key, value), search_call(fn, **{key: value}))
        if fn in SEARCHES:
            add(fn + "-k1", search_call(fn, k=1))
            for allow in (False, True):
                add("%s-packed4-allow%d" % (fn, allow), search_call(fn, packed4=True, allow=allow, layout="rows"))
        else:
            for capacity in (0, 1):
                add("%s-capacity%d" % (fn, capacity), search_call(fn, capacity=capacity))
            add(fn + "-capacity1-stream", search_call(fn, capacity=1, stream=True, allow=True))
            for thr in ("numpy", "tensor", "numpy-scalar", "tensor-scalar"):
                for multi in (False, True):
                    add("%s-thr-%s-multi%d" % (fn, thr, multi), search_call(fn, thr=thr, multi=multi))
    # quantizer B (int32 codes) in every wrapper that takes them.  The library serves them in the two plain exhaustive
    # searches only: with a mask, and in the range searches, the call is made and refused, which is recorded as well.
    for fn in SEARCHES[:2] + RANGES:
        for n, layout in ((0, "contig"), (1, "contig"), (37, "contig"), (37, "rows"), (37, "cols")):
            add("%s-B-n%d-%s" % (fn, n, layout),
                search_call(fn, q="B", n=n, layout=layout, allow=layout == "cols", check=n == 1, scales=layout == "rows"))

    # ---- the other wrappers, once per distinct argument shape ----------------------------------------------------------
    def x_rows(E, q, n, layout="contig", seed=800):
        M, _, d = QUANTIZERS[q]
        return E.laid_out(E.f32(seed + n, (n, M * d)), layout)

    def empty(E, shape, dtype):
        return E.dev(np.zeros(shape, dtype))

    for q in "AB":
        M, K, d = QUANTIZERS[q]
        for n in (0, 1, 37):
            for layout in LAYOUTS:
                add("quantize-%s-n%d-%s" % (q, n, layout), call("quantize_batch_device", lambda E, q=q, n=n, layout=layout:
                    {"x": x_rows(E, q, n, layout)}, q))
                add("reconstruct-%s-n%d-%s" % (q, n, layout), call("reconstruct_batch_device", lambda E, q=q, n=n, layout=layout:
                    {"codes": E.codes(q, n, layout)}, q))
                add("scan-%s-n%d-%s" % (q, n, layout), call("adc_scan_device", lambda E, q=q, n=n, layout=layout:
                    {"codes": E.codes(q, n, layout), "tables": E.tables(q, layout != "rows"), "check": n == 1}, q))
        for dtype in ("int16", "int32", "int64"):
            add("quantize-%s-out-%s" % (q, dtype), call("quantize_batch_device", lambda E, q=q, M=M, dtype=dtype:
                {"x": x_rows(E, q, 37), "out": empty(E, (37, M + 2), dtype)[:, :M], "stream": E.side_stream.cuda_stream}, q))
            add("reconstruct-%s-%s" % (q, dtype), call("reconstruct_batch_device", lambda E, q=q, M=M, K=K, d=d, dtype=dtype:
                {"codes": E.dev(E.ints(810, (37, M), K, dtype)), "out": empty(E, (37, M * d + 1), "float32")[:, :M * d],
                 "check": False}, q))
        add("scan-%s-out" % q, call("adc_scan_device", lambda E, q=q:
            {"codes": E.codes(q, 37), "tables": E.tables(q, True), "out": empty(E, (NQ, 37), "float32"),
             "stream": E.side_stream.cuda_stream}, q))
        add("scan-%s-out-one-row" % q, call("adc_scan_device", lambda E, q=q:
            {"codes": E.codes(q, 1, "rows"), "tables": E.tables(q, False), "out": empty(E, (1,), "float32")}, q))
        for ip in ("", "ip_"):
            add("%stables-%s-one" % (ip, q), call("adc_%stables_device" % ip, lambda E, q=q: {"queries": x_rows(E, q, 1)[0]}, q))
            for layout in LAYOUTS:
                add("%stables-%s-%s" % (ip, q, layout), call("adc_%stables_device" % ip, lambda E, q=q, layout=layout:
                    {"queries": x_rows(E, q, NQ, layout), "stream": E.side_stream.cuda_stream if layout == "rows" else None}, q))

    def rows_of(E, n, r=4):
        return E.dev(E.ints(820, (r,), max(n, 1), np.int64))

    for n in (1, 37):
        for layout in LAYOUTS:
            add("reconstruct-rows-n%d-%s" % (n, layout), call("reconstruct_rows_device", lambda E, n=n, layout=layout:
                {"codes": E.codes("A", n, layout), "rows": rows_of(E, n), "scales": E.dev(E.f32(830, (n,))) if n == 37 else None,
                 "check": layout == "contig"}))
    add("reconstruct-rows-none", call("reconstruct_rows_device", lambda E:
        {"codes": E.codes("A", 37), "rows": rows_of(E, 37, 0), "check": False}))
    add("reconstruct-rows-one-out", call("reconstruct_rows_device", lambda E:
        {"codes": E.codes("A", 37), "rows": rows_of(E, 37, 1), "out": empty(E, (1, 23), "float32")[:, :20],
         "stream": E.side_stream.cuda_stream}))

    def records(E, n):
        rec, off = E.pq["A"].interleave_records(E.codes("A", n), E.dev(E.f32(830, (n,))))
        return {"records": rec, "scale_offset": off}
    for r in (0, 1, 4):
        add("reconstruct-records-r%d" % r, call("reconstruct_records_device", lambda E, r=r:
            dict(records(E, 37), rows=rows_of(E, 37, r), check=r == 4)))
    add("reconstruct-records-out", call("reconstruct_records_device", lambda E:
        dict(records(E, 37), rows=rows_of(E, 37, 1), out=empty(E, (1, 23), "float32")[:, :20], check=False,
             stream=E.side_stream.cuda_stream)))

    for n in (0, 1, 37):
        for layout in LAYOUTS:
            add("pack4-n%d-%s" % (n, layout), call("pack_codes4_device", lambda E, n=n, layout=layout:
                {"codes": E.codes("A", n, layout), "check": n == 37}))
            add("unpack4-n%d-%s" % (n, layout), call("unpack_codes4_device", lambda E, n=n, layout=layout:
                {"packed": E.codes("A", n, layout, True), "check": n == 37}))
    add("pack4-int32", call("pack_codes4_device", lambda E: {"codes": E.codes("A", 37).to(E.torch.int32)}))
    add("pack4-out-one-row", call("pack_codes4_device", lambda E:
        {"codes": E.codes("A", 1), "out": empty(E, (1, 6), "uint8")[:, :3], "stream": E.side_stream.cuda_stream}))
    add("unpack4-rows", call("unpack_codes4_device", lambda E:
        {"packed": E.codes("A", 37, "rows", True), "rows": rows_of(E, 37), "check": True}))
    add("unpack4-rows-out", call("unpack_codes4_device", lambda E:
        {"packed": E.codes("A", 37, packed4=True), "rows": rows_of(E, 37, 1), "out": empty(E, (1, 8), "uint8")[:, :5],
         "stream": E.side_stream.cuda_stream}))
    add("unpack4-empty-with-rows", call("unpack_codes4_device", lambda E:
        {"packed": E.codes("A", 0, packed4=True), "rows": rows_of(E, 0, 2), "check": True}))      # every row id is out of range

    def allowed(E, n, kind):
        a = E.dev(E.ints(840, (n,), 2, np.uint8))
        return a.bool() if kind == "bool" else a
    for n in (0, 1, 37):
        for kind in ("bool", "uint8"):
            add("row-mask-n%d-%s" % (n, kind), call("pack_row_mask_device", lambda E, n=n, kind=kind:
                {"allow": allowed(E, n, kind), "check": n == 37}))
    add("row-mask-perm", call("pack_row_mask_device", lambda E:
        {"allow": allowed(E, 37, "bool"), "perm": rows_of(E, 37, 40), "check": True, "stream": E.side_stream.cuda_stream}))
    add("row-mask-perm-strided", call("pack_row_mask_device", lambda E:
        {"allow": allowed(E, 74, "uint8")[::2], "perm": rows_of(E, 37, 80)[::2]}))
    add("row-mask-perm-none", call("pack_row_mask_device", lambda E:
        {"allow": allowed(E, 37, "bool"), "perm": rows_of(E, 37, 0)}))
    add("row-mask-n-src-0", call("pack_row_mask_device", lambda E:
        {"allow": allowed(E, 0, "bool"), "perm": rows_of(E, 0, 3), "check": True}))                # every entry is out of range

    def rerank(E, N, half=False, one=False, layout="contig", **more):
        v = E.laid_out(E.f32(850, (N, 6)), layout)
        q = E.laid_out(E.f32(851, (NQ, 6)), layout)
        c = E.laid_out(E.ints(852, (NQ, 7), max(N, 1), np.int64) - (N == 0), layout)
        kw = {"queries": q[0] if one else q, "vectors": v.half() if half else v, "candidates": c[0] if one else c, "k": 3}
        kw.update(more)
        return kw
    for N in (0, 1, 37):
        for half in (False, True):
            add("rerank-N%d-f%d" % (N, 16 if half else 32), call("rerank_device", lambda E, N=N, half=half:
                rerank(E, N, half, check=N == 37, ip=half)))
    for layout in LAYOUTS[1:]:
        add("rerank-" + layout, call("rerank_device", lambda E, layout=layout: rerank(E, 37, layout=layout)))
    add("rerank-one-query", call("rerank_device", lambda E: rerank(E, 37, one=True, stream=E.side_stream.cuda_stream)))
    add("rerank-one-query-rows", call("rerank_device", lambda E: rerank(E, 1, one=True, layout="rows", ip=True)))

    def merge(E, n_a, n_b, cols=3, dtype=np.uint8, **more):
        off = lambda n: E.dev(np.array(LIST_OFF[n], np.int64))
        shape = lambda n: (n, cols) if cols else (n,)
        kw = {"list_off_a": off(n_a), "a": E.dev(E.ints(860, shape(n_a), 200, dtype)),
              "list_off_b": off(n_b), "b": E.dev(E.ints(861, shape(n_b), 200, dtype))}
        kw.update(more)
        return kw
    for n_a, n_b in ((0, 0), (0, 37), (37, 0), (37, 1), (1, 37)):
        add("merge-%d-%d" % (n_a, n_b), call("merge_lists_device", lambda E, n_a=n_a, n_b=n_b:
            merge(E, n_a, n_b, check=n_a == 37)))
    add("merge-vectors-out", call("merge_lists_device", lambda E:
        merge(E, 37, 1, cols=0, dtype=np.int64, out=empty(E, (38,), "int64"), stream=E.side_stream.cuda_stream)))

    def assign(E, n, dtype=np.int64):
        return E.dev(E.ints(870 + n, (n,), N_LISTS, dtype))
    for n in (0, 1, 37):
        for want in (False, True):
            add("layout-n%d-lists%d" % (n, want), call("lists_layout_device", lambda E, n=n, want=want:
                {"assign": assign(E, n, np.int32 if want else np.int64), "n_lists": N_LISTS, "want_lists": want,
                 "check": n == 37, "stream": E.side_stream.cuda_stream if n == 1 else None}))

    cent = lambda E: E.dev(E.f32(880, (N_LISTS, 20)))
    for n in (0, 1, 37):
        for layout in LAYOUTS[:2]:
            add("residuals-n%d-%s" % (n, layout), call("residuals_device", lambda E, n=n, layout=layout:
                {"x": x_rows(E, "A", n, layout), "assign": assign(E, n), "centroids": cent(E), "check": n == 37}))
            add("residual-terms-n%d-%s" % (n, layout), call("residual_terms_device", lambda E, n=n, layout=layout:
                {"codes": E.codes("A", n, layout), "assign": assign(E, n), "centroids": cent(E), "check": n == 37}))
    add("residuals-out", call("residuals_device", lambda E:
        {"x": x_rows(E, "A", 1), "assign": assign(E, 1), "centroids": cent(E), "out": empty(E, (1, 25), "float32")[:, :20],
         "stream": E.side_stream.cuda_stream}))
    add("residual-terms-out", call("residual_terms_device", lambda E:
        {"codes": E.codes("A", 37), "assign": assign(E, 37), "centroids": cent(E), "out": empty(E, (37,), "float32"),
         "stream": E.side_stream.cuda_stream}))

    # ---- every PanicError text of the wrappers; where two arguments are wrong, the first check of the parent speaks ----
    def put(key, make):
        def edit(E, kw):
            kw[key] = make(E, kw)
        return edit

    def both(*edits):
        def edit(E, kw):
            for e in edits:
                e(E, kw)
        return edit
    narrow_codes = put("codes", lambda E, kw: kw["codes"][:, :4])
    def bad_tables(E, kw):
        key = "ip_tables" if "ip_tables" in kw else "tables"
        kw[key] = kw[key][..., :15].contiguous()
    bad_scales = put("scales", lambda E, kw: E.dev(E.f32(1, (36,))))
    bad_mask = put("allow", lambda E, kw: E.mask(70))
    bad_probes = put("probes", lambda E, kw: kw["probes"][:2])
    bad_bias = put("probe_bias", lambda E, kw: kw["probe_bias"][:, :1])
    bad_terms = put("row_terms", lambda E, kw: kw["row_terms"][:36])
    bad_thr = put("threshold", lambda E, kw: np.zeros(2, np.float32))
    for fn in ("adc_search_device", "adc_ip_search_device", "adc_range_device", "adc_ip_range_device"):
        add("error-%s-codes-then-tables" % fn, search_call(fn, edit=both(narrow_codes, bad_tables)))
        add("error-%s-tables-then-mask" % fn, search_call(fn, edit=both(bad_tables, bad_mask)))
        add("error-%s-mask" % fn, search_call(fn, edit=bad_mask))
    add("error-search-tables-then-scales", search_call("adc_ip_search_device", edit=both(bad_tables, bad_scales)))
    add("error-search-scales-then-mask", search_call("adc_ip_search_device", edit=both(bad_scales, bad_mask)))
    add("error-search-packed4-width", search_call("adc_search_device", packed4=True, edit=put("codes", lambda E, kw: kw["codes"][:, :2])))
    add("error-search-packed4-K", search_call("adc_search_device", q="B", packed4=True))
    add("error-search-packed4-K-then-tables", search_call("adc_ip_search_device", q="B", packed4=True, edit=bad_tables))
    for fn in ("adc_search_lists_residual_device", "adc_ip_search_lists_residual_device"):
        add("error-%s-tables-then-probes" % fn, search_call(fn, edit=both(bad_tables, bad_probes)))
        add("error-%s-probes-then-bias" % fn, search_call(fn, edit=both(bad_probes, bad_bias)))
        add("error-%s-bias-then-mask" % fn, search_call(fn, edit=both(bad_bias, bad_mask)))
        add("error-%s-no-bias" % fn, search_call(fn, edit=put("probe_bias", lambda E, kw: None)))
    add("error-search-lists-probes-then-scales", search_call("adc_ip_search_lists_device", edit=both(bad_probes, bad_scales)))
    add("error-search-lists-scales-then-bias", search_call("adc_ip_search_lists_residual_device", edit=both(bad_scales, bad_bias)))
    add("error-search-lists-bias-then-terms", search_call("adc_search_lists_residual_device", edit=both(bad_bias, bad_terms)))
    add("error-search-lists-terms-then-mask", search_call("adc_search_lists_residual_device", edit=both(bad_terms, bad_mask)))
    add("error-search-lists-no-terms", search_call("adc_search_lists_residual_device", edit=put("row_terms", lambda E, kw: None)))
    add("error-search-lists-no-offsets", search_call("adc_search_lists_device", edit=put("list_off", lambda E, kw: kw["list_off"][:0])))
    for fn in ("adc_range_lists_residual_device", "adc_ip_range_lists_residual_device"):
        add("error-%s-tables-then-threshold" % fn, search_call(fn, edit=both(bad_tables, bad_thr)))
        add("error-%s-threshold-then-others" % fn,
            search_call(fn, edit=both(bad_thr, bad_scales, bad_mask) if "ip_" in fn else both(bad_thr, bad_mask)))
        add("error-%s-mask-then-probes" % fn, search_call(fn, edit=both(bad_mask, bad_probes)))
        add("error-%s-probes-then-bias" % fn, search_call(fn, edit=both(bad_probes, bad_bias)))
        add("error-%s-bias-then-capacity" % fn, search_call(fn, capacity=-1, edit=bad_bias))
        add("error-%s-capacity" % fn, search_call(fn, capacity=-1))
        add("error-%s-no-bias" % fn, search_call(fn, edit=put("probe_bias", lambda E, kw: None)))
    add("error-range-scales-then-mask", search_call("adc_ip_range_device", edit=both(bad_scales, bad_mask)))
    add("error-range-terms-then-capacity", search_call("adc_range_lists_residual_device", capacity=-1, edit=bad_terms))
    add("error-range-no-terms", search_call("adc_range_lists_residual_device", edit=put("row_terms", lambda E, kw: None)))

    add("error-quantize-width", call("quantize_batch_device", lambda E: {"x": x_rows(E, "A", 2)[:, :19]}))
    add("error-quantize-out-shape", call("quantize_batch_device", lambda E: {"x": x_rows(E, "A", 2), "out": empty(E, (2, 4), "uint8")}))
    add("error-quantize-index-width", call("quantize_batch_device", lambda E: {"x": x_rows(E, "B", 2), "out": empty(E, (2, 2), "uint8")}, "B"))
    add("error-reconstruct-width", call("reconstruct_batch_device", lambda E: {"codes": E.codes("A", 2)[:, :4]}))
    add("error-reconstruct-out-shape", call("reconstruct_batch_device", lambda E: {"codes": E.codes("A", 2), "out": empty(E, (2, 19), "float32")}))
    add("error-reconstruct-range", call("reconstruct_batch_device", lambda E: {"codes": E.codes("A", 2) + 200, "check": True}))
    add("error-reconstruct-rows-width", call("reconstruct_rows_device", lambda E: {"codes": E.codes("A", 2)[:, :4], "rows": rows_of(E, 2)}))
    add("error-reconstruct-rows-scales", call("reconstruct_rows_device", lambda E:
        {"codes": E.codes("A", 2), "rows": rows_of(E, 2), "scales": E.dev(E.f32(1, (3,))), "out": empty(E, (1, 1), "float32")}))
    add("error-reconstruct-rows-out-shape", call("reconstruct_rows_device", lambda E:
        {"codes": E.codes("A", 2), "rows": rows_of(E, 2), "out": empty(E, (3, 20), "float32")}))
    add("error-reconstruct-records-out-shape", call("reconstruct_records_device", lambda E:
        dict(records(E, 2), rows=rows_of(E, 2), out=empty(E, (3, 20), "float32"))))
    add("error-tables-width", call("adc_tables_device", lambda E: {"queries": x_rows(E, "A", 2)[:, :19]}))
    add("error-ip-tables-width", call("adc_ip_tables_device", lambda E: {"queries": x_rows(E, "A", 1)[0, :19]}))
    add("error-scan-width-then-tables", call("adc_scan_device", lambda E: {"codes": E.codes("A", 2)[:, :4], "tables": E.tables("B", False)}))
    add("error-scan-tables", call("adc_scan_device", lambda E: {"codes": E.codes("A", 2), "tables": E.tables("B", True)}))
    add("error-pack4-K", call("pack_codes4_device", lambda E: {"codes": E.codes("B", 2)}, "B"))
    add("error-pack4-width", call("pack_codes4_device", lambda E: {"codes": E.codes("A", 2)[:, :4]}))
    add("error-unpack4-K", call("unpack_codes4_device", lambda E: {"packed": E.codes("A", 2, packed4=True)}, "B"))
    add("error-unpack4-width", call("unpack_codes4_device", lambda E: {"packed": E.codes("A", 2)}))

    host = lambda E, t: t.cpu()
    for name, kw in (("not-a-tensor", {"vectors": lambda E, t: [1.0]}), ("queries", {"queries": lambda E, t: t.double()}),
                     ("vectors", {"vectors": lambda E, t: t.double()}), ("candidates", {"candidates": lambda E, t: t.int()}),
                     ("widths", {"vectors": lambda E, t: t[:, :5]}), ("candidate-rows", {"candidates": lambda E, t: t[:2]}),
                     ("no-candidates", {"candidates": lambda E, t: t[:, :0]}), ("k", {"k": lambda E, t: 0}),
                     ("host", {"queries": host})):
        add("error-rerank-" + name, call("rerank_device", lambda E, kw=kw:
            {key: kw[key](E, value) if key in kw else value for key, value in rerank(E, 37).items()}))
    for name, kw in (("not-a-tensor", {"b": lambda E, t: None}), ("dtypes", {"b": lambda E, t: t.int()}),
                     ("shapes", {"b": lambda E, t: t[:, :2]}), ("offsets", {"list_off_b": lambda E, t: t[:4]}),
                     ("row-bytes", {"a": lambda E, t: t[:, :0], "b": lambda E, t: t[:, :0]}),
                     ("no-list", {"list_off_a": lambda E, t: t[:1], "list_off_b": lambda E, t: t[:1]}),
                     ("out", {"out": lambda E, t: t[:37]}), ("strided", {"a": lambda E, t: E.laid_out(t.cpu().numpy(), "rows")}),
                     ("host", {"a": host})):
        add("error-merge-" + name, call("merge_lists_device", lambda E, kw=kw:
            {key: kw[key](E, value) if key in kw else value
             for key, value in merge(E, 37, 1, out=empty(E, (38, 3), "uint8")).items()}))
    for name, kw in (("not-a-tensor", {"assign": lambda E, t: [0]}), ("dtype", {"assign": lambda E, t: t.short()}),
                     ("n-lists", {"n_lists": lambda E, t: 0}), ("strided", {"assign": lambda E, t: t[::2]}), ("host", {"assign": host})):
        add("error-layout-" + name, call("lists_layout_device", lambda E, kw=kw:
            {key: kw[key](E, value) if key in kw else value for key, value in (("assign", assign(E, 37)), ("n_lists", N_LISTS))}))

    def residual_kw(E, what, kw):
        base = {"assign": assign(E, 37), "centroids": cent(E)}
        base.update({"x": x_rows(E, "A", 37), "out": empty(E, (37, 20), "float32")} if what == "residuals" else
                    {"codes": E.codes("A", 37), "out": empty(E, (37,), "float32")})
        return {key: kw[key](E, value) if key in kw else value for key, value in base.items()}
    first = {"residuals": "x", "residual_terms": "codes"}
    for what in ("residuals", "residual_terms"):
        for name, kw in (("not-a-tensor", {first[what]: lambda E, t: None}), ("input", {first[what]: lambda E, t: t.double()}),
                         ("assign-not-a-tensor", {"assign": lambda E, t: None}), ("assign", {"assign": lambda E, t: t[:36]}),
                         ("centroids", {"centroids": lambda E, t: t[:, :19]}), ("lists-strided", {"centroids": lambda E, t: t.t().contiguous().t()}),
                         ("out", {"out": lambda E, t: t[:36]}), ("columns", {first[what]: lambda E, t: t.t().contiguous().t()}),
                         ("host", {first[what]: host})):
            add("error-%s-%s" % (what, name), call(what + "_device", lambda E, what=what, kw=kw: residual_kw(E, what, kw)))
    add("error-residual_terms-projection", call("residual_terms_device", lambda E: residual_kw(E, "residual_terms", {}), "P"))
    add("error-residual_terms-K", call("residual_terms_device", lambda E: residual_kw(E, "residual_terms", {}), "B"))
    return cases


CASES = _cases()


def _describe(t):
    """shape, dtype, strides and a digest of the bytes of a returned tensor"""
    return [list(t.shape), str(t.dtype), list(t.stride()),
            hashlib.sha256(t.cpu().contiguous().reshape(-1).numpy().tobytes()).hexdigest()[:16]]


def run_case(E, make, setattr_):
    """One case -> its record.  `setattr_(module, name, value)` puts the proxy in (monkeypatch.setattr in the test)."""
    torch = E.torch
    pq, fn, kw = make(E)
    rec = Recorder(E.ra._lib.lib())
    rec.cb = pq._cb().value
    rec.stream = kw.get("stream") or 0
    for name, t in kw.items():
        if hasattr(t, "untyped_storage") and t.is_cuda and t.untyped_storage().nbytes():
            rec.inputs[name] = (t.untyped_storage().data_ptr(), t.untyped_storage().nbytes())
    torch.cuda.synchronize()
    setattr_(E.ra._lib, "lib", lambda: rec)
    out, error = None, None
    try:
        out = getattr(pq, fn)(**kw)
    except Exception as e:      # the record is what the wrapper raised
        error = [type(e).__name__, str(e)]
    finally:
        setattr_(E.ra._lib, "lib", lambda: rec._real)
    torch.cuda.synchronize()
    outs = [] if out is None else [out] if hasattr(out, "shape") else list(out)
    return json.loads(json.dumps({"calls": rec.calls, "error": error,
                                  "returns": [None if t is None else _describe(t) for t in outs]}))


def main(out_path, commit, package_dir=None):
    sys.path.insert(0, os.path.abspath(package_dir or os.path.dirname(HERE)))
    sys.path.insert(0, HERE)
    import reductive_amd
    E = Env(reductive_amd)
    with open(out_path, "w") as f:
        f.write('{"written_from": %s,\n "cases": {\n' % json.dumps(commit))
        for i, (name, make) in enumerate(CASES.items()):
            record = run_case(E, make, setattr)
            assert record == run_case(E, make, setattr), "%s: two runs differ" % name
            f.write('%s  %s: %s' % (",\n" if i else "", json.dumps(name), json.dumps(record, separators=(",", ":"))))
        f.write("\n }}\n")
    print("%d cases -> %s" % (len(CASES), out_path))


if __name__ == "__main__":
    main(*sys.argv[1:4])
