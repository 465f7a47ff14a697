"""CPU tests of the matrix-core range screen and the batch searches built on it (pqhip_flat_screen_f32_dev,
Pq.flat_screen_device / flat_range_batch_device / flat_search_batch_device): the references of the compositions against
the exhaustive references, the bound model against exact values, the pure rules, the declarations and the wrappers'
argument checks.  No GPU is needed; the GPU tests are tests/test_gpu_flat_screen.py and tests/test_gpu_flat_batch.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import flat_range_ref as frr
import flat_screen_ref as fsr
import flat_search_ref as fr
import rerank_ref as rr
from test_flat_among import _data, _special, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def _rules():
    from reductive_amd import pq
    return pq


# ---- the compositions' references against the exhaustive references -------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_batch_search_reference_is_the_flat_search_reference_on_the_special_rows(ip, half):
    pq = _rules()
    q, x = _data(11, 300, 70, 5, half)
    x = _special(q, x)
    allow = np.random.default_rng(3).random(300) < 0.8
    for k in (1, 7, 40):
        for a in (None, allow):
            want_v, want_i = fr.ref_flat_search(q, x, k, ip=ip, allow=a)
            got_v, got_i, _ = fsr.ref_flat_search_batch(q, x, k, pq.flat_batch_sample, pq.flat_batch_falls_back, x_exp=10, ip=ip,
                                                        allow=a)
            assert got_i.tolist() == want_i.tolist() and bits(got_v) == bits(want_v), (k, a is None)
    # a sample that is too thin: 3 allowed rows, k = 7 -> the plain call, the same result
    thin = np.zeros(300, bool)
    thin[[5, 17, 140]] = True
    got_v, got_i, plain = fsr.ref_flat_search_batch(q, x, 7, pq.flat_batch_sample, pq.flat_batch_falls_back, x_exp=10, ip=ip,
                                                    allow=thin)
    want_v, want_i = fr.ref_flat_search(q, x, 7, ip=ip, allow=thin)
    assert plain.all() and got_i.tolist() == want_i.tolist() and bits(got_v) == bits(want_v)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_batch_range_reference_is_the_flat_range_reference_on_the_special_rows(ip, half):
    q, x = _data(12, 300, 70, 5, half)
    x = _special(q, x)
    v = frr.all_values(q, x, ip)
    allow = np.random.default_rng(4).random(300) < 0.7
    finite = v[np.isfinite(v)]
    for thr in (float(np.median(finite)), np.inf, -np.inf, np.nan, v[:, 8].copy(), 0.0):
        for a in (None, allow):
            want = frr.ref_flat_range(q, x, thr, ip=ip, allow=a, values=v)
            got = fsr.ref_flat_range_batch(q, x, thr, x_exp=10, ip=ip, allow=a)
            assert got[0].tolist() == want[0].tolist() and got[2].tolist() == want[2].tolist()
            assert bits(got[1]) == bits(want[1])


# ---- the bound model ----------------------------------------------------------------------------------------------------
def _bound_rows(rng, n, d, mag):
    x = (rng.standard_normal((n, d)) * mag).astype(np.float32)
    x[0] = 0
    x[1] = 0
    x[1, d // 2] = mag                                   # one-hot
    x[2] = mag * (1 - 2 * (np.arange(d) & 1))            # cancelling against a constant query
    x[3] = -x[4]
    x[5] = mag * 2.0 ** -16                              # below f16's normal range once scaled
    return x


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("mag_exp", [-20, 0, 20])
@pytest.mark.parametrize("d", [1, 7, 300, 2048])
def test_bound_covers_the_model_and_stays_inside_the_slack(d, mag_exp, flush):
    pq = _rules()
    rng = np.random.default_rng(100 * d + mag_exp + 50)
    mag = 2.0 ** mag_exp
    n = 48
    x = _bound_rows(rng, n, d, mag)
    q = (rng.standard_normal((6, d)) * mag).astype(np.float32)
    q[0] = x[7]                                          # a distance of exactly zero
    q[1] = mag
    q[2] = 0
    q[3] *= 2.0 ** -9                                    # a query far below the rows
    q[4] *= 2.0 ** 9
    x_exp = pq.flat_screen_x_exp(float(np.abs(x).max()))
    assert 2.0 ** 13 <= float(np.abs(x).max()) * 2.0 ** x_exp < 2.0 ** 14
    assert fsr.regular_rows(x, x_exp).all()
    for ip in (False, True):
        v = np.stack([rr.row_values(qv, x, ip=ip) for qv in q]).astype(np.float64)
        vh, arith = fsr.model_values(x, q, x_exp, ip=ip, flush=flush)
        E = fsr.screen_bound(x, q, x_exp, ip=ip)
        worst = np.abs(vh - v) + arith
        assert (worst <= E).all(), (ip, float((worst / E).max()))
        # the cap of the contract: a row passes only within 2 E of the threshold (E for the inner product's half slack)
        cap = fsr.slack(x, q, x_exp) * (0.5 if ip else 1.0) + 2 * fsr.constants()["kFlatScreenAbs"]
        assert (2 * E <= cap).all(), ip


def test_bound_constants_are_those_of_the_derivation():
    c = fsr.constants()
    # DESIGN.md 5c, per unit of xx + qq for L2: operand rounding 2u + u^2 and query elements below f16's normal range
    # 2^-21.5, accumulation 2047 * 2^-23 (1 + u)^2 (the dot product enters twice, S <= (xx + qq) / 2), xx 2049 * 2^-24,
    # the exact value's own rounding 82 * 2^-23, the epilogue 8 * 2^-24
    need = (2 * fsr.U16 + fsr.U16 ** 2 + 2.0 ** -21.5) + 2047 * 2.0 ** -23 * (1 + fsr.U16) ** 2 + 2049 * fsr.U32 \
        + 82 * 2.0 ** -23 + 8 * fsr.U32
    assert abs(need - 1.354e-3) < 1e-6
    assert need * (1 + 2.0 ** -12) <= c["kFlatScreenRel"] <= 2.0 ** -9 * 0.99
    assert c["kFlatScreenAbsX"] == 2.0 ** -13 and c["kFlatScreenAbs"] == 2.0 ** -100
    assert c["kFlatScreenMaxD"] == 2048 and c["kFlatScreenQueryTop"] == 13


# ---- the pure rules -----------------------------------------------------------------------------------------------------
def test_x_exp_rule():
    pq = _rules()
    for m in (1.0, 1.5, 3.99, 2.0 ** -20, 2.0 ** 20, 65504.0, 1e-6, 7e8):
        e = pq.flat_screen_x_exp(m)
        assert 2.0 ** 13 <= m * 2.0 ** e < 2.0 ** 14, m
    assert pq.flat_screen_x_exp(0.0) == 0 and pq.flat_screen_x_exp(float("nan")) == 0
    assert pq.flat_screen_x_exp(float("inf")) == 0
    assert pq.flat_screen_x_exp(1e-30) == pq.FLAT_SCREEN_MAX_EXP and pq.flat_screen_x_exp(1e30) == -pq.FLAT_SCREEN_MAX_EXP
    assert pq.FLAT_SCREEN_MAX_EXP == fsr.constants()["kFlatScreenMaxExp"]
    assert pq.FLAT_SCREEN_MAX_D == fsr.constants()["kFlatScreenMaxD"]


def test_sample_and_fallback_rules():
    pq = _rules()
    for n, k in ((1, 1), (31, 10), (100, 10), (4100, 1024), (4100, 10), (10 ** 7, 10), (10 ** 7, 1024), (2 ** 33, 100)):
        S, t = pq.flat_batch_sample(n, k)
        assert t >= 1 and S == len(range(0, n, t)) and S <= n
        assert S >= min(n, 4 * k)                       # at least 4 k rows when the matrix has them
        want = 2.0 * (n * k) ** 0.5
        assert S <= max(2 * want + 1, 8 * k + 1, 1) or S == n
        assert pq.flat_batch_sample(n, k) == (S, t)     # a pure function
    assert pq.flat_batch_sample(0, 5) == (0, 1)
    assert pq.flat_batch_sample(10 ** 7, 10) == (20000, 500)
    f = pq.FLAT_BATCH_FALLBACK_FRACTION
    assert f == 1.0 / 16
    assert not pq.flat_batch_falls_back(1000, 1000, 16) and pq.flat_batch_falls_back(1001, 1000, 16)
    assert not pq.flat_batch_falls_back(0, 0, 4)
    for n, nq in ((1000, 16), (10 ** 7, 256), (5, 1)):
        cap = pq.flat_batch_capacity(n, nq, 10, 100)
        assert not pq.flat_batch_falls_back(cap - 1, n, nq) or cap - 1 > f * n * nq - 1
        assert pq.flat_batch_falls_back(cap + 1, n, nq)  # whatever exceeds the allocation falls back: no second call


# ---- the declarations -----------------------------------------------------------------------------------------------------
def test_header_exports_library_and_ffi_name_the_entry_point(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    ctx = open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    mk = open(os.path.join(ROOT, "reductive_amd", "csrc", "Makefile")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    name = fsr.NAME
    assert "pqhip_flat_screen" in mk
    assert name in declared and name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(L, name)
    fn = getattr(L, name)
    # the range call's arguments without d_val and with x_exp behind the metric
    rng_args = list(L.pqhip_flat_range_f32_dev.argtypes)
    assert fn.restype is i32 and list(fn.argtypes) == rng_args[:12] + [i32] + rng_args[12:14] + rng_args[15:]
    proto = re.search(r"int32_t %s\((.*?)\);" % name, hdr, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    params = [p.strip() for p in proto.split(",")]
    assert len(params) == len(fn.argtypes)
    for p, t in zip(params, fn.argtypes):
        want = vp if "*" in p else i32 if p.startswith("int32_t") else i64
        assert t is want, p
    assert "d_val" not in proto and "int32_t x_exp" in proto
    rust = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, ffi, re.S).group(1)
    assert len(rust.split(",")) == len(fn.argtypes) and "x_exp: i32" in rust
    for text in (hdr, ffi, ctx):
        assert '"%s"' % fsr.OPTION in text
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    for sentence in ("Sound, unconditionally", "A row is left out only when the kernel has proved",
                     "the capacity protocol is exactly that of the range calls", "does not read the matrix",
                     "a disallowed row is not loaded", "d > 2048: PQHIP_EUNSUPPORTED"):
        assert sentence in flat, sentence


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    fn = getattr(L, fsr.NAME)
    assert fn(None, 0, p, 1, 4, p, 4, 2, 4, 4, None, 0, 0, p, p, p, 1, z) == _lib.EINVAL
    assert fn(None, 7, None, 0, 0, None, 3, 0, 4096, 0, None, 2, 99, None, None, None, -1, z) == _lib.EINVAL


# ---- the wrappers -----------------------------------------------------------------------------------------------------------
def test_argument_checks_raise_before_the_library_is_reached(monkeypatch):
    import torch
    import reductive_amd
    from reductive_amd import _lib
    from reductive_amd.pq import PanicError

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    pq = reductive_amd.Pq(None, np.zeros((2, 4, 3), np.float32))
    monkeypatch.setattr(pq, "_cb", no_library)
    q = torch.zeros(2, 6)
    x = torch.zeros(40, 6)
    bad = [
        (dict(queries=q.double()), "queries must be float32"),
        (dict(queries=torch.zeros(1, 2, 6)), "queries must be float32"),
        (dict(vectors=x.to(torch.bfloat16)), "vectors must be float32 or float16"),
        (dict(vectors=x[0]), "vectors must be float32 or float16"),
        (dict(vectors=torch.zeros(40, 7)), "length mismatch"),
        (dict(queries=torch.zeros(2, 2049), vectors=torch.zeros(2, 2049)), "at most 2048 elements"),
        (dict(allow=torch.zeros(2, dtype=torch.int64)), "allow must be the int32 mask words"),
        (dict(allow=torch.zeros(5, dtype=torch.int32)), r"ceil\(n / 32\) words"),
        (dict(queries=q.numpy()), "must be a torch tensor"),
        (dict(vectors=x.numpy()), "must be a torch tensor"),
        (dict(), "must be CUDA tensors"),               # everything else in order: host tensors stop here
        (dict(allow=torch.zeros(2, dtype=torch.int32)), "must be CUDA tensors"),
    ]
    for change, message in bad:
        args = dict(queries=q, vectors=x)
        args.update(change)
        with pytest.raises(PanicError, match=message):
            pq.flat_screen_device(threshold=1.0, **args)
        with pytest.raises(PanicError, match=message):
            pq.flat_range_batch_device(threshold=1.0, x_exp=0, **args)
        with pytest.raises(PanicError, match=message):
            pq.flat_search_batch_device(k=3, x_exp=0, **args)
    with pytest.raises(PanicError, match="k must be between 1 and 1024"):
        pq.flat_search_batch_device(q, x, 1025, x_exp=0)


def test_class_methods_take_screen_and_default_to_the_plain_route():
    import inspect
    from reductive_amd import qmatrix
    for cls in (qmatrix.QuantizedMatrix, qmatrix.PartitionedMatrix, qmatrix.ResidualPartitionedMatrix):
        for name in ("exact_nearest", "exact_most_similar", "exact_within", "exact_similar_above"):
            fn = getattr(cls, name)
            assert fn is getattr(qmatrix._Refine, name), (cls, name)
            assert inspect.signature(fn).parameters["screen"].default is False
    for name in ("nearest", "most_similar", "within", "similar_above"):
        assert inspect.signature(getattr(qmatrix.FlatMatrix, name)).parameters["screen"].default is False
    # an unsupported width falls back silently: the plain route is chosen without touching the device
    import torch
    flat = object.__new__(qmatrix.FlatMatrix)
    flat.vectors = torch.zeros(4, 2049)
    assert not flat._screens(True)
    flat.vectors = torch.zeros(4, 2048)
    assert flat._screens(True) and not flat._screens(False)
    # the cached maximum follows the tensor
    flat.vectors = torch.full((4, 3), 2.0)
    assert flat._screen_x_exp() == 12
    flat.vectors = torch.full((4, 3), 0.5)
    assert flat._screen_x_exp() == 14
    flat.vectors.mul_(4.0)
    assert flat._screen_x_exp() == 12
