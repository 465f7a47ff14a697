"""Building a partitioned index on the device, CPU side: the two references (tests/lists_layout_ref.py against ivf_layout,
tests/residual_terms_ref.py against exact rational arithmetic), the bound that ties the device row terms to the host
route's checked on the fixture of the GPU tests with torch's CPU float64 sum standing in for the host route; header,
EXPORTS, library and rust/pqhip_ffi.rs name the three entry points and the option; the statuses a null codebook reaches;
the wrappers' shape and dtype checks, which come before any device call; partition(on_device=True) without a GPU.
(Everything that needs a codebook handle: tests/test_gpu_lists_layout.py, test_gpu_residual_terms.py,
test_gpu_qmatrix_build.py.)"""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import synth
from lists_layout_ref import PATTERNS, pattern, ref_layout
from residual_terms_ref import abs_sum, ref_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_lists_layout_dev", "pqhip_residuals_f32_dev", "pqhip_residual_terms_f32_dev")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.mark.parametrize("kind", PATTERNS + ("sorted", "reversed"))
@pytest.mark.parametrize("n,n_lists", [(0, 5), (1, 1), (65, 2), (1025, 24), (3001, 300)])
def test_layout_reference_is_ivf_layout(kind, n, n_lists):
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(n * 31 + n_lists)
    if kind in ("sorted", "reversed"):
        a = np.sort(rng.integers(0, n_lists, n).astype(np.int64))
        a = a[::-1].copy() if kind == "reversed" else a
    else:
        a = pattern(kind, n, n_lists, rng)
    assert a.shape == (n,) and (n == 0 or (a.min() >= 0 and a.max() < n_lists))
    ids, list_off, positions, lists = ref_layout(a, n_lists)
    perm, off = ivf_layout(a, n_lists)
    assert np.array_equal(ids, perm) and np.array_equal(list_off, off)
    assert np.array_equal(positions[perm], np.arange(n)) and np.array_equal(lists, a[perm])
    if kind == "edges" and n_lists > 2 and n > 1:
        assert off[1] == off[-2]                         # every list between the first and the last is empty
    if kind == "one_list" and n:
        assert np.array_equal(ids, np.arange(n))


def test_layout_reference_refuses_bad_ids():
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            ref_layout(np.array([0, 3, bad, 1]), 4)


def exact_term(q, codes_row, centroid):
    """sum_j (r^2 + 2 c r) of one row as a Fraction"""
    M, K, ds = q.shape
    tot = Fraction(0)
    for m in range(M):
        for e in range(ds):
            r, c = Fraction(float(q[m, codes_row[m], e])), Fraction(float(centroid[m * ds + e]))
            tot += r * r + 2 * c * r
    return tot


@pytest.mark.parametrize("M,ds,K", [(1, 1, 2), (1, 5, 3), (15, 4, 256), (15, 20, 256), (16, 1, 16), (100, 3, 16)])
def test_term_reference_against_exact_arithmetic(M, ds, K):
    """|t_ref - exact| <= 2^-24 |exact| (1 + 2^-20) + (d + M + 2) 2^-53 S: one f32 rounding of an f64 sum of d + M terms whose
    accumulated error is at most (d + M) 2^-53 S (first order; the + 2 pays for the second order)"""
    rng = np.random.default_rng(M * 100 + ds)
    d, n, n_lists = M * ds, 6, 5
    q = (synth.normalish(M + ds, (M, K, ds)) * np.float32(0.7)).astype(np.float32)
    q[0, 0, 0] = np.float32(-0.0)
    cen = (synth.normalish(M + ds + 1, (n_lists, d)) * np.exp2(rng.integers(-20, 20, (n_lists, d)))).astype(np.float32)
    cen[0, 0] = np.float32(0.0)
    codes = rng.integers(0, K, (n, M))
    codes[0] = 0
    assign = rng.integers(0, n_lists, n)
    assign[0] = 0
    t = ref_terms(q, codes, assign, cen)
    S = abs_sum(q, codes, assign, cen)
    assert t.dtype == np.float32 and t.shape == (n,)
    for i in range(n):
        exact = exact_term(q, codes[i], cen[assign[i]])
        err = abs(Fraction(float(t[i])) - exact)
        assert err <= abs(exact) * Fraction(1, 2 ** 24) * (1 + Fraction(1, 2 ** 20)) + Fraction(float(S[i])) * (d + M + 2) / 2 ** 53, i
    # out-of-range inputs: a code >= K reads entry 0, a bad list id gives +0
    if K < 256:
        c2 = codes.copy()
        c2[1, 0] = K
        c3 = codes.copy()
        c3[1, 0] = 0
        assert ref_terms(q, c2, assign, cen).tobytes() == ref_terms(q, c3, assign, cen).tobytes()
    a2 = assign.copy()
    a2[2], a2[3] = -1, n_lists
    t2 = ref_terms(q, codes, a2, cen)
    assert t2[2].tobytes() == np.float32(0.0).tobytes() and t2[3].tobytes() == np.float32(0.0).tobytes()
    assert t2[4].tobytes() == t[4].tobytes()


@pytest.mark.parametrize("name", ["base", "wide"])
def test_the_agreement_bound_holds_on_the_gpu_fixture_with_a_cpu_float64_sum(name):
    """The GPU test asserts |t_dev - t_host| <= 2^-23 |t_host| + 2^-40 S on the fixture of tests/test_gpu_qmatrix_add.py (the
    recipe is copied here).  Both values are one f32 rounding of an f64 sum of d + M terms with accumulated error at most
    (d + M) 2^-53 S; 2^-40 covers d + M <= 8,192.  Here torch's CPU float64 reduction stands in for the host route."""
    import torch
    from oracle import pq_oracle as orc
    CONFIGS = {"base": (15, 4, 24), "lists300": (15, 4, 300), "wide": (15, 20, 24)}
    N, B = 30011, 4099
    M, dsub, n_lists = CONFIGS[name]
    d, seed = M * dsub, 7000 + 10 * sorted(CONFIGS).index(name)
    rq = synth.normalish(seed + 1, (M, 256, dsub)) * np.float32(0.7)
    centres = synth.normalish(seed + 2, (40, d)) * np.float32(3.0)
    x = (centres[np.random.default_rng(seed + 3).integers(0, 40, N + B)] + synth.normalish(seed + 4, (N + B, d))).astype(np.float32)
    centroids = np.ascontiguousarray(x[np.random.default_rng(seed + 5).choice(N, n_lists, replace=False)])
    n = N                                      # the old rows of the fixture, whose terms the GPU test compares
    assign = orc.cluster_assignments(centroids, x[:n]).astype(np.int64)
    codes = orc.quantize_batch(rq, (x[:n] - centroids[assign]).astype(np.float32), n_threads=4)
    r = torch.from_numpy(orc.reconstruct_batch(rq, codes)).double()
    c = torch.from_numpy(centroids[assign]).double()
    t_host = (r * r + 2.0 * c * r).sum(1).float().numpy().astype(np.float64)
    t_ref = ref_terms(rq, codes, assign, centroids).astype(np.float64)
    S = abs_sum(rq, codes, assign, centroids)
    assert d + M <= 8192
    assert (np.abs(t_ref - t_host) <= 2.0 ** -23 * np.abs(t_host) + 2.0 ** -40 * S).all()


def test_header_exports_library_and_ffi_name_the_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS
        assert hasattr(L, name)
        assert re.search(r"pub fn %s\(" % name, ffi)
        assert getattr(L, name).argtypes[-1] is ctypes.c_void_p
    assert len(L.pqhip_lists_layout_dev.argtypes) == 11 and L.pqhip_lists_layout_dev.argtypes[3] is ctypes.c_int32
    assert len(L.pqhip_residuals_f32_dev.argtypes) == 12 and len(L.pqhip_residual_terms_f32_dev.argtypes) == 10
    assert '"lists_layout_wgs"' in hdr and '"lists_layout_wgs"' in ffi
    assert "#define PQHIP_LISTS_LAYOUT_MAX_LISTS 16384" in hdr
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "no element of d_ids, d_positions or d_lists is written" in flat
    assert "A codebook WITH A PROJECTION is PQHIP_EUNSUPPORTED" in flat
    ctx_src = open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    assert '{"lists_layout_wgs", &o.lists_layout_wgs}' in ctx_src


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    lay, res, trm = L.pqhip_lists_layout_dev, L.pqhip_residuals_f32_dev, L.pqhip_residual_terms_f32_dev
    assert lay(None, 0, None, 4, 0, 1, None, None, None, None, z) == _lib.EINVAL
    assert lay(None, 0, p, 8, 3, 2, p, p, p, p, z) == _lib.EINVAL
    assert lay(None, 7, p, 2, -1, 1 << 20, p, p, p, None, z) == _lib.EINVAL
    assert res(None, 0, None, 0, 1, 1, None, None, 1, None, 1, z) == _lib.EINVAL
    assert res(None, 0, p, 2, 2, 2, p, p, 1, p, 2, z) == _lib.EINVAL
    assert res(None, 9, p, -1, 0, 0, p, p, 0, p, 0, z) == _lib.EINVAL
    assert trm(None, 0, None, 0, 1, None, None, 1, None, z) == _lib.EINVAL
    assert trm(None, 0, p, 2, 2, p, p, 1, p, z) == _lib.EINVAL
    assert trm(None, 9, p, -1, 0, p, p, 0, p, z) == _lib.EINVAL


def test_wrappers_check_shapes_before_any_device_call(ra):
    """CPU tensors throughout: a mismatch must be refused before a wrapper asks for a device, a handle or a stream"""
    import torch
    pq = ra.Pq(None, np.zeros((2, 4, 3), np.float32))                  # M = 2, d = 6
    a64 = torch.zeros(5, dtype=torch.int64)
    lay = pq.lists_layout_device
    with pytest.raises(ra.PanicError, match="torch tensor"):
        lay(np.zeros(5, np.int64), 3)
    with pytest.raises(ra.PanicError, match="int32 or int64 vector"):
        lay(torch.zeros(5, dtype=torch.int16), 3)
    with pytest.raises(ra.PanicError, match="int32 or int64 vector"):
        lay(torch.zeros((5, 1), dtype=torch.int64), 3)
    for bad in (0, 16385, -1):
        with pytest.raises(ra.PanicError, match="between 1 and 16384"):
            lay(a64, bad)
    with pytest.raises(ra.PanicError, match="contiguous"):
        lay(torch.zeros(10, dtype=torch.int64)[::2], 3)
    with pytest.raises(ra.PanicError, match="CUDA tensor"):
        lay(a64, 3)
    x = torch.zeros((5, 6))
    cen = torch.zeros((3, 6))
    res = pq.residuals_device
    with pytest.raises(ra.PanicError, match="torch tensor"):
        res(np.zeros((5, 6), np.float32), a64, cen)
    with pytest.raises(ra.PanicError, match=r"float32 \[n, d\]"):
        res(x.double(), a64, cen)
    with pytest.raises(ra.PanicError, match=r"float32 \[n, d\]"):
        res(x[0], a64, cen)
    with pytest.raises(ra.PanicError, match="one list id per row"):
        res(x, a64[:4], cen)
    with pytest.raises(ra.PanicError, match="one list id per row"):
        res(x, a64.int(), cen)
    with pytest.raises(ra.PanicError, match="centroids must be float32"):
        res(x, a64, torch.zeros((3, 7)))
    with pytest.raises(ra.PanicError, match="centroids must be float32"):
        res(x, a64, cen[:0])
    with pytest.raises(ra.PanicError, match="centroids must be float32"):
        res(x, a64, cen.double())
    with pytest.raises(ra.PanicError, match="contiguous assign and centroids"):
        res(x, torch.zeros(10, dtype=torch.int64)[::2], cen)
    with pytest.raises(ra.PanicError, match="out must be"):
        res(x, a64, cen, out=torch.zeros((4, 6)))
    with pytest.raises(ra.PanicError, match="out must be"):
        res(x, a64, cen, out=torch.zeros((5, 6), dtype=torch.float64))
    with pytest.raises(ra.PanicError, match="unit column stride"):
        res(torch.zeros((5, 12))[:, ::2], a64, cen)
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        res(x, a64, cen)
    codes = torch.zeros((5, 2), dtype=torch.uint8)
    trm = pq.residual_terms_device
    with pytest.raises(ra.PanicError, match="torch tensor"):
        trm(np.zeros((5, 2), np.uint8), a64, cen)
    with pytest.raises(ra.PanicError, match=r"uint8 \[n, 2\]"):
        trm(codes.int(), a64, cen)
    with pytest.raises(ra.PanicError, match=r"uint8 \[n, 2\]"):
        trm(torch.zeros((5, 3), dtype=torch.uint8), a64, cen)
    with pytest.raises(ra.PanicError, match="one list id per row"):
        trm(codes, a64[:3], cen)
    with pytest.raises(ra.PanicError, match="centroids must be float32"):
        trm(codes, a64, torch.zeros((3, 5)))
    with pytest.raises(ra.PanicError, match="out must be"):
        trm(codes, a64, cen, out=torch.zeros(4))
    with pytest.raises(ra.PanicError, match="unit column stride"):
        trm(torch.zeros((5, 4), dtype=torch.uint8)[:, ::2], a64, cen)
    with pytest.raises(ra.PanicError, match="CUDA tensors"):
        trm(codes, a64, cen)
    assert pq._handle is None                    # no codebook handle was created: nothing reached the library
    # a quantizer with a projection is refused by the wrapper, before the library is asked
    opq = ra.Pq(np.eye(6, dtype=np.float32), np.zeros((2, 4, 3), np.float32))
    with pytest.raises(ra.PanicError, match="projection"):
        opq.residual_terms_device(codes, a64, cen)
    assert opq._handle is None


def test_on_device_build_fails_loudly_without_a_gpu(ra):
    """a matrix that is not resident on a GPU cannot take the device route: no host fallback"""
    from reductive_amd import qmatrix
    pq = ra.Pq(None, synth.normalish(11, (2, 4, 3)))
    qm = qmatrix.QuantizedMatrix(pq, np.zeros((20, 2), np.uint8), device="cpu")
    with pytest.raises(ra.PanicError, match="resident on a GPU"):
        qm.partition(3, on_device=True)
    with pytest.raises(ra.PanicError, match="resident on a GPU"):
        qm.partition_residual(3, on_device=True)
    assert pq._handle is None
    # the constructors refuse a device assignment that is not on the device of the codes
    import torch
    with pytest.raises(ra.PanicError, match="int64 CUDA tensor"):
        qmatrix.PartitionedMatrix(qm, np.zeros((3, 6), np.float32), torch.zeros(20, dtype=torch.int64))
    assert qmatrix.ResidualPartitionedMatrix.device_terms is False
