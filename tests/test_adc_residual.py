"""ADC list searches over residual codes, CPU side: the reference of tests/adc_residual_ref.py reduces to the plain
list and exhaustive references, its formulas agree with the quantities they stand for (|q - c_l - r^_i|^2 and
<q, c_l + r^_i>, evaluated directly in float64 from orc.reconstruct_batch) within a bound derived from the f32 roundings,
and the C ABI declares and exports both entry points with the formulas stated in the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import synth
from adc_ip_ref import ref_ip_search, scores
from adc_lists_ref import ref_lists_search
from adc_residual_ref import probe_slots, ref_residual_search, residual_values, scan
from oracle import pq_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_adc_search_lists_residual_f32_dev", "pqhip_adc_ip_search_lists_residual_f32_dev")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    return reductive_amd


def _case(seed, M, K, dsub, opq, n, n_lists, nq):
    d = M * dsub
    q = synth.normalish(seed, (M, K, dsub))
    P = synth.orthonormal(seed + 1, d) if opq else None
    ys = synth.normalish(seed + 2, (nq, d))
    codes = synth.codes_u8(seed + 3, (n, M), K)
    rng = np.random.default_rng(seed + 4)
    cuts = np.sort(rng.integers(0, n + 1, n_lists - 1))
    list_off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    return q, P, ys, codes, list_off, rng


@pytest.mark.parametrize("M,K,dsub,opq", [(15, 256, 20, False), (3, 7, 5, True)])
def test_reference_reduces_to_the_plain_searches(M, K, dsub, opq):
    """bias = 0 and no scales: the similarity reference is the plain list reference over the same scan; with every
    list probed it is the exhaustive reference.  (fl(0 + s) = s: a scan from +0 is never -0.)"""
    n, n_lists, nq = 3001, 23, 6
    q, P, ys, codes, list_off, rng = _case(9600 + M, M, K, dsub, opq, n, n_lists, nq)
    s = scan(q, ys, codes, projection=P)
    for n_probe in (1, 3, n_lists):
        probes = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
        if n_probe == 3:
            probes[0, 1] = -1
            probes[4] = -1
        zero = np.zeros(probes.shape, np.float32)
        for k in (1, 10, 64, 1024):
            got_s, got_i = ref_residual_search(s, list_off, probes, zero, k, ip=True)
            want_s, want_i = ref_lists_search(scores(s), list_off, probes, k, ip=True)
            assert np.array_equal(got_i, want_i) and got_s.tobytes() == want_s.tobytes()
    allp = np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))
    got_s, got_i = ref_residual_search(s, list_off, allp, np.zeros(allp.shape, np.float32), 50, ip=True)
    want_s, want_i = ref_ip_search(s, 50)
    assert np.array_equal(got_i, want_i) and got_s.tobytes() == want_s.tobytes()
    # scales and a constant bias: a constant shift of the scan before the multiply
    sc = (synth.uniform01(9609, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    got_s, got_i = ref_residual_search(s, list_off, allp, np.full(allp.shape, 2.5, np.float32), 50, scales=sc, ip=True)
    want_s, want_i = ref_ip_search(scores((s + np.float32(2.5)).astype(np.float32), sc), 50)
    assert np.array_equal(got_i, want_i) and got_s.tobytes() == want_s.tobytes()


def test_reference_slots_and_skipped_bias():
    """the slot map follows the rules for bad input, and a bias at a skipped slot (here NaN) reaches no value"""
    off = np.array([0, 3, 3, 12, 8], np.int64)         # n = 10: list 1 empty, list 2 clamped, list 3 inverted
    assert probe_slots(off, [1, -1, 7, 0], 10).tolist() == [3, 3, 3] + [-1] * 7
    assert probe_slots(off, [2, 3], 10).tolist() == [-1] * 3 + [0] * 7
    s = np.arange(10, dtype=np.float32)[None]
    bias = np.array([[np.nan, np.nan, np.nan, 1.0]], np.float32)
    v, i = ref_residual_search(s, off, [[1, -1, 7, 0]], bias, 5, ip=True)
    assert i[0].tolist() == [2, 1, 0, -1, -1] and v[0, :3].tolist() == [3.0, 2.0, 1.0] and np.isneginf(v[0, 3:]).all()
    d, i = ref_residual_search(s, off, [[1, -1, 7, 0]], bias, 5, terms=np.full(10, 0.5, np.float32))
    assert i[0].tolist() == [2, 1, 0, -1, -1] and d[0, :3].tolist() == [-2.5, -0.5, 1.5]


def test_formulas_agree_with_the_quantities_they_stand_for():
    """The f32 formulas against |y - c_l - r^_i|^2 and <y, c_l + r^_i> evaluated directly in float64 from
    orc.reconstruct_batch (plain PQ: the reconstruction is the concatenation of centroids, exactly).

    Take the f32 data y, c_l, r^_i as exact reals and let A = |y - c_l|^2, T = |r^|^2 + 2 <c_l, r^>, S = <y, r^>,
    B = <y, c_l>; then D = A + T - 2 S and <y, c_l + r^> = B + S exactly.  With u = 2^-24 and g(n) = n u / (1 - n u):
      a = f32(A), t = f32(T), b = f32(B)   (evaluated in float64, rounded once):   |a - A| <= u |A|, likewise t, b;
      s, the oracle's scan: a dsub-term f32 dot per subquantizer (at most dsub roundings on any term's path) followed
        by the M-term sequential sum, hence |s - S| <= g(dsub + M) sum_j |y_j r^_j|   (Higham, Accuracy and Stability,
        eq. 3.4-3.5: error of a sum of products whatever the order of summation);
      x1 = fl(a + t): |x1 - (a + t)| <= u |a + t|;   fl(s + s) = 2 s exactly;   dist = fl(x1 - 2 s): <= u |x1 - 2 s|.
    So |dist - D|  <= u (|A| + |T| + |a + t| + |x1 - 2 s|) + 2 g(dsub + M) sum_j |y_j r^_j|
       |score - (B + S)| <= u (|B| + |b + s|) + g(dsub + M) sum_j |y_j r^_j|
    plus the float64 evaluation of A, T, B, S, D themselves: (d + 4) 2^-52 times the sum of the absolute values of
    their terms, which the bound carries as `slack`."""
    M, K, dsub, n, n_lists, nq = 8, 16, 4, 2003, 11, 5
    d = M * dsub
    q, _, ys, codes, list_off, rng = _case(9620, M, K, dsub, False, n, n_lists, nq)
    ys = (ys * np.float32(2.0)).astype(np.float32)
    C = (synth.normalish(9625, (n_lists, d)) * np.float32(3.0)).astype(np.float32)
    rec = orc.reconstruct_batch(q, codes).astype(np.float64)
    lists = np.searchsorted(list_off[1:], np.arange(n), side="right")
    cl = C[lists].astype(np.float64)
    T = (rec * rec + 2.0 * cl * rec).sum(1)
    T_abs = (rec * rec + np.abs(2.0 * cl * rec)).sum(1)
    t = T.astype(np.float32)
    s = scan(q, ys, codes)
    u = 2.0 ** -24
    g = (dsub + M) * u / (1.0 - (dsub + M) * u)
    probes = np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))
    A_all = ((ys[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(2)      # [nq, n_lists]
    B_all = ys.astype(np.float64) @ C.astype(np.float64).T
    dist = residual_values(s, list_off, probes, A_all.astype(np.float32), terms=t)
    score = residual_values(s, list_off, probes, B_all.astype(np.float32), ip=True)
    worst = 0.0
    for qq in range(nq):
        y = ys[qq].astype(np.float64)
        A, B = A_all[qq][lists], B_all[qq][lists]
        a, b = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
        S_abs = (np.abs(y[None] * rec)).sum(1)
        D = ((y[None] - cl - rec) ** 2).sum(1)
        s64 = s[qq].astype(np.float64)
        x1 = (a.astype(np.float32) + t).astype(np.float64)
        slack = (d + 4) * 2.0 ** -52 * (2.0 * (A + T_abs + 2.0 * S_abs) + np.abs(y[None] * cl).sum(1))
        bound_d = u * (np.abs(A) + np.abs(T) + np.abs(a + t) + np.abs(x1 - 2.0 * s64)) + 2.0 * g * S_abs + slack
        err_d = np.abs(dist[qq].astype(np.float64) - D)
        assert (err_d <= bound_d).all(), (err_d.max(), bound_d.min())
        sim = (y[None] * (cl + rec)).sum(1)
        bound_s = u * (np.abs(B) + np.abs(b + s64)) + g * S_abs + slack
        err_s = np.abs(score[qq].astype(np.float64) - sim)
        assert (err_s <= bound_s).all(), (err_s.max(), bound_s.min())
        # the bound is a bound on rounding, not a licence: leaving the row term out, or the factor 2, misses it
        no_term = residual_values(s[qq:qq + 1], list_off, probes[:1], A_all[qq:qq + 1].astype(np.float32),
                                  terms=np.zeros(n, np.float32))[0]
        assert (np.abs(no_term.astype(np.float64) - D) > bound_d).mean() > 0.99
        assert (np.abs((x1 - s64) - D) > bound_d).mean() > 0.99
        worst = max(worst, float((bound_d / np.maximum(D, 1e-30)).max()))
    assert worst < 1e-3                                 # and it is tight: relative to the distances, below 1e-3


def test_header_exports_and_library_declare_the_residual_searches(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "dist = fl( fl(bias[q][p] + term[i]) - fl(s + s) )" in flat
    assert "score = fl( fl(bias[q][p] + s) * scale[i] )" in flat
    assert "score = fl(bias[q][p] + s)" in flat
    assert "The bias of a skipped probe" in flat
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in ffi, name


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    assert L.pqhip_adc_search_lists_residual_f32_dev(None, 0, None, 1, None, 1, 10, 4, None, 2, None, 1, 1, None, 1, None,
                                                     5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_residual_f32_dev(None, 0, None, 1, None, 1, 10, 4, None, 2, None, 1, 1, None, 1, None,
                                                        5, None, 5, None, 5, z) == _lib.EINVAL
