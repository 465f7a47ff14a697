"""ADC similarity search, CPU side (include/pqhip.h: pqhip_adc_ip_tables_f32_dev, pqhip_adc_ip_search_f32_dev): the
reference inner-product tables are pinned to the oracle's distance tables bit for bit, their table sums to the real
inner product with the oracle's reconstructions, and the reference selection to the declared order; the C ABI declares
and exports both entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import synth
from adc_ip_ref import ip_tables, l2_from_ip, ref_ip_search, unrolled_dot_rows
from oracle import pq_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(15, 256, 20, False), (48, 256, 16, False), (10, 128, 2, False), (3, 7, 5, True)]


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    return reductive_amd


def test_unrolled_dot_matches_oracle():
    for n in (1, 5, 8, 16, 20, 23):
        a = synth.normalish(9600 + n, (9, n))
        b = synth.normalish(9601 + n, (n,))
        got = unrolled_dot_rows(a, b)
        assert got.tobytes() == np.array([orc.dot_unrolled(a[r], b) for r in range(9)], np.float32).tobytes()
    # the query rotation (rotate_query) is pinned to the oracle by the OPQ case of the next test


@pytest.mark.parametrize("M,K,dsub,opq", SHAPES)
def test_ip_tables_are_the_dp_term_of_the_distance_tables(M, K, dsub, opq):
    d = M * dsub
    q = synth.normalish(9610 + d + K, (M, K, dsub))
    P = synth.orthonormal(9611 + d, d) if opq else None
    ys = synth.normalish(9612 + d, (3, d))
    ip = ip_tables(q, ys, projection=P)
    assert ip.shape == (3, M, K) and ip.dtype == np.float32
    assert l2_from_ip(q, ys, ip, projection=P).tobytes() == orc.adc_tables(q, ys, projection=P).tobytes()
    one = ip_tables(q, ys[1], projection=P)
    assert one.shape == (M, K) and one.tobytes() == ip[1].tobytes()


@pytest.mark.parametrize("M,K,dsub,opq", SHAPES)
def test_ip_table_sum_is_the_inner_product_with_the_reconstruction(M, K, dsub, opq):
    d = M * dsub
    q = synth.normalish(9620 + d + K, (M, K, dsub))
    P = synth.orthonormal(9621 + d, d) if opq else None
    ys = synth.normalish(9622 + d, (2, d))
    codes = synth.codes_u8(9623 + d, (500, M), K)
    ip = ip_tables(q, ys, projection=P)
    s = orc.adc_scan(ip, codes)
    rec = orc.reconstruct_batch(q, codes, projection=P).astype(np.float64)
    want = ys.astype(np.float64) @ rec.T
    scale = np.linalg.norm(ys.astype(np.float64), axis=1)[:, None] * np.linalg.norm(rec, axis=1)[None, :]
    assert (np.abs(s - want) <= 1e-4 * scale).all()


def test_reference_selection_order_and_padding():
    v = np.array([np.nan, -np.inf, 0.0, -0.0, 1.0, np.nan, np.inf, 1.0, -2.0], np.float32)
    s, i = ref_ip_search(v, 12)
    # +Inf, the two 1.0 (smaller index first), the two zeros (equal: index order), -2, -Inf, then the NaNs
    assert i[0].tolist() == [6, 4, 7, 2, 3, 8, 1, 0, 5, -1, -1, -1]
    assert s[0, :7].tolist() == [np.inf, 1.0, 1.0, 0.0, 0.0, -2.0, -np.inf]
    assert not np.signbit(s[0, 4])                    # -0 comes back as +0
    assert np.isnan(s[0, 7:9]).all() and np.isneginf(s[0, 9:]).all()
    # the selection of a score is the distance selection of its negation (first-minimum order, oracle first_min)
    rng = np.random.default_rng(9630)
    for _ in range(100):
        n = int(rng.integers(1, 200))
        w = rng.integers(-3, 4, n).astype(np.float32)
        for special in (np.nan, np.inf, -np.inf, -0.0):
            w[rng.random(n) < 0.1] = special
        _, i = ref_ip_search(w, 3)
        assert i[0, 0] == orc.first_min(-w)


def test_header_exports_and_library_declare_both_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in ("pqhip_adc_ip_tables_f32_dev", "pqhip_adc_ip_search_f32_dev"):
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    rc = L.pqhip_adc_ip_tables_f32_dev(None, 0, None, 1, 4, None, None)
    assert rc == _lib.EINVAL
    rc = L.pqhip_adc_ip_search_f32_dev(None, 0, None, 1, None, 1, 10, 4, None, 5, None, 5, None, 5, ctypes.c_void_p(0))
    assert rc == _lib.EINVAL
