"""ADC search over a partitioned code matrix, CPU side: qmatrix.ivf_layout on hand cases, and the reference of
tests/adc_lists_ref.py against the exhaustive references on the gathered sub-matrix codes[rows of S_q] with positions
mapped back -- the sentence include/pqhip.h states for pqhip_adc_search_lists_f32_dev and its similarity twin.  The C
ABI declares and exports both entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import synth
from adc_ip_ref import ip_tables, ref_ip_search, scores
from adc_lists_ref import probed_positions, ref_lists_search
from oracle import pq_oracle as orc
from test_gpu_adc_search import ref_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    return reductive_amd


def test_ivf_layout_hand_cases(ra):
    from reductive_amd.qmatrix import ivf_layout
    perm, off = ivf_layout(np.array([2, 0, 2, 4, 0, 2]), 6)          # lists 1, 3 and 5 are empty
    assert perm.tolist() == [1, 4, 0, 2, 5, 3] and perm.dtype == np.int64
    assert off.tolist() == [0, 2, 2, 5, 5, 6, 6] and off.dtype == np.int64
    perm, off = ivf_layout(np.full(5, 3, np.uint8), 4)               # all rows in one list
    assert perm.tolist() == [0, 1, 2, 3, 4] and off.tolist() == [0, 0, 0, 0, 5]
    perm, off = ivf_layout(np.zeros(0, np.int64), 3)                 # no rows
    assert perm.size == 0 and off.tolist() == [0, 0, 0, 0]
    perm, off = ivf_layout(np.zeros(0, np.int64), 0)
    assert perm.size == 0 and off.tolist() == [0]
    for bad in (np.array([0, 3]), np.array([-1, 0])):
        with pytest.raises(ValueError):
            ivf_layout(bad, 3)
    with pytest.raises(ValueError):
        ivf_layout(np.array([0.0, 1.0]), 3)


def test_ivf_layout_is_stable_and_a_partition(ra):
    from reductive_amd.qmatrix import ivf_layout
    rng = np.random.default_rng(9300)
    for n, n_lists in ((1, 1), (1000, 7), (5000, 300), (4096, 5000)):
        a = rng.integers(0, n_lists, n)
        perm, off = ivf_layout(a, n_lists)
        assert sorted(perm.tolist()) == list(range(n))
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
        for l in range(n_lists):
            rows = perm[off[l]:off[l + 1]]
            assert (a[rows] == l).all() and (np.diff(rows) > 0).all()      # ascending original row number
            assert rows.size == (a == l).sum()


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
def test_reference_is_the_exhaustive_reference_on_the_gathered_rows(M, K, dsub, opq):
    n, n_lists, nq = 3001, 23, 6
    q, P, ys, codes, list_off, rng = _case(9310 + M, M, K, dsub, opq, n, n_lists, nq)
    dist = orc.adc_scan(orc.adc_tables(q, ys, projection=P), codes)
    sc = (synth.uniform01(9319, (n,)) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    score = scores(orc.adc_scan(ip_tables(q, ys, projection=P), codes), sc)
    dist[1, ::17] = np.nan
    dist[2, ::5] = np.float32(-0.0)
    score[1, ::13] = np.nan
    score[2, ::7] = np.float32(-0.0)
    for n_probe in (1, 3, n_lists):
        probes = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
        if n_probe == 3:
            probes[0, 1] = -1                         # padding is skipped
            probes[4] = -1                            # nothing probed
        for k in (1, 10, 64, 1024):
            got_d, got_i = ref_lists_search(dist, list_off, probes, k)
            got_s, got_j = ref_lists_search(score, list_off, probes, k, ip=True)
            for qq in range(nq):
                rows = probed_positions(list_off, probes[qq], n)
                # the exhaustive reference orders by the index in the gathered matrix: gather in position order
                rows = np.sort(rows)
                wd, wi = ref_search(dist[qq, rows], k)
                ws, wj = ref_ip_search(score[qq, rows], k)
                wi = np.where(wi < 0, -1, rows[np.clip(wi, 0, None)] if rows.size else -1)
                wj = np.where(wj < 0, -1, rows[np.clip(wj, 0, None)] if rows.size else -1)
                assert np.array_equal(got_i[qq], wi[0]) and np.array_equal(got_j[qq], wj[0])
                assert got_d[qq].tobytes() == wd[0].tobytes()
                assert np.array_equal(np.isnan(got_s[qq]), np.isnan(ws[0]))
                ok = ~np.isnan(ws[0])
                assert got_s[qq][ok].tobytes() == ws[0][ok].tobytes()
    # all lists probed: the exhaustive reference itself
    allp = np.tile(np.arange(n_lists, dtype=np.int64), (nq, 1))
    got_d, got_i = ref_lists_search(dist, list_off, allp, 50)
    wd, wi = ref_search(dist, 50)
    assert np.array_equal(got_i, wi) and got_d.tobytes() == wd.tobytes()


def test_reference_skips_bad_ids_and_clamps_ranges():
    v = np.arange(10, dtype=np.float32)[None]
    off = np.array([0, 3, 3, 12, 8], np.int64)        # list 2 runs past n = 10, list 3 is inverted
    d, i = ref_lists_search(v, off, [[1, -1, 7, 0]], 5)
    assert i[0].tolist() == [0, 1, 2, -1, -1] and np.isposinf(d[0, 3:]).all()
    d, i = ref_lists_search(v, off, [[2, 3]], 8)
    assert i[0].tolist() == [3, 4, 5, 6, 7, 8, 9, -1]
    s, i = ref_lists_search(v, off, [[2]], 3, ip=True)
    assert i[0].tolist() == [9, 8, 7] and s[0].tolist() == [9.0, 8.0, 7.0]


def test_header_exports_and_library_declare_the_list_searches(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in ("pqhip_adc_search_lists_f32_dev", "pqhip_adc_ip_search_lists_f32_dev"):
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert "every row outside S_q removed" in re.sub(r"\s*\n \*\s*", " ", hdr)
    assert "adc_lists_wgs_per_query" in hdr


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    assert L.pqhip_adc_search_lists_f32_dev(None, 0, None, 1, None, 1, 10, 4, None, 2, None, 1, 1,
                                            5, None, 5, None, 5, z) == _lib.EINVAL
    assert L.pqhip_adc_ip_search_lists_f32_dev(None, 0, None, 1, None, 1, 10, 4, None, 2, None, 1, 1, None,
                                               5, None, 5, None, 5, z) == _lib.EINVAL
