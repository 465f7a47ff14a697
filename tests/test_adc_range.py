"""ADC range searches, CPU side: the references of tests/adc_range_ref.py tied to the top-k references the suite
already trusts (a threshold equal to the k-th value returns, as a set, the top-k' rows for k' = its count; integer values,
so ties sit on the boundary), their IEEE edge cases (NaN values, NaN / +-Inf thresholds, -0), masks against "remove the
rows and map back", the residual values against adc_residual_ref.residual_values; sort_ranges on CPU tensors against a
Python sort per segment; header, EXPORTS, library and rust/pqhip_ffi.rs name the six entry points and the two options;
the argument checks that a null codebook reaches.  (A status that needs a codebook handle -- EUNSUPPORTED, ESHAPE and the
precedence among them -- needs a device to create one: tests/test_gpu_adc_range.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from adc_ip_ref import ref_ip_search
from adc_lists_ref import probed_positions, ref_lists_search
from adc_masked_ref import compressed_offsets, pack_ref, unpack_ref
from adc_range_ref import ref_range, ref_range_lists, ref_range_residual
from adc_residual_ref import ref_residual_search, residual_values
from test_gpu_adc_search import ref_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_adc_range_f32_dev", "pqhip_adc_ip_range_f32_dev", "pqhip_adc_range_lists_f32_dev",
         "pqhip_adc_ip_range_lists_f32_dev", "pqhip_adc_range_lists_residual_f32_dev",
         "pqhip_adc_ip_range_lists_residual_f32_dev")
OPTIONS = ("adc_range_wgs", "adc_range_wgs_per_query")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def draw_values(rng, nq, n, specials=True):
    """small integers (many ties); with specials NaN, +-Inf and -0 planted"""
    v = rng.integers(-3, 4, (nq, n)).astype(np.float32)
    if specials:
        for special in (np.nan, np.inf, -np.inf, -0.0):
            v[rng.random((nq, n)) < 0.08] = special
    return v


def draw_lists(rng, n, n_lists):
    cuts = np.sort(rng.integers(0, n + 1, n_lists - 1))
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    for l in range(0, n_lists - 1, 4):
        off[l + 1] = off[l]
    return np.maximum.accumulate(off)


def draw_probes(rng, nq, n_lists, n_probe):
    pr = np.stack([rng.permutation(n_lists)[:n_probe] for _ in range(nq)]).astype(np.int64)
    pr[rng.random(pr.shape) < 0.2] = -1
    return pr


def segment(csr, q):
    lims, val, idx = csr
    return val[lims[q]:lims[q + 1]], idx[lims[q]:lims[q + 1]]


def check_against_topk(csr, q, values_q, topk, kth, ip):
    """topk(k) -> (val [k], idx [k]) of query q under the trusted reference; kth: the threshold was its kth value"""
    val, idx = segment(csr, q)
    assert val.tobytes() == values_q[idx].tobytes()                       # bit for bit, the sign of a zero included
    c = idx.size
    if np.isnan(kth):
        assert c == 0                                                     # a NaN threshold matches nothing
        return
    assert c >= 1
    tv, ti = topk(c)
    assert sorted(idx.tolist()) == sorted(ti.tolist())                    # as a set: the top-k' rows, k' = the count
    assert not np.isnan(tv).any()
    more_v, more_i = topk(c + 1)                                          # and the next row, if any, is beyond the threshold
    if more_i[c] >= 0:
        nxt = more_v[c]
        assert np.isnan(nxt) or (nxt < kth if ip else nxt > kth)


@pytest.mark.parametrize("ip", [False, True])
def test_threshold_at_the_kth_value_is_the_topk_set(ip):
    rng = np.random.default_rng(7101)
    for n in (1, 40, 300):
        v = draw_values(rng, 3, n)
        for k in (1, 5, 37):
            if k > n:
                continue
            tv, _ = (ref_ip_search(v, k) if ip else ref_search(v, k))
            thr = tv[:, k - 1].copy()
            csr = ref_range(v, thr, ip=ip)
            assert csr[0][0] == 0 and csr[0].dtype == np.int64
            for q in range(3):
                _, idx = segment(csr, q)
                assert (np.diff(idx) > 0).all()                           # ascending row index
                one = lambda kk, q=q: tuple(a[0] for a in (ref_ip_search(v[q:q + 1], kk) if ip else ref_search(v[q:q + 1], kk)))
                check_against_topk(csr, q, v[q], one, thr[q], ip)


@pytest.mark.parametrize("ip", [False, True])
def test_list_and_residual_forms_against_the_topk_references(ip):
    rng = np.random.default_rng(7102)
    for n in (50, 400):
        nq, n_lists = 3, 9
        v = draw_values(rng, nq, n)
        off, pr = draw_lists(rng, n, n_lists), draw_probes(rng, nq, n_lists, 4)
        bias = rng.integers(-2, 3, pr.shape).astype(np.float32)
        extra = rng.integers(-2, 3, n).astype(np.float32)
        kw = dict(scales=extra) if ip else dict(terms=extra)
        rvals = residual_values(v, off, pr, bias, ip=ip, **kw)
        for k in (1, 6, 30):
            tv, _ = ref_lists_search(v, off, pr, k, ip=ip)
            thr = tv[:, k - 1].copy()                                     # +-Inf padding when |S_q| < k: a legal threshold
            csr = ref_range_lists(v, off, pr, thr, ip=ip)
            rv, _ = ref_residual_search(v, off, pr, bias, k, ip=ip, **kw)
            rthr = rv[:, k - 1].copy()
            rcsr = ref_range_residual(v, off, pr, bias, rthr, ip=ip, **kw)
            for q in range(nq):
                pos = probed_positions(off, pr[q], n)
                _, idx = segment(csr, q)
                assert np.array_equal(idx, pos[np.isin(pos, idx)])        # the order of the concatenation
                if pos.size >= k:
                    one = lambda kk, q=q: tuple(a[0] for a in ref_lists_search(v[q:q + 1], off, pr[q:q + 1], kk, ip=ip))
                    check_against_topk(csr, q, v[q], one, thr[q], ip)
                    rval, ridx = segment(rcsr, q)
                    # the residual values are those of residual_values (which carries a zero distance as +0)
                    assert np.array_equal(rval + np.float32(0.0), rvals[q, ridx] + np.float32(0.0))
                    one = lambda kk, q=q: tuple(a[0] for a in ref_residual_search(v[q:q + 1], off, pr[q:q + 1], bias[q:q + 1],
                                                                                  kk, ip=ip, **kw))
                    check_against_topk((rcsr[0], rvals[q, rcsr[2]], rcsr[2]), q, rvals[q], one, rthr[q], ip)


def test_ieee_edge_cases():
    v = np.array([[1.0, np.nan, -0.0, 0.0, np.inf, -np.inf, 2.0]], np.float32)
    assert ref_range(v, np.nan)[0].tolist() == [0, 0] and ref_range(v, np.nan, ip=True)[0].tolist() == [0, 0]
    assert ref_range(v, np.inf)[2].tolist() == [0, 2, 3, 4, 5, 6]        # +Inf: every non-NaN row
    assert ref_range(v, -np.inf, ip=True)[2].tolist() == [0, 2, 3, 4, 5, 6]
    assert ref_range(v, -np.inf)[2].tolist() == [5] and ref_range(v, np.inf, ip=True)[2].tolist() == [4]
    lims, val, idx = ref_range(v, -0.0)                                   # -0 == +0 in the comparison ...
    assert idx.tolist() == [2, 3, 5]
    assert np.signbit(val).tolist() == [True, False, True]                # ... and the sign of a zero is kept
    assert ref_range(v, 0.0, ip=True)[2].tolist() == [0, 2, 3, 4, 6]
    assert ref_range(v, 1.0)[2].tolist() == [0, 2, 3, 5]                  # the boundary is included
    # several queries, each its own threshold; lims are the running counts
    v2 = np.array([[1, 2, 3], [3, 2, 1]], np.float32)
    lims, val, idx = ref_range(v2, [2.0, 0.5])
    assert lims.tolist() == [0, 2, 2] and idx.tolist() == [0, 1] and val.tolist() == [1.0, 2.0]
    # a list named twice returns its rows twice; -1 and a bad id are skipped; non-ascending probe order is kept
    off = np.array([0, 2, 2, 5], np.int64)
    lims, val, idx = ref_range_lists(np.arange(5, dtype=np.float32)[None], off, np.array([[2, -1, 0, 7, 2, 1]]), 10.0)
    assert idx.tolist() == [2, 3, 4, 0, 1, 2, 3, 4] and lims.tolist() == [0, 8]
    # residual: the bias of the slot through which the row is reached, NaN bias on a skipped probe enters nothing
    s = np.zeros((1, 5), np.float32)
    bias = np.array([[10.0, np.nan, 20.0, np.nan, 30.0, np.nan]], np.float32)
    lims, val, idx = ref_range_residual(s, off, np.array([[2, -1, 0, 7, 2, 1]]), bias, 25.0, terms=np.zeros(5, np.float32))
    assert idx.tolist() == [2, 3, 4, 0, 1] and val.tolist() == [10.0] * 3 + [20.0] * 2
    lims, val, idx = ref_range_residual(s, off, np.array([[2, -1, 0, 7, 2, 1]]), bias, 25.0, ip=True)
    assert idx.tolist() == [2, 3, 4] and val.tolist() == [30.0] * 3


@pytest.mark.parametrize("ip", [False, True])
def test_masks_remove_the_rows_and_map_back(ip):
    rng = np.random.default_rng(7103)
    for trial in range(20):
        n, nq, n_lists = int(rng.integers(1, 300)), 3, 7
        v = draw_values(rng, nq, n)
        allow = rng.random(n) < rng.choice([0.0, 0.01, 0.5, 1.0])
        assert np.array_equal(unpack_ref(pack_ref(allow), n), allow)
        rows = np.flatnonzero(allow)
        thr = rng.integers(-2, 3, nq).astype(np.float32)
        lims, val, idx = ref_range(v, thr, ip=ip, allow=allow)
        l2, v2, i2 = ref_range(v[:, rows], thr, ip=ip)
        assert np.array_equal(lims, l2) and val.tobytes() == v2.tobytes() and np.array_equal(idx, rows[i2])
        off, pr = draw_lists(rng, n, n_lists), draw_probes(rng, nq, n_lists, 4)
        coff = compressed_offsets(off, allow)
        lims, val, idx = ref_range_lists(v, off, pr, thr, ip=ip, allow=allow)
        l2, v2, i2 = ref_range_lists(v[:, rows], coff, pr, thr, ip=ip)
        assert np.array_equal(lims, l2) and val.tobytes() == v2.tobytes() and np.array_equal(idx, rows[i2])
        bias = rng.integers(-2, 3, pr.shape).astype(np.float32)
        extra = rng.integers(-2, 3, n).astype(np.float32)
        poisoned = extra.copy()
        poisoned[~allow] = np.nan                                         # a NaN term / scale in a disallowed row changes nothing
        kw = lambda e: dict(scales=e) if ip else dict(terms=e)
        got = ref_range_residual(v, off, pr, bias, thr, ip=ip, allow=allow, **kw(poisoned))
        l2, v2, i2 = ref_range_residual(v[:, rows], coff, pr, bias, thr, ip=ip, **kw(extra[rows]))
        assert np.array_equal(got[0], l2) and got[1].tobytes() == v2.tobytes() and np.array_equal(got[2], rows[i2])
        ones = np.ones(n, bool)
        for a, b in zip(ref_range_lists(v, off, pr, thr, ip=ip, allow=ones), ref_range_lists(v, off, pr, thr, ip=ip)):
            assert a.tobytes() == b.tobytes()


def test_sort_ranges_on_cpu_tensors():
    import torch
    from reductive_amd.qmatrix import sort_ranges
    rng = np.random.default_rng(7104)
    for descending in (False, True):
        counts = np.array([5, 0, 1, 0, 0, 40, 3, 0])
        lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        val = rng.integers(-2, 3, lims[-1]).astype(np.float32)            # equal values: ties keep the unsorted order
        val[rng.random(val.size) < 0.2] = -0.0
        idx = rng.permutation(1000)[:lims[-1]].astype(np.int64)
        sv, si = sort_ranges(torch.from_numpy(lims), torch.from_numpy(val), torch.from_numpy(idx), descending)
        want_v, want_i = [], []
        for q in range(counts.size):
            seg = list(range(lims[q], lims[q + 1]))
            seg.sort(key=lambda j: -float(val[j]) if descending else float(val[j]))   # Python's sort is stable
            want_v += [val[j] for j in seg]
            want_i += [idx[j] for j in seg]
        assert si.tolist() == [int(i) for i in want_i]
        assert sv.numpy().tobytes() == np.array(want_v, np.float32).tobytes()
    e = torch.zeros(0)
    sv, si = sort_ranges(torch.zeros(3, dtype=torch.int64), e, e.long(), False)       # all segments empty
    assert sv.numel() == 0 and si.numel() == 0


def test_header_exports_library_and_ffi_name_the_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        fn = getattr(L, name)
        assert fn.argtypes[8] is ctypes.c_void_p and fn.argtypes[-2] is ctypes.c_int64   # d_allow .. capacity, stream
    for opt in OPTIONS:
        assert '"%s"' % opt in hdr and '"%s"' % opt in ffi, opt
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "valid prefix" in flat and "ascending row index" in flat
    assert "capacity == 0 is a pure count call" in flat
    assert "second call always suffices" in flat


def test_argument_checks_a_null_codebook_reaches(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    lists = (None, 2, None, 1, 1)

    def calls(code_bytes, capacity, lims):
        head = (None, 0, None, 1, None, code_bytes, 10, 4, None)          # .., codes_row_stride, d_allow
        tail = (None, lims, None, None, capacity, z)                      # threshold, lims, val, idx, capacity, stream
        return [L.pqhip_adc_range_f32_dev(*head, *tail),
                L.pqhip_adc_ip_range_f32_dev(*head, None, *tail),
                L.pqhip_adc_range_lists_f32_dev(*head, *lists, *tail),
                L.pqhip_adc_ip_range_lists_f32_dev(*head, *lists, None, *tail),
                L.pqhip_adc_range_lists_residual_f32_dev(*head, *lists, None, 1, None, *tail),
                L.pqhip_adc_ip_range_lists_residual_f32_dev(*head, *lists, None, 1, None, *tail)]

    buf = (ctypes.c_int64 * 2)()
    # Whatever else is passed, a null codebook is EINVAL: that is all a call without a handle can show.  capacity < 0,
    # a null d_lims, the scope, the shape and their precedence need a handle and are in
    # test_gpu_adc_range.py::test_gpu_range_status_codes_and_precedence.
    assert calls(1, 0, None) == [_lib.EINVAL] * 6
    assert calls(1, -1, ctypes.cast(buf, ctypes.c_void_p)) == [_lib.EINVAL] * 6
    assert calls(4, 0, ctypes.cast(buf, ctypes.c_void_p)) == [_lib.EINVAL] * 6
    assert list(buf) == [0, 0]                                            # nothing was written


def test_python_wrappers():
    from reductive_amd import Pq, qmatrix
    for name in ("adc_range_device", "adc_ip_range_device", "adc_range_lists_device", "adc_ip_range_lists_device",
                 "adc_range_lists_residual_device", "adc_ip_range_lists_residual_device"):
        par = inspect.signature(getattr(Pq, name)).parameters
        assert "threshold" in par and "k" not in par, name
        assert par["allow"].default is None and par["capacity"].default is None, name
    for cls in (qmatrix.QuantizedMatrix, qmatrix.PartitionedMatrix, qmatrix.ResidualPartitionedMatrix):
        for name in ("within", "similar_above"):
            par = inspect.signature(getattr(cls, name)).parameters
            assert par["allow"].default is None and par["sort"].default is False and "refine" not in par, (cls, name)
            assert ("nprobe" in par) == (cls is not qmatrix.QuantizedMatrix)
            assert "1,024" in getattr(cls, "within").__doc__
