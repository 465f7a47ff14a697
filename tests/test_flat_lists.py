"""CPU tests of the exact search in probed lists (include/pqhip.h: pqhip_flat_search_lists_f32_dev): pins
tests/flat_lists_ref.py -- flat_search_ref.ref_flat_search under the mask "the row lies in a probed list and is allowed",
plus the range flag -- on empty lists, probe order, -1 padding, k beyond the probed rows, ties across lists, NaN in an
unprobed list and bad ids / offsets; header, EXPORTS, SIGNATURES, library and rust/pqhip_ffi.rs name the entry point and
its option; a null codebook is EINVAL; the argument checks of Pq.flat_search_lists_device raise before the library is
reached."""
import ctypes
import os
import re

import numpy as np
import pytest

import flat_lists_ref as flr
import flat_search_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_flat_search_lists_f32_dev"
OPTION = "flat_lists_wgs_per_query"


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def _data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ip", [False, True])
def test_reference_is_the_flat_search_under_the_mask_of_the_probed_lists(ip):
    q, x = _data(1, 60, 9, 3)
    off = flr.offsets([0, 7, 0, 20, 1, 32, 0])                   # empty lists first, between and last
    probes = np.array([[3, 0, 4], [6, 2, 0], [5, 1, -1]], np.int64)
    v, i, flag = flr.ref_flat_search_lists(q, x, off, probes, 12, ip=ip)
    assert not flag
    for qi, lists in enumerate(([3, 4], [], [5, 1])):
        mask = np.zeros(60, bool)
        for l in lists:
            mask[off[l]:off[l + 1]] = True
        wv, wi = fr.ref_flat_search(q[qi:qi + 1], x, 12, ip=ip, allow=mask)
        flr.assert_same(v[qi:qi + 1], i[qi:qi + 1], wv, wi)
    assert (i[1] == -1).all() and (v[1] == (-np.inf if ip else np.inf)).all()      # only empty lists probed
    assert (i[0, :12] >= 0).all() and set(i[0].tolist()) <= set(range(7, 28))


def test_reference_does_not_depend_on_the_probe_order_or_the_padding():
    q, x = _data(2, 50, 5, 1)
    off = flr.offsets([10, 0, 15, 25])
    want = flr.ref_flat_search_lists(q, x, off, [[3, 0, 2]], 30)
    for probes in ([[0, 2, 3]], [[2, 3, 0]], [[-1, 2, -1, 3, 0, -1]], [[1, 0, 1, 2, 3]]):
        got = flr.ref_flat_search_lists(q, x, off, probes, 30)
        flr.assert_same(got[0], got[1], want[0], want[1])
        assert not got[2]
    # every list probed: the unmasked exhaustive search
    wv, wi = fr.ref_flat_search(q, x, 30)
    flr.assert_same(want[0], want[1], wv, wi)
    v, i, flag = flr.ref_flat_search_lists(q, x, off, [[-1, -1]], 4)
    assert (i == -1).all() and (v == np.inf).all() and not flag


def test_reference_pads_when_k_exceeds_the_probed_rows():
    q, x = _data(3, 40, 6, 2)
    off = flr.offsets([3, 30, 7])
    v, i, _ = flr.ref_flat_search_lists(q, x, off, [[0, -1], [2, 0]], 12, ip=True)
    assert sorted(i[0, :3].tolist()) == [0, 1, 2] and (i[0, 3:] == -1).all() and (v[0, 3:] == -np.inf).all()
    assert sorted(i[1, :10].tolist()) == [0, 1, 2, 33, 34, 35, 36, 37, 38, 39] and (i[1, 10:] == -1).all()


def test_reference_ties_across_lists_go_to_the_smaller_position():
    q = np.zeros((1, 8), np.float32)
    x = np.ones((12, 8), np.float32)
    x[9] = 0.5
    x[2] = x[9]                                      # the same row in list 0 and in list 2
    off = flr.offsets([4, 4, 4])
    for probes in ([[2, 0]], [[0, 2]]):              # the list probed last holds the smaller position
        v, i, _ = flr.ref_flat_search_lists(q, x, off, probes, 4)
        assert i.tolist() == [[2, 9, 0, 1]] and v[0, 0] == v[0, 1] == np.float32(2.0)
    v, i, _ = flr.ref_flat_search_lists(q + 1, x, off, [[2, 1]], 3, ip=True)
    assert i.tolist() == [[4, 5, 6]] and (v == np.float32(8.0)).all()
    allow = np.ones(12, bool)
    allow[2] = False
    v, i, _ = flr.ref_flat_search_lists(q, x, off, [[0, 2]], 2, allow=allow)
    assert i.tolist() == [[9, 0]]


def test_reference_nan_in_an_unprobed_list_or_a_disallowed_row_changes_nothing():
    q, x = _data(4, 30, 7, 2)
    off = flr.offsets([10, 10, 10])
    probes = [[0, 2], [2, -1]]
    allow = np.ones(30, bool)
    allow[[3, 25]] = False
    want = flr.ref_flat_search_lists(q, x, off, probes, 8, allow=allow)
    bad = x.copy()
    bad[10:20] = np.nan
    bad[[3, 25]] = np.nan
    got = flr.ref_flat_search_lists(q, bad, off, probes, 8, allow=allow)
    flr.assert_same(got[0], got[1], want[0], want[1])
    assert not np.isnan(got[0]).any()
    v, _, _ = flr.ref_flat_search_lists(q, bad, off, [[1], [1]], 10)       # probed: NaN rows come last, canonical
    assert np.isnan(v).all()


def test_reference_flags_bad_ids_and_offsets_and_clamps():
    q, x = _data(5, 20, 4, 1)
    off = flr.offsets([5, 5, 10])
    want = flr.ref_flat_search_lists(q, x, off, [[0, 2]], 20)
    for probes in ([[0, 3, 2]], [[0, -2, 2]], [[2, 0, 1 << 40]]):
        got = flr.ref_flat_search_lists(q, x, off, probes, 20)
        assert got[2]
        flr.assert_same(got[0], got[1], want[0], want[1])
    beyond = off.copy()
    beyond[3] = 27                                    # the last list runs past the rows: clamped to n
    got = flr.ref_flat_search_lists(q, x, beyond, [[0, 2]], 20)
    assert got[2]
    flr.assert_same(got[0], got[1], want[0], want[1])
    assert not flr.ref_flat_search_lists(q, x, beyond, [[0, 1]], 20)[2]   # an offset nobody probes is not looked at
    inverted = np.array([0, 5, 3, 20], np.int64)      # list 1 = [5, 3): empty, flagged
    got = flr.ref_flat_search_lists(q, x, inverted, [[1, 0]], 6)
    assert got[2] and sorted(got[1][0, :5].tolist()) == [0, 1, 2, 3, 4] and got[1][0, 5] == -1
    mask, flag = flr.probed_mask(np.array([-4, 5, 20], np.int64), [0], 20)
    assert flag and mask[:5].all() and not mask[5:].any()


# ---- the declarations ------------------------------------------------------------------------------------------------------
def test_header_exports_library_and_ffi_name_the_entry_point(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    ctx = open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    mk = open(os.path.join(ROOT, "reductive_amd", "csrc", "Makefile")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    assert NAME in declared and NAME in _lib.EXPORTS and NAME in _lib.SIGNATURES
    assert hasattr(L, NAME)
    assert re.search(r"pub fn %s\(" % NAME, ffi)
    assert not NAME.startswith("pqhip_adc_")
    assert "pqhip_flat_search_lists" in mk
    for text in (hdr, ffi, ctx):
        assert '"%s"' % OPTION in text
    fn = getattr(L, NAME)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert fn.restype is i32
    assert list(fn.argtypes) == [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i64, vp, i32, i64, vp, i32, i32,
                                 vp, i64, vp, i64, vp]
    # the C declaration has as many parameters, in the same widths
    proto = re.search(r"int32_t %s\((.*?)\);" % NAME, hdr, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    params = [p.strip() for p in proto.split(",")]
    assert len(params) == len(fn.argtypes)
    for p, t in zip(params, fn.argtypes):
        want = vp if "*" in p else i32 if p.startswith("int32_t") else i64
        assert t is want and (want is vp or p.startswith(("int32_t", "int64_t"))), p
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert ("the result of query q equals pqhip_flat_search_f32_dev on the same matrix with the mask of S_q, query by "
            "query, bit for bit") in flat
    assert "With every list probed once, in any order, the result equals the unmasked exhaustive call" in flat
    assert "No byte of a disallowed or unprobed row is loaded" in flat
    assert "in POSITION order" in flat


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    fn = getattr(L, NAME)
    assert fn(None, 0, p, 1, 4, p, 4, 2, 4, 4, p, 1, p, 1, 1, None, 0, 1, p, 1, p, 1, z) == _lib.EINVAL
    assert fn(None, 7, None, 0, 0, None, 3, 0, 0, 0, None, -1, None, 0, 0, None, 2, 0, None, 0, None, 0, z) == _lib.EINVAL
    assert fn(None, 0, p, 1, 4, p, 4, 2, 4, 4, p, 1, p, 1, 0, p, 1, 2000, p, 1, p, 1, z) == _lib.EINVAL


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
    off = torch.tensor([0, 10, 40])
    pr = torch.zeros(2, 2, dtype=torch.int64)
    w = torch.zeros(2, dtype=torch.int32)
    bad = [
        (dict(queries=q.double()), "queries must be float32"),
        (dict(queries=torch.zeros(1, 2, 6)), "queries must be float32"),
        (dict(vectors=x.to(torch.bfloat16)), "vectors must be float32 or float16"),
        (dict(vectors=x[0]), "vectors must be float32 or float16"),
        (dict(vectors=torch.zeros(40, 7)), "length mismatch"),
        (dict(queries=torch.zeros(2, 16385), vectors=torch.zeros(2, 16385)), "at most 16384 elements"),
        (dict(k=0), "k must be between 1 and 1024"),
        (dict(k=1025), "k must be between 1 and 1024"),
        (dict(list_off=off.int()), "int64 offsets"),
        (dict(list_off=off[None]), "int64 offsets"),
        (dict(list_off=off[:0]), "int64 offsets"),
        (dict(list_off=off.numpy()), "list_off must be a torch tensor"),
        (dict(probes=pr.int()), "probes must be int64"),
        (dict(probes=pr[None]), "probes must be int64"),
        (dict(probes=pr[:1]), "one probe row"),
        (dict(probes=pr[0]), "one probe row"),                       # one row for two queries
        (dict(probes=pr[:, :0]), "one probe row"),
        (dict(probes=pr.numpy()), "probes must be a torch tensor"),
        (dict(allow=w.long()), "int32 mask words"),
        (dict(allow=torch.zeros(40, dtype=torch.bool)), "int32 mask words"),
        (dict(allow=torch.zeros(3, dtype=torch.int32)), r"ceil\(n / 32\) words"),
        (dict(queries=q.numpy()), "must be a torch tensor"),
        (dict(vectors=x.numpy()), "must be a torch tensor"),
        (dict(), "must be CUDA tensors"),                  # everything else in order: host tensors stop here
        (dict(allow=w), "must be CUDA tensors"),
    ]
    for change, message in bad:
        args = dict(queries=q, vectors=x, list_off=off, probes=pr, k=3)
        args.update(change)
        with pytest.raises(PanicError, match=message):
            pq.flat_search_lists_device(**args)


def test_partitioned_flat_matrix_is_a_group_part_and_has_no_range_search():
    """class-level facts that need no device: the class shares the list layout of the partitioned classes, is accepted
    by MatrixGroup's type check and is refused by its range searches"""
    from reductive_amd import qmatrix
    cls = qmatrix.PartitionedFlatMatrix
    assert issubclass(cls, qmatrix._ListLayout) and issubclass(qmatrix._Lists, qmatrix._ListLayout)
    assert not issubclass(cls, qmatrix._Lists)
    assert cls._init_lists is qmatrix.PartitionedMatrix._init_lists           # the two layout routes are shared code
    assert cls.probes is qmatrix.PartitionedMatrix.probes and cls.assign is qmatrix.PartitionedMatrix.assign
    for name in ("nearest", "most_similar", "probes", "assign", "embeddings", "row_filter", "add", "compact", "remove"):
        assert callable(getattr(cls, name)), name
    assert callable(qmatrix.FlatMatrix.partition)
    assert qmatrix.MatrixGroup._more(object.__new__(cls), 5) == {"nprobe": 5}
