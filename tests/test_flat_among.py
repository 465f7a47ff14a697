"""CPU tests of the exact searches among given rows (include/pqhip.h: pqhip_flat_among_f32_dev,
pqhip_flat_range_among_f32_dev): pins tests/flat_among_ref.py against the exact references that exist already
(flat_search_ref.ref_flat_search under the mask of the candidates, rerank_ref.ref_rerank, flat_range_ref.ref_flat_range)
on ties, NaN / +-Inf / -0, k beyond the candidates, empty and all-padding lists, duplicates and permutations; header,
EXPORTS, SIGNATURES, library and rust/pqhip_ffi.rs name the entry points and their options; a null codebook is EINVAL;
the wrappers and the class methods refuse CPU tensors and bad `rows` before the library is reached; and the chunk
arithmetic of the two drivers is pinned to the source, with the two cases the GPU test drives into a third launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import flat_among_ref as far
import flat_range_ref as frr
import flat_search_ref as fr
import rerank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_flat_among_f32_dev", "pqhip_flat_range_among_f32_dev")


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def _data(seed, n, d, nq, half=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float16 if half else np.float32)
    return rng.standard_normal((nq, d)).astype(np.float32), x


def _special(q, x):
    """ties, NaN, +-Inf and a distance of exactly zero among the rows"""
    x[17] = x[5]
    x[140] = x[5]
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1]
    x[9] = 0                                          # inner product -0 / +0 with a query of mixed signs
    return x


def _ragged(seed, nq, n, lengths):
    rng = np.random.default_rng(seed)
    parts = [rng.permutation(n)[:m].astype(np.int64) for m in lengths]
    lims = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return lims, np.concatenate(parts) if parts else np.zeros(0, np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_topk_reference_is_the_flat_search_under_the_mask_of_the_candidates(ip, half):
    n, d, nq = 150, 70, 4
    q, x = _data(9100 + half, n, d, nq, half)
    x = _special(q, x)
    lims, ids = _ragged(9101, nq, n, (60, 0, 150, 17))
    ids[lims[2]:lims[3]][::7] = -1                    # padding inside a list
    values = frr.all_values(q, x, ip)
    for k in (1, 10, 64, 200):                        # 200 > every |C_q|
        v, i, flagged = far.ref_flat_among(q, x, ids, k, lims=lims, ip=ip, values=values)
        assert not flagged
        for j in range(nq):
            mine = ids[lims[j]:lims[j + 1]]
            allow = np.zeros(n, bool)
            allow[mine[mine >= 0]] = True
            wv, wi = fr.ref_flat_search(q[j], x, k, ip=ip, allow=allow)
            assert i[j].tolist() == wi[0].tolist()
            rr.assert_same(v[j:j + 1], i[j:j + 1], wv, wi)
            assert bits(np.nan_to_num(v[j], nan=7.0)) == bits(np.nan_to_num(wv[0], nan=7.0))
            m = min(k, int(allow.sum()))
            assert (i[j, m:] == -1).all() and (v[j, m:] == (-np.inf if ip else np.inf)).all()
    assert (far.ref_flat_among(q, x, ids, 5, lims=lims, ip=ip, values=values)[1][1] == -1).all()    # the empty list


@pytest.mark.parametrize("ip", [False, True])
def test_topk_reference_is_the_rerank_reference_and_ignores_the_order_of_the_ids(ip):
    n, d, nq = 150, 70, 3
    q, x = _data(9110, n, d, nq)
    x = _special(q, x)
    rng = np.random.default_rng(9111)
    ids = rng.permutation(n)[:90].astype(np.int64)
    ids[::11] = -1
    values = frr.all_values(q, x, ip)
    for k in (1, 33, 128):
        v, i, flagged = far.ref_flat_among(q, x, ids, k, ip=ip, values=values)
        wv, wi, wflag = rr.ref_rerank(q, x, np.broadcast_to(ids, (nq, ids.size)), k, ip=ip)
        assert not flagged and not wflag
        assert i.tolist() == wi.tolist() and bits(np.nan_to_num(v, nan=7.0)) == bits(np.nan_to_num(wv, nan=7.0))
        pv, pi, _ = far.ref_flat_among(q, x, rng.permutation(ids), k, ip=ip, values=values)
        assert pi.tolist() == i.tolist() and bits(np.nan_to_num(pv, nan=7.0)) == bits(np.nan_to_num(v, nan=7.0))
    # a row named twice may come back twice; all-padding and empty lists give the padding
    v, i, _ = far.ref_flat_among(q, x, np.array([5, 5, 17, -1], np.int64), 4, ip=ip, values=values)
    assert sorted(i[0].tolist()) == [-1, 5, 5, 17]
    for empty in (np.zeros(0, np.int64), np.full(9, -1, np.int64)):
        v, i, flagged = far.ref_flat_among(q, x, empty, 3, ip=ip, values=values)
        assert (i == -1).all() and (v == (-np.inf if ip else np.inf)).all() and not flagged


def test_zero_values_come_back_as_plus_zero_and_nan_rows_last():
    q = np.array([[1.0, -1.0, 0.0]], np.float32)
    x = np.array([[0, 0, 0], [1, 1, 0], [np.nan, 0, 0], [-1, 1, 5]], np.float32)
    v, i, _ = far.ref_flat_among(q, x, np.array([2, 3, 1, 0], np.int64), 4, ip=True)
    assert i[0].tolist() == [0, 1, 3, 2] and bits(v[0][:2]) == [0, 0] and np.isnan(v[0][3])
    lims, val, idx, _ = far.ref_flat_range_among(q, x, np.array([2, 3, 1, 0], np.int64), 0.0, ip=True)
    assert idx.tolist() == [1, 0] and lims.tolist() == [0, 2]            # as named; NaN never qualifies; -2 < 0


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_range_reference_against_the_exhaustive_range_reference(ip, half):
    n, d, nq = 150, 70, 4
    q, x = _data(9120 + half, n, d, nq, half)
    x = _special(q, x)
    values = frr.all_values(q, x, ip)
    finite = np.sort(values[0][np.isfinite(values[0])])
    thr = np.array([finite[finite.size // 2], values[1, 17], -np.inf if ip else np.inf, np.nan], np.float32)
    # every row, shared: the unmasked exhaustive range
    got = far.ref_flat_range_among(q, x, np.arange(n, dtype=np.int64), thr, ip=ip, values=values)
    want = frr.ref_flat_range(q, x, thr, ip=ip, values=values)
    assert not got[3] and got[0].tolist() == want[0].tolist() and got[2].tolist() == want[2].tolist()
    assert bits(got[1]) == bits(want[1])
    assert got[0][4] == got[0][3]                     # a NaN threshold matches nothing
    # ascending subsets per query: the masked call with the mask of C_q
    rng = np.random.default_rng(9121)
    subsets = [np.sort(rng.permutation(n)[:m]).astype(np.int64) for m in (40, 0, 150, 16)]
    lims = np.concatenate([[0], np.cumsum([s.size for s in subsets])]).astype(np.int64)
    ids = np.concatenate(subsets)
    got = far.ref_flat_range_among(q, x, ids, thr, lims=lims, ip=ip, values=values)
    for j in range(nq):
        allow = np.zeros(n, bool)
        allow[subsets[j]] = True
        w = frr.ref_flat_range(q[j:j + 1], x, thr[j], ip=ip, allow=allow, values=values[j:j + 1])
        assert got[2][got[0][j]:got[0][j + 1]].tolist() == w[2].tolist()
        assert bits(got[1][got[0][j]:got[0][j + 1]]) == bits(w[1])
    # permuted and duplicated ids: the sub-sequence of the places, in the order named
    ids = np.array([9, 140, 5, -1, 17, 5, 9, 3, 4], np.int64)
    got = far.ref_flat_range_among(q[2:3], x, ids, thr[2], ip=ip, values=values[2:3])
    keep = [r for r in ids.tolist() if r >= 0 and not np.isnan(values[2, r])]
    assert got[2].tolist() == keep and got[0].tolist() == [0, len(keep)]
    # the (lims, idx) of a range at a wider threshold fed back at the narrow one: the narrow range itself
    wide = frr.ref_flat_range(q, x, np.where(np.isfinite(thr), thr - 40 if ip else thr + 40, thr), ip=ip, values=values)
    back = far.ref_flat_range_among(q, x, wide[2], thr, lims=wide[0], ip=ip, values=values)
    assert back[0].tolist() == want[0].tolist() and back[2].tolist() == want[2].tolist() and bits(back[1]) == bits(want[1])


def test_reference_flags_bad_ids_and_lims_and_clamps():
    q, x = _data(9130, 20, 5, 3)
    ids = np.arange(12, dtype=np.int64)
    for bad in (-2, 20, 1 << 62):
        b = ids.copy()
        b[4] = bad
        v, i, flagged = far.ref_flat_among(q, x, b, 20)
        assert flagged and sorted(i[0][i[0] >= 0].tolist()) == [r for r in range(12) if r != 4]
        assert far.ref_flat_range_among(q, x, b, np.inf)[3]
    b = ids.copy()
    b[4] = -1
    assert not far.ref_flat_among(q, x, b, 20)[2]
    for lims, sizes in (([-3, 4, 12, 12], [4, 8, 0]), ([0, 4, 40, 12], [4, 8, 0]), ([0, 8, 4, 12], [8, 0, 8]),
                        ([0, 30, 35, 12], [12, 0, 0])):
        v, i, flagged = far.ref_flat_among(q, x, ids, 20, lims=np.array(lims, np.int64))
        assert flagged and [(r >= 0).sum() for r in i] == sizes, lims
        got = far.ref_flat_range_among(q, x, ids, np.inf, lims=np.array(lims, np.int64))
        assert got[3] and np.diff(got[0]).tolist() == sizes
    assert not far.ref_flat_among(q, x, ids, 20, lims=np.array([0, 4, 4, 12], np.int64))[2]
    # no rows at all: every id other than -1 flags
    empty = np.zeros((0, 5), np.float32)
    assert far.ref_flat_among(q, empty, np.array([0], np.int64), 2)[2]
    assert not far.ref_flat_among(q, empty, np.array([-1], np.int64), 2)[2]


# ---- the declarations ------------------------------------------------------------------------------------------------------
def test_header_exports_library_and_ffi_name_the_entry_points(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    ctx = open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    mk = open(os.path.join(ROOT, "reductive_amd", "csrc", "Makefile")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    head = [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, vp, i64, i32]
    tails = {NAMES[0]: [i32, vp, i64, vp, i64, vp], NAMES[1]: [vp, vp, vp, vp, i64, vp]}
    assert "pqhip_flat_among" in mk
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert re.search(r"pub fn %s\(" % name, ffi)
        fn = getattr(L, name)
        assert fn.restype is i32 and list(fn.argtypes) == head + tails[name]
        proto = re.search(r"int32_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        params = [p.strip() for p in proto.split(",")]
        assert len(params) == len(fn.argtypes)
        for p, t in zip(params, fn.argtypes):
            want = vp if "*" in p else i32 if p.startswith("int32_t") else i64
            assert t is want and (want is vp or p.startswith(("int32_t", "int64_t"))), p
        rust = re.search(r"pub fn %s\((.*?)\) -> i32;" % name, ffi, re.S).group(1)
        assert len(rust.split(",")) == len(fn.argtypes)
    for option in (far.OPTION, far.OPTION_RANGE):
        for text in (hdr, ffi, ctx):
            assert '"%s"' % option in text
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    for sentence in ("Candidates: exactly those of pqhip_adc_among_f32_dev",
                     "Value of a row: exactly that of pqhip_rerank_f32_dev, operation for operation",
                     "are exactly those of pqhip_flat_search_f32_dev",
                     "The predicate is exactly that of pqhip_flat_range_f32_dev",
                     "IN THE ORDER IN WHICH THEY WERE NAMED",
                     "The capacity protocol is exactly that of the other range calls",
                     "no address is formed for it",
                     "Anything not served is PQHIP_EUNSUPPORTED, never another path"):
        assert sentence in flat, sentence


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    topk, rng = (getattr(L, n) for n in NAMES)
    assert topk(None, 0, p, 1, 4, p, 4, 2, 4, 4, None, p, 1, 0, 1, p, 1, p, 1, z) == _lib.EINVAL
    assert topk(None, 7, None, 0, 0, None, 3, 0, 0, 0, None, None, -1, 2, 2000, None, 0, None, 0, z) == _lib.EINVAL
    assert rng(None, 0, p, 1, 4, p, 4, 2, 4, 4, None, p, 1, 0, p, p, p, p, 1, z) == _lib.EINVAL
    assert rng(None, 7, None, 0, 0, None, 3, 0, 0, 0, None, None, -1, 2, None, None, None, None, -1, z) == _lib.EINVAL


# ---- the wrappers ----------------------------------------------------------------------------------------------------------
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
    ids = torch.arange(9)
    lims = torch.tensor([0, 4, 9])
    bad = [
        (dict(queries=q.double()), "queries must be float32"),
        (dict(queries=torch.zeros(1, 2, 6)), "queries must be float32"),
        (dict(vectors=x.to(torch.bfloat16)), "vectors must be float32 or float16"),
        (dict(vectors=x[0]), "vectors must be float32 or float16"),
        (dict(vectors=torch.zeros(40, 7)), "length mismatch"),
        (dict(queries=torch.zeros(2, 16385), vectors=torch.zeros(2, 16385)), "at most 16384 elements"),
        (dict(ids=ids.int()), "candidate ids must be one contiguous int64 vector"),
        (dict(ids=ids[None]), "candidate ids must be one contiguous int64 vector"),
        (dict(ids=torch.arange(18)[::2]), "candidate ids must be one contiguous int64 vector"),
        (dict(ids=ids.numpy()), "candidate ids must be one contiguous int64 vector"),
        (dict(lims=lims.int()), "lims must be a contiguous int64 vector"),
        (dict(lims=lims[:2]), "one offset per query and the end"),
        (dict(queries=q.numpy()), "must be a torch tensor"),
        (dict(vectors=x.numpy()), "must be a torch tensor"),
        (dict(), "expects CUDA tensors on one device"),    # everything else in order: host tensors stop here
        (dict(lims=lims), "expects CUDA tensors on one device"),
    ]
    for change, message in bad:
        args = dict(queries=q, vectors=x, ids=ids)
        args.update(change)
        with pytest.raises(PanicError, match=message):
            pq.flat_among_device(k=3, **args)
        with pytest.raises(PanicError, match=message):
            pq.flat_range_among_device(threshold=1.0, **args)


def test_class_methods_exist_and_refuse_bad_rows():
    from reductive_amd import qmatrix
    from reductive_amd.pq import PanicError
    names = ("exact_nearest_among", "exact_most_similar_among", "exact_within_among", "exact_similar_above_among")
    for cls in (qmatrix.QuantizedMatrix, qmatrix.PartitionedMatrix, qmatrix.ResidualPartitionedMatrix):
        for name in names:
            assert getattr(cls, name) is getattr(qmatrix._Refine, name), (cls, name)
    for cls in (qmatrix.FlatMatrix, qmatrix.PartitionedFlatMatrix):
        for name in ("nearest_among", "most_similar_among", "within_among", "similar_above_among"):
            assert callable(getattr(cls, name)), (cls, name)
    assert "m.exact_within_among(q, m.within(q, r + slack)[::2], r)" in qmatrix._Refine.exact_within_among.__doc__
    assert "POSITION" in qmatrix.PartitionedFlatMatrix.nearest_among.__doc__
    # the vectors are asked for first; then `rows` is parsed by nearest_among's helper, on the host
    m = object.__new__(qmatrix.QuantizedMatrix)
    with pytest.raises(PanicError, match="call attach_vectors first"):
        m.exact_within_among(np.zeros(3, np.float32), np.arange(3), 1.0)
    import torch
    flat = object.__new__(qmatrix.FlatMatrix)
    flat.vectors = torch.zeros(4, 3)
    for rows, message in ((np.zeros(3), "rows must be integers"), (np.zeros((2, 2), np.int64), "vector of integers"),
                          ((np.arange(2), np.arange(3), np.arange(3)), "the pair"), (torch.zeros(3), "vector of integers"),
                          ((np.zeros(2), np.arange(3)), "lims must be integers")):
        for call in (lambda r: flat.nearest_among(np.zeros(3, np.float32), r, 2),
                     lambda r: flat.similar_above_among(np.zeros(3, np.float32), r, 0.5),
                     lambda r: flat.exact_within_among(np.zeros(3, np.float32), r, 0.5)):
            with pytest.raises(PanicError, match=message):
                call(rows)


# ---- the chunks of the two drivers -----------------------------------------------------------------------------------------
def test_driver_chunk_expressions_are_the_model():
    text = far.src()
    c = far.constants()
    assert c["scan_max"] == 1 << 20 and c["waves"] == 16 and c["scratch"] == 512 << 20
    assert far.grid_caps() == (4096, 4096)
    for line in ("const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));",
                 "const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, "
                 "(int64_t)(kListsScratchBytes / lists_q)}));",
                 "const int64_t units = G * kRangeWaves;",
                 "const size_t part_q = (size_t)units * sizeof(int64_t);",
                 "const int64_t mean = d_lims ? n_ids / nq : n_ids;",
                 "const int64_t span = d_lims ? std::min<int64_t>(n_ids, 4 * mean + 1024) : n_ids;",
                 "const int64_t bm_tiles = round_up(span / kFlatTile + 65 * G + 1, 4);",
                 "const size_t bm_q = (size_t)bm_tiles * sizeof(uint16_t);",
                 "(int64_t)(kListsScratchBytes / (part_q + bm_q)),",
                 "kFlatAmongScanMax / units}));",
                 "for (int64_t q = 0; q < nq; q += chunk) {",
                 "const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);",
                 "d_q + q * q_rs", "d_lims ? d_lims + q : nullptr", "d_thr + q", "d_out_lims + q",
                 "d_val + q * v_rs", "d_idx + q * i_rs"):
        assert line in text, line


def test_the_gpu_chunk_cases_need_three_launches():
    """what tests/test_gpu_flat_among.py drives: the grid options at their cap"""
    cap_t, cap_r = far.grid_caps()
    # top-k, k = 1,024: 4,096 x 64 x 16 entries of 12 bytes per query leave 10 queries to 512 MB -> 25 = 10 + 10 + 5
    assert far.topk_chunk(1 << 40, cap_t, 1024) == 10 and far.topk_chunk(1 << 40, 10 * cap_t, 1024) == 10
    assert far.topk_chunk(25, cap_t, 1024) == 10 and -(-25 // 10) == 3 and 25 % 10 == 5
    assert far.topk_chunk(25, cap_t, 10) == 25                     # a small k: one launch
    # range: one scan sums 2^20 counts = 16 queries of 4,096 x 16 units -> 37 = 16 + 16 + 5
    for shared in (False, True):
        assert far.range_chunk(1 << 40, 37 * 40, cap_r, shared) == 16
        assert far.range_chunk(37, 37 * 40, cap_r, shared) == 16 and -(-37 // 16) == 3 and 37 % 16 == 5
    assert far.range_chunk(1 << 40, 1000, 1, True) == far.GRID_Y
    # a long shared list: the bitmap (n_ids / 8 bytes per query) bounds the chunk through the scratch
    per_q = 8 * 16 * 8 + far.bitmap_tiles(100_000_000, 8) * 2
    assert far.range_chunk(1 << 40, 100_000_000, 8, True) == (512 << 20) // per_q == 42
    # per-query lists: the bitmap follows the mean range, and a longer range falls back to tiles without a mask
    assert far.bitmap_span(64, 64_000_000, False) == 4 * 1_000_000 + 1024
    assert far.bitmap_span(1, 500, False) == 500


def test_bitmap_has_a_slot_for_every_tile_of_span_places():
    for span in (1, 15, 16, 17, 900, 1023, 1024, 1025, 100_000):
        for G in (1, 2, 5, 64, 4096):
            for total in {0, 1, span // 3, span - 1, span}:
                assert frr.used_tiles(total, G) <= far.bitmap_tiles(span, G), (span, G, total)
