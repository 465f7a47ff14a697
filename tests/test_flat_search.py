"""CPU tests of the exact search over resident vectors (include/pqhip.h: pqhip_flat_search_f32_dev): pins
tests/flat_search_ref.py -- rerank_ref.ref_rerank over the allowed rows -- on ties, NaN / Inf / -0 rows, k beyond the
allowed rows and an all-zero mask; the numpy model of the kernel's tile reduction (the transposed butterfly) against
rerank_ref.row_values, bit for bit, for every tile size the kernel instantiates; header, EXPORTS, SIGNATURES, library and
rust/pqhip_ffi.rs name the entry point and its option; a null codebook is EINVAL; the argument checks of
Pq.flat_search_device raise before the library is reached."""
import ctypes
import os
import re

import numpy as np
import pytest

import flat_search_ref as fr
import rerank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_flat_search_f32_dev"


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
def test_reference_is_the_rerank_of_all_rows_and_of_the_allowed_rows(ip):
    q, x = _data(1, 200, 70, 3)
    v, i = fr.ref_flat_search(q, x, 20, ip=ip)
    wv, wi, flag = rr.ref_rerank(q, x, np.tile(np.arange(200), (3, 1)), 20, ip=ip)
    assert not flag
    rr.assert_same(v, i, wv, wi)
    # against a plain sort of the row values
    for qi in range(3):
        vals = rr.row_values(q[qi], x, ip=ip)
        order = np.lexsort((np.arange(200), -vals if ip else vals))[:20]
        assert i[qi].tolist() == order.tolist() and v[qi].tobytes() == vals[order].tobytes()
    allow = np.random.default_rng(2).random(200) < 0.3
    v, i = fr.ref_flat_search(q, x, 20, ip=ip, allow=allow)
    assert allow[i].all()
    wv, wi, _ = rr.ref_rerank(q, x, np.tile(np.flatnonzero(allow), (3, 1)), 20, ip=ip)
    rr.assert_same(v, i, wv, wi)


def test_reference_ties_go_to_the_smaller_row():
    q = np.zeros((1, 8), np.float32)
    x = np.ones((9, 8), np.float32)
    x[4] = 0.5
    x[7] = x[4]                                     # duplicate rows
    v, i = fr.ref_flat_search(q, x, 9)
    assert i.tolist() == [[4, 7, 0, 1, 2, 3, 5, 6, 8]]
    assert v[0, 0] == v[0, 1] == np.float32(2.0) and (v[0, 2:] == np.float32(8.0)).all()
    v, i = fr.ref_flat_search(q + 1, x, 3, ip=True)
    assert i.tolist() == [[0, 1, 2]] and (v == np.float32(8.0)).all()
    allow = np.ones(9, bool)
    allow[[0, 4]] = False
    v, i = fr.ref_flat_search(q, x, 3, allow=allow)
    assert i.tolist() == [[7, 1, 2]]


def test_reference_nan_inf_and_signed_zero_rows():
    q = np.ones((1, 4), np.float32)
    x = np.array([[1, 1, 1, 1],                      # L2 +0, IP 4
                  [np.nan, 1, 1, 1],                 # NaN: last in both
                  [np.inf, 1, 1, 1],                 # L2 +Inf, IP +Inf
                  [-np.inf, 1, 1, 1],                # L2 +Inf, IP -Inf
                  [0, 0, 0, 0],                      # IP +0
                  [-0.0, -0.0, -0.0, -0.0],          # IP: fl(+0 + -0) = +0, equal to row 4
                  [2, 2, 2, 2]], np.float32)
    v, i = fr.ref_flat_search(q, x, 7)
    assert i.tolist() == [[0, 4, 5, 6, 2, 3, 1]]
    assert v[0, :6].tolist() == [0, 4, 4, 4, np.inf, np.inf] and np.isnan(v[0, 6])
    v, i = fr.ref_flat_search(q, x, 7, ip=True)
    assert i.tolist() == [[2, 6, 0, 4, 5, 3, 1]]
    assert v[0, :6].tolist() == [np.inf, 8, 4, 0, 0, -np.inf] and np.isnan(v[0, 6])
    assert not np.signbit(v[0, 3:5]).any()           # a zero comes back as +0
    # a NaN or Inf in a disallowed row changes nothing
    allow = np.array([1, 0, 0, 0, 1, 1, 1], bool)
    v, i = fr.ref_flat_search(q, x, 5, allow=allow)
    assert i.tolist() == [[0, 4, 5, 6, -1]] and v[0, 4] == np.inf


def test_reference_pads_beyond_the_allowed_rows_and_for_an_all_zero_mask():
    q, x = _data(3, 12, 5, 2)
    v, i = fr.ref_flat_search(q, x, 15)
    assert (i[:, :12] >= 0).all() and (i[:, 12:] == -1).all() and (v[:, 12:] == np.inf).all()
    v, i = fr.ref_flat_search(q, x, 4, ip=True, allow=np.zeros(12, bool))
    assert (i == -1).all() and (v == -np.inf).all()
    v, i = fr.ref_flat_search(q, x[:0], 4)
    assert (i == -1).all() and (v == np.inf).all()
    allow = np.zeros(12, bool)
    allow[[3, 9]] = True
    v, i = fr.ref_flat_search(q, x, 4, allow=allow)
    assert sorted(i[0, :2].tolist()) == [3, 9] and i[0, 2:].tolist() == [-1, -1]


def test_mask_words_round_trip_and_ignore_bits_beyond_n():
    rng = np.random.default_rng(4)
    for n in (0, 1, 31, 32, 33, 70, 1025):
        allow = rng.random(n) < 0.5
        w = fr.mask_words(allow)
        assert w.dtype == np.int32 and w.shape == (-(-n // 32),)
        assert np.array_equal(fr.words_allow(w, n), allow)
        for r in range(n):
            assert bool((int(w.view(np.uint32)[r >> 5]) >> (r & 31)) & 1) == bool(allow[r])
        if n % 32:
            junk = w.copy()
            junk.view(np.uint32)[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
            assert np.array_equal(fr.words_allow(junk, n), allow)


# ---- the kernel's reduction schedule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", fr.TILES)
@pytest.mark.parametrize("ip", [False, True])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 300, 768])
def test_tile_reduction_model_equals_the_tree_bit_for_bit(d, ip, tile):
    """The transposed butterfly pairs (l, l + s) exactly as the tree does and f32 addition commutes: every row's value is
    the tree's, whatever its place in the tile, and all lanes of a row's group hold it."""
    q, x = _data(100 + d, 3 * tile + 5, d, 2)
    x[3] *= np.float32(1e20)                          # rows of very different magnitude side by side in one tile
    x[4] *= np.float32(1e-20)
    for qi in range(2):
        want = rr.row_values(q[qi], x, ip=ip)
        got = fr.model_row_values(q[qi], x, ip=ip, tile=tile)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("tile", fr.TILES)
def test_tile_reduction_model_on_the_order_sensitive_case(tile):
    """the case of test_rerank.test_summation_order_is_lane_chains_then_the_tree, in every place of the tile"""
    d = 130
    q = np.ones(d, np.float32)
    row = np.zeros(d, np.float32)
    row[0], row[64], row[128] = 2.0 ** 24, 1.0, 1.0
    row[32] = -2.0 ** 24
    row[1] = 3.0
    assert rr.row_values(q, row[None], ip=True)[0] == np.float32(3.0)
    rng = np.random.default_rng(5)
    for u in range(tile):
        x = rng.standard_normal((tile, d)).astype(np.float32)
        x[u] = row
        got = fr.model_row_values(q, x, ip=True, tile=tile)
        assert got[u] == np.float32(3.0)
        assert got.tobytes() == rr.row_values(q, x, ip=True).tobytes()


@pytest.mark.parametrize("tile", fr.TILES)
def test_tile_reduction_model_steps(tile):
    """which lane keeps, sends and adds what: after the step at s, the lanes with bit s clear hold register u's pair sums
    and the others those of register u + half; the row of a lane at the end is lane // (64 / tile)"""
    p = np.arange(tile * 64, dtype=np.float32).reshape(tile, 64)        # small integers: every sum exact
    out = fr.tile_reduce(p, tile)
    group = 64 // tile
    for lane in range(64):
        assert out[lane] == p[lane // group].sum()
    a, b = p[0], p[tile // 2]
    f = fr._fold(a, b, 32)
    assert np.array_equal(f[:32], a[:32] + a[32:]) and np.array_equal(f[32:], b[:32] + b[32:])
    f = fr._fold(a, b, 4)
    lane = np.arange(64)
    lo = (lane & 4) == 0
    assert np.array_equal(f[lo], a[lo] + a[lane[lo] + 4]) and np.array_equal(f[~lo], b[~lo] + b[lane[~lo] - 4])
    src = open(os.path.join(ROOT, "reductive_amd", "csrc", "kernels_flat_search.hip.h")).read()
    assert [int(t) for t in re.findall(r"constexpr int kFlatTile = (\d+);", src)] == list(fr.TILES)


# ---- the declarations ------------------------------------------------------------------------------------------------------
def test_header_exports_library_and_ffi_name_the_entry_point(ra):
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", hdr))
    from reductive_amd import _lib
    L = ra.lib()
    assert NAME in declared and NAME in _lib.EXPORTS and NAME in _lib.SIGNATURES
    assert hasattr(L, NAME)
    assert re.search(r"pub fn %s\(" % NAME, ffi)
    fn = getattr(L, NAME)
    assert len(fn.argtypes) == 18 and fn.argtypes[6] is ctypes.c_int32 and fn.argtypes[-1] is ctypes.c_void_p
    assert not NAME.startswith(("pqhip_adc_search", "pqhip_adc_range"))
    assert '"flat_search_wgs"' in hdr and '"flat_search_wgs"' in ffi
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr))
    assert "for n_rows <= 1024 the call equals pqhip_rerank_f32_dev with the candidate list 0 .. n_rows - 1" in flat
    assert "the result does not depend on the number of workgroups, on the rows each takes or on how many queries share a pass" in flat
    assert "A row whose bit is clear enters nothing and none of its bytes is loaded" in flat


def test_null_codebook_is_einval(ra):
    from reductive_amd import _lib
    L = ra.lib()
    z = ctypes.c_void_p(0)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)
    fn = getattr(L, NAME)
    assert fn(None, 0, p, 1, 4, p, 4, 2, 4, 4, None, 0, 1, p, 1, p, 1, z) == _lib.EINVAL
    assert fn(None, 7, None, 0, 0, None, 3, 0, 0, 0, None, 2, 0, None, 0, None, 0, z) == _lib.EINVAL
    assert fn(None, 0, p, 1, 4, p, 4, 2, 4, 4, p, 1, 2000, p, 1, p, 1, z) == _lib.EINVAL


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
    w = torch.zeros(2, dtype=torch.int32)
    bad = [
        (dict(queries=q.double()), "queries must be float32"),
        (dict(queries=torch.zeros(1, 2, 6)), "queries must be float32"),
        (dict(vectors=x.to(torch.bfloat16)), "vectors must be float32 or float16"),
        (dict(vectors=x[0]), "vectors must be float32 or float16"),
        (dict(vectors=torch.zeros(40, 7)), "length mismatch"),
        (dict(queries=torch.zeros(1, 16385), vectors=torch.zeros(2, 16385)), "at most 16384 elements"),
        (dict(k=0), "k must be between 1 and 1024"),
        (dict(k=1025), "k must be between 1 and 1024"),
        (dict(allow=w.long()), "int32 mask words"),
        (dict(allow=torch.zeros(40, dtype=torch.bool)), "int32 mask words"),
        (dict(allow=w[None]), "int32 mask words"),
        (dict(allow=torch.zeros(3, dtype=torch.int32)), r"ceil\(n / 32\) words"),
        (dict(allow=torch.zeros(1, dtype=torch.int32)), r"ceil\(n / 32\) words"),
        (dict(queries=q.numpy()), "must be a torch tensor"),
        (dict(vectors=x.numpy()), "must be a torch tensor"),
        (dict(), "must be CUDA tensors"),                  # everything else in order: host tensors stop here
        (dict(allow=w), "must be CUDA tensors"),
    ]
    for change, message in bad:
        args = dict(queries=q, vectors=x, k=3)
        args.update(change)
        with pytest.raises(PanicError, match=message):
            pq.flat_search_device(**args)


def test_exact_search_without_vectors_raises_before_any_search():
    from reductive_amd.pq import PanicError
    from reductive_amd.qmatrix import _Refine

    class Stub(_Refine):
        pass
    m = Stub()
    for fn in (m.exact_nearest, m.exact_most_similar):
        with pytest.raises(PanicError, match="call attach_vectors first"):
            fn(None, 10)
