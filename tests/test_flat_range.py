"""CPU tests of the exact range searches over resident vectors (include/pqhip.h: pqhip_flat_range_f32_dev,
pqhip_flat_range_lists_f32_dev): the reference against the exact top-k reference, a numpy model of the kernel's schedule
(units, tiles, offering lanes) that must reproduce ascending row order, and the chunk arithmetic of the list driver pinned
to its source."""
import numpy as np
import pytest

import flat_range_ref as frr
import flat_search_ref as fr
import rerank_ref as rr


def _data(seed, n, d, nq, half):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float16 if half else np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return q, x


# ---- (a) the range is the passing part of the exact top-k over all rows ------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("ip", [False, True])
def test_range_reference_is_the_passing_part_of_the_full_search(ip, half):
    n, d, nq = 150, 70, 4
    q, x = _data(9100 + half, n, d, nq, half)
    x[17] = x[5]                                     # ties
    x[140] = x[5]
    x[3, 5] = np.nan
    x[4, 6] = np.inf
    x[6, 69] = -np.inf
    x[8] = q[1]                                      # distance 0 to query 1
    allow = np.random.default_rng(9102).random(n) < 0.7
    values = frr.all_values(q, x, ip)
    finite = np.sort(values[0][np.isfinite(values[0])])
    thr = np.array([finite[finite.size // 2], values[1, 17], np.inf if not ip else -np.inf, np.nan], np.float32)
    for mask in (None, allow):
        lims, val, idx = frr.ref_flat_range(q, x, thr, ip=ip, allow=mask)
        top_v, top_i = fr.ref_flat_search(q, x, n, ip=ip, allow=mask)
        for i in range(nq):
            with np.errstate(invalid="ignore"):
                ok = (top_i[i] >= 0) & ((top_v[i] >= thr[i]) if ip else (top_v[i] <= thr[i]))
            rows = top_i[i][ok]
            order = np.argsort(rows)
            got_i, got_v = idx[lims[i]:lims[i + 1]], val[lims[i]:lims[i + 1]]
            assert got_i.tolist() == rows[order].tolist()
            # the chains start at +0: no value is -0, so the search's canonical zero changes no bit
            assert got_v.view(np.uint32).tolist() == top_v[i][ok][order].view(np.uint32).tolist()
        assert lims[0] == 0 and lims[-1] == val.size == idx.size
        assert lims[4] == lims[3]                    # a NaN threshold matches nothing
        n_nan = int(np.isnan(values[2] if mask is None else values[2][mask]).sum())
        assert lims[3] - lims[2] == (n if mask is None else int(mask.sum())) - n_nan     # +-Inf: every non-NaN row


# ---- (b) the schedule: units, then tiles, then offering lanes ----------------------------------------------------------
def _model_range(query, x, thr, ip, wgs, allow=None):
    """One query of k_flat_range as the kernel walks it: workgroup b owns rows [b R, (b + 1) R), R a multiple of 1,024;
    its wave w the contiguous sub-range of R / 16 rows; a wave reduces tiles of 16 rows in ascending order
    (flat_search_ref.tile_reduce) and the lanes that hold a row offer it; hits are ranked by lane."""
    n = x.shape[0]
    p = fr.lane_partials(query, x, ip=ip)
    R = -(-(-(-n // wgs)) // 1024) * 1024
    grid = -(-n // R)
    sub = R // 16
    assert sub % 64 == 0
    out_v, out_i, counts = [], [], []
    for unit in range(grid * 16):
        b, w = divmod(unit, 16)
        lo = b * R + w * sub
        hi = min(lo + sub, (b + 1) * R, n)
        cnt = 0
        for row0 in range(lo, hi, 16):
            m = min(16, hi - row0)
            t = np.zeros((16, 64), np.float32)
            t[:m] = p[row0:row0 + m]
            if allow is not None:
                t[:m][~allow[row0:row0 + m]] = np.float32(123.0)      # a masked row is not loaded: junk, never offered
            v = fr.tile_reduce(t)
            hit = np.zeros(64, bool)
            for u in range(m):
                lane = fr.tile_lane_of_row(u)
                assert lane == 4 * u
                if allow is not None and not allow[row0 + u]:
                    continue
                with np.errstate(invalid="ignore"):
                    hit[lane] = v[lane] >= thr if ip else v[lane] <= thr
            for lane in np.flatnonzero(hit):                           # rank = the hit lanes below
                out_v.append(v[lane])
                out_i.append(row0 + (lane >> 2))
                cnt += 1
        counts.append(cnt)
    return np.array(out_v, np.float32), np.array(out_i, np.int64), counts


@pytest.mark.parametrize("n", [1, 16, 17, 64, 1025, 2100])
def test_schedule_model_gives_ascending_rows_for_every_grid(n):
    d = 70
    q, x = _data(9200 + n, n, d, 1, half=(n % 2 == 0))
    if n > 20:
        x[n // 2, 3] = np.nan
        x[n // 3] = x[0]
    allow = np.random.default_rng(9201).random(n) < 0.6
    for ip in (False, True):
        values = rr.row_values(q[0], x, ip=ip)
        thr = np.float32(np.nanmedian(values))
        for mask in (None, allow):
            want = frr.ref_flat_range(q, x, thr, ip=ip, allow=mask)
            for wgs in (1, 2, 3, 7):
                v, i, counts = _model_range(q[0], x, thr, ip, wgs, mask)
                assert i.tolist() == want[2].tolist(), (n, wgs)
                assert v.view(np.uint32).tolist() == want[1].view(np.uint32).tolist()
                assert sum(counts) == want[0][1]


# ---- (c) the chunks of the list driver ---------------------------------------------------------------------------------
def test_list_driver_chunk_expression_is_the_model():
    text = frr.src()
    c = frr.constants()
    assert c["scan_max"] == 1 << 20 and c["waves"] == 16 and c["queries"] == 4 and c["scratch"] == 512 << 20
    assert frr.lists_grid_cap() == 4096 and frr.grid_cap() == 16384
    for line in ("const int64_t units = G * kRangeWaves;",
                 "const size_t part_q = (size_t)units * sizeof(int64_t);",
                 "const int64_t bm_tiles = round_up(n_rows / kFlatTile + 65 * G + 1, 4);",
                 "const size_t bm_q = (size_t)bm_tiles * sizeof(uint16_t);",
                 "const size_t plan_q = ((size_t)std::max(n_probe, 1) * 2 + 1) * sizeof(int64_t);",
                 "const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, "
                 "(int64_t)(kListsScratchBytes / (plan_q + part_q + bm_q)),",
                 "kFlatRangeScanMax / units}));",
                 "for (int64_t q = 0; q < nq; q += chunk) {",
                 "const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);",
                 "d_probes + q * p_rs", "d_q + q * q_rs", "d_thr + q", "d_lims + q"):
        assert line in text, line


def test_list_driver_chunks():
    cap = frr.lists_grid_cap()
    # the forced cap: the scan bounds the chunk (2^20 / (4096 * 16) = 16 queries)
    assert frr.lists_chunk(1 << 40, 900, cap, 3) == 16
    assert frr.lists_chunk(1 << 40, 900, 10 * cap, 3) == 16
    assert frr.lists_chunk(37, 900, cap, 3) == 16              # 16 + 16 + 5: a third, shorter chunk
    assert frr.lists_chunk(5, 900, cap, 3) == 5
    # one workgroup per query: gridDim.y bounds it
    assert frr.lists_chunk(1 << 40, 900, 1, 3) == frr.GRID_Y
    # a large matrix: the bitmap (n / 8 bytes per query) bounds it through the scratch
    n = 10_000_000
    per_q = frr.lists_query_bytes(n, 8, 64)
    assert per_q == (64 * 2 + 1) * 8 + 8 * 16 * 8 + frr.bitmap_tiles(n, 8) * 2
    assert frr.lists_chunk(1 << 40, n, 8, 64) == (512 << 20) // per_q == 428
    assert frr.lists_chunk(1 << 40, (1 << 32) - 2, 1, 1) == 1   # never less than one query


def test_bitmap_has_a_slot_for_every_tile_of_n_places():
    for n in (1, 15, 16, 17, 900, 1023, 1024, 1025, 100_000, 10_000_000):
        for G in (1, 2, 5, 64, 4096):
            for total in {0, 1, n // 3, n - 1, n}:
                assert frr.used_tiles(total, G) <= frr.bitmap_tiles(n, G), (n, G, total)
