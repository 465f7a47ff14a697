"""The planner of the ADC top-k searches (tests/adc_search_cells.py) on the CPU: the calls that
test_gpu_adc_search_grid.py makes cover every instantiation the launchers name, the value lists the planner mirrors
still stand literally in the sources, and option "adc_search_wgs" is wired where its siblings are."""
import os
import re

import adc_search_cells as cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reductive_amd", "csrc")


def src(name, base=CSRC):
    with open(os.path.join(base, name)) as f:
        return f.read()


def lst(values, last=None):
    """'1, 2, 4' -- with the last value written as the constant the sources use"""
    v = [str(x) for x in values]
    if last:
        v[-1] = last
    return ", ".join(v)


def test_declared_cell_counts():
    by = {}
    for c in cells.declared_cells():
        by[c.family] = by.get(c.family, 0) + 1
    assert len(cells.NQ_L_PAIRS) == 10
    assert by == {"u8": 2 * 2 * 6 * 10, "u8_lists": 2 * 2 * 2 * 4 * 5, "p4": 2 * 2 * 5 * 10, "p4_lists": 2 * 2 * 2 * 3 * 5,
                  "any_u8": 2 * 5 * 2, "any_u32": 2 * 5 * 2, "merge": 2 * 5}


def test_grid_calls_cover_every_declared_cell():
    """No instantiation is left out, and the planner never plans a cell that is not declared.  A cell that no call of
    the C API can reach would be a dead instantiation: none was found (e.g. 8 queries per pass at 25 dwords is reached
    with M = 53 and K <= 77: 8 * 53 * 77 * 4 + 32,768 <= 163,840)."""
    declared = cells.declared_cells()
    reached = set()
    for call in cells.all_grid_calls():
        p = cells.plan(call)
        assert p is not None, call
        assert set(p.cells) <= declared, (call, set(p.cells) - declared)
        assert sum(cnt for name, cnt in p.log if "merge" in name) == p.cells[[c for c in p.cells if c.family == "merge"][0]]
        reached |= set(p.cells)
    missing = sorted(declared - reached)
    assert not missing, "%d cells no grid call reaches, e.g. %s" % (len(missing), missing[:5])


def test_passes_of_the_grid_queries():
    """nq = 13: 8 + 4 + 1 at L <= 2, 4 + 4 + 4 + 1 at L = 4, 13 x 1 beyond; one table per pass when only one fits"""
    small = 3 * 16 * 4
    assert cells.passes(13, 1, small, True) == [(8, 1), (4, 1), (1, 1)]
    assert cells.passes(13, 2, small, True) == [(8, 1), (4, 1), (1, 1)]
    assert cells.passes(13, 4, small, True) == [(4, 3), (1, 1)]
    assert cells.passes(13, 8, small, True) == [(1, 13)]
    assert cells.passes(13, 1, small, False) == [(1, 13)]
    assert cells.passes(5, 1, small, True) == [(4, 1), (1, 1)]
    assert cells.passes(13, 1, 100 * 256 * 4, True) == [(1, 13)]            # one table of 100 KB
    assert cells.passes(13, 1, 15 * 256 * 4, True) == [(8, 1), (4, 1), (1, 1)]
    assert cells.passes(13, 1, 33 * 256 * 4, True) == [(4, 3), (1, 1)]      # 8 tables of 33 KB do not fit, 4 do
    assert cells.passes(13, 1, 53 * 77 * 4, True)[0] == (8, 1) and cells.passes(13, 1, 53 * 78 * 4, True)[0] == (4, 3)


def test_plan_names_and_log():
    C = cells.Call
    p = cells.plan(C("u8", False, False, False, False, 15, 256, 10, 13, 1, 0, 0))
    assert cells.log_text(p.log) == ("k_adc_search_u8_mq<8 queries> + k_adc_search_merge x3 + "
                                     "k_adc_search_u8_mq<4 queries> + k_adc_search_u8")
    p = cells.plan(C("u8", False, True, True, False, 15, 256, 1024, 2, 1, 0, 0))
    assert cells.log_text(p.log) == "k_adc_ip_search_masked_u8 x2 + k_adc_ip_search_merge x2"
    p = cells.plan(C("p4", True, True, True, True, 17, 13, 100, 13, 1, 10, 2))
    assert cells.log_text(p.log) == "k_adc_lists_plan + k_adc_ip_search_lists_residual_p4 + k_adc_ip_search_merge"
    assert list(p.cells) == [cells.Cell("p4_lists", True, True, True, 8, 1, 2, None), cells.Cell("merge", True, False, False, 0, 0, 2, None)]
    p = cells.plan(C("u8", True, False, True, True, 17, 13, 100, 13, 1, 10, 2))
    assert cells.log_text(p.log) == "k_adc_lists_plan + k_adc_search_lists_residual_masked_u8 + k_adc_search_merge"
    p = cells.plan(C("u8", False, False, False, False, 15, 4096, 64, 3, 4, 0, 0))
    assert cells.log_text(p.log) == "k_adc_search_any x3 + k_adc_search_merge x3"
    p = cells.plan(C("u8", False, True, False, False, 101, 4, 64, 1, 1, 0, 0))
    assert cells.log_text(p.log) == "k_adc_ip_search_wide + k_adc_ip_search_merge"
    # what the library does not serve
    assert cells.plan(C("u8", False, False, True, False, 101, 4, 64, 1, 1, 0, 0)) is None      # a mask: the u8 route or nothing
    assert cells.plan(C("u8", True, False, False, False, 101, 4, 64, 1, 1, 1, 1)) is None
    assert cells.plan(C("p4", False, False, False, False, 5, 17, 64, 1, 1, 0, 0)) is None
    assert cells.plan(C("p4", False, False, False, False, 101, 16, 64, 1, 1, 0, 0)) is None
    assert cells.plan(C("u8", False, False, False, False, 5, 16, 1025, 1, 1, 0, 0)) is None


def test_buckets():
    assert [cells.search_nv_bucket(cells.u8_words(M)) for M in cells.U8_MS] == [1, 1, 2, 2, 4, 4, 8, 8, 13, 13, 25, 25]
    assert [cells.lists_nv_bucket(cells.u8_words(M)) for M in cells.U8_MS] == [4, 4, 4, 4, 4, 4, 8, 8, 13, 13, 25, 25]
    assert [cells.packed4_nv_bucket(cells.packed4_words(M)) for M in cells.P4_MS] == [1, 1, 2, 2, 4, 4, 8, 8, 13, 13]
    assert [cells.packed4_lists_nv_bucket(cells.packed4_words(M)) for M in cells.P4_MS] == [2, 2, 2, 2, 8, 8, 8, 8, 13, 13]
    assert cells.search_nv_bucket(26) == 0 and cells.packed4_nv_bucket(14) == 0
    assert [cells.search_list_regs(k) for k in cells.GRID_KS] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    for M in cells.U8_MS:
        K = cells.small_k(M)
        assert M * K <= 4096 and K & (K - 1) and K < 128
        assert cells.search_lds(8 * M * K * 4, 8, 1) <= cells.LDS_BYTES          # 8 tables fit


def test_planner_in_sync_with_the_sources():
    """the value lists the planner mirrors, literally: a change there must break this test, not silently the coverage"""
    u8 = src("adc_search_u8_launch.hip.h")
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_U8, "pqhip::kAdcMaxValueWords") in u8
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_U8_LISTS, "pqhip::kAdcMaxValueWords") in u8
    assert len(re.findall(r"dispatch_int<[^>]*>\(nvb", u8)) == 2
    assert "if constexpr (NQ * L > 16)" in u8
    p4 = src("pqhip_adc_packed4.hip")
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_P4, "kPacked4MaxValueWords") in p4
    assert "for (int b : {%s})" % lst(cells.NV_P4, "kPacked4MaxValueWords") in p4
    assert "for (int b : {%s})" % lst(cells.NV_P4_LISTS, "kPacked4MaxValueWords") in p4
    assert "if constexpr (NQ * L > 16)" in p4
    assert "(size_t)cb->M * 16 * sizeof(float)" in p4 and "cb->K > 16 || cb->M > 100 || k > kSearchMaxK" in p4
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_P4_LISTS, "kPacked4MaxValueWords") in src("pqhip_adc_packed4_lists.hip")
    rng = src("pqhip_adc_range.hip")
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_U8, "kAdcMaxValueWords") in rng
    assert "dispatch_int<%s>(nvb" % lst(cells.NV_U8_LISTS, "kAdcMaxValueWords") in rng
    launch = src("adc_search_launch.h")
    assert "dispatch_list_regs(int L, F&& f) { return dispatch_int<%s>(L, f); }" % lst(cells.LIST_REGS) in launch
    assert "dispatch_queries_per_pass(int nq_pass, F&& f) { return dispatch_int<%s>(nq_pass, f); }" % lst(cells.QUERIES_PER_PASS) in launch
    assert "kListsScratchBytes = 512u << 20" in launch and cells.LISTS_SCRATCH_BYTES == 512 << 20
    adc = src("pqhip_adc.hip")
    assert adc.count("for (int b : {%s})" % lst(cells.NV_U8, "kAdcMaxValueWords")) == 1
    assert adc.count("for (int b : {%s})" % lst(cells.NV_U8_LISTS, "kAdcMaxValueWords")) == 1
    assert "for (int nqp : {%s})" % lst(cells.QUERIES_PER_PASS) in adc and "for (int c : {8, 4})" in adc
    assert "c * L <= 16 && search_lds(table * c, c, L) <= 160 * 1024" in adc
    assert "int lk = 64; while (lk < k) lk <<= 1; return lk / 64;" in adc
    assert "(size_t)kSearchWaves * nq * kSearchQueue * 2 * sizeof(unsigned)" in adc
    assert "(size_t)kSearchWaves * nq * 64 * L * 2 * sizeof(unsigned)" in adc
    assert "kAdcMaxValueWords = %d;" % cells.ADC_MAX_VALUE_WORDS in src("kernels_adc.hip.h")
    assert "kPacked4MaxValueWords = %d;" % cells.PACKED4_MAX_VALUE_WORDS in src("kernels_adc_packed4.hip.h")
    ks = src("kernels_adc_search.hip.h")
    assert "kSearchQueue = %d;" % cells.SEARCH_QUEUE in ks and "kSearchWaves = %d;" % cells.SEARCH_WAVES in ks
    assert "kSearchMaxK = %d;" % cells.MAX_K in ks
    # the kernel names of the log, where the launchers write them
    for call in cells.all_grid_calls():
        for name, cnt in cells.plan(call).log:
            assert cnt >= 1
    names = {name for call in cells.all_grid_calls() for name, cnt in cells.plan(call).log}
    text = u8 + p4 + src("pqhip_adc_packed4_lists.hip") + adc
    for name in names:
        assert '"%s"' % name in text, name


def test_option_adc_search_wgs_is_wired():
    for path in (os.path.join(ROOT, "include", "pqhip.h"), os.path.join(CSRC, "pqhip_ctx.hip"),
                 os.path.join(ROOT, "rust", "pqhip_ffi.rs")):
        with open(path) as f:
            assert '"adc_search_wgs"' in f.read(), path
    assert "adc_search_wgs{0}" in src("pqhip_internal.h")
    assert "cb->ctx->opt.adc_search_wgs.load(std::memory_order_relaxed), producer}" in src("pqhip_adc.hip")
    assert "`adc_search_wgs`" in src("DESIGN.md", ROOT)
    assert "adc_search_wgs" not in src(os.path.join("tests", "conftest.py"), ROOT)
