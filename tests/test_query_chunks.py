"""The model of the search drivers' query loops (tests/query_chunks.py) on the CPU: every call of
test_gpu_query_chunks.py needs at least three launches with a shorter last one, stays within computed memory bounds, the
period of its repeated queries divides no chunk, and the chunk expressions the model mirrors still stand literally in
the five sources -- a rewrite of a loop has to update the model knowingly."""
import adc_search_cells as cells
import query_chunks as qc


def test_constants_come_from_the_sources():
    assert qc.LISTS_SCRATCH_BYTES == cells.LISTS_SCRATCH_BYTES == 512 << 20
    assert qc.RERANK_SCRATCH_BYTES == 64 << 20
    assert qc.RANGE_SCAN_MAX == 1 << 20 and qc.RANGE_WAVES == 16 and qc.RERANK_MAX_CAND == 1024
    assert qc.GRID_CAPS == {"lists": 4096, "flat_lists": 4096, "among": 4096, "range_lists": 4096, "rerank": 1024}
    assert qc.constant("kX", "constexpr size_t kX = 3u << 4;   // text") == 48
    assert qc.constant("kY", "constexpr int kY = 2 * 8;") == 16


def test_chunk_values():
    """the bounds one at a time: the queries, gridDim.y, the scratch, the scan"""
    big = qc.MANY
    assert qc.chunk("lists", big, 4096, 1024, 3) == 10 == qc.chunk("flat_lists", big, 4096, 1024, 3)
    assert qc.chunk("among", big, 4096, 1024) == 10
    assert qc.chunk("lists", big, 9999, 1024, 3) == 10                       # the cap on the forced grid
    assert qc.chunk("lists", big, 4096, 513, 3) == 10 and qc.chunk("lists", big, 4096, 64, 3) == 170
    assert qc.chunk("range_lists", big, 4096, 1, 3) == 16                    # kRangeScanMax / (16 G)
    assert qc.chunk("range_lists", big, 1024, 1, 3) == 64
    assert qc.chunk("rerank", big, 1024, 5, 0, 1024) == 8192 and qc.chunk("rerank", big, 1, 3, 0, 2) == 65535
    for d in ("lists", "flat_lists", "among", "range_lists"):
        assert qc.chunk(d, big, 1, 3, 3) == 65535 and qc.chunk(d, 17, 1, 3, 3) == 17
    assert qc.chunk("lists", big, 1, 3, (1 << 24) - 1) == 1                  # the plan alone fills half of the scratch
    assert qc.chunk("padding", big, 1, 2) == 65535
    assert qc.launches("lists", 23, 4096, 1024, 3) == 3 and qc.launches("lists", 20, 4096, 1024, 3) == 2
    # the lists formula is the planner's: the same launches for the same call
    for nq, G, k, n_probe in ((23, 4096, 1024, 3), (343, 4096, 64, 3), (131075, 1, 3, 3), (13, 2, 129, 10), (99, 700, 513, 40)):
        planned = cells.plan(cells.Call("u8", True, False, False, False, qc.M, qc.K_U8, k, nq, 1, n_probe, G))
        assert {cnt for name, cnt in planned.log} == {qc.launches("lists", nq, G, k, n_probe)}, (nq, G, k, n_probe)


def test_every_case_enters_the_third_launch_with_a_shorter_last_chunk():
    assert len(qc.CASES) == 2 * sum(len(qc.ITEMS[d]) for d in qc.DRIVER_FILES) + len(qc.ITEMS["padding"])
    for c in qc.CASES:
        assert c.launches >= 3, c
        rest = c.nq - 2 * c.chunk
        assert 0 < rest < c.chunk and c.launches == 3, c
        assert c.chunk == qc.chunk(c.driver, c.nq, c.G, c.k, c.n_probe, c.n_cand)
        assert c.launches == qc.launches(c.driver, c.nq, c.G, c.k, c.n_probe, c.n_cand)
    # the routes are the ones they are named after: S is bounded by the scratch (the scan for the range calls), Y by gridDim.y
    for c in qc.CASES:
        if c.route == "Y":
            assert c.chunk == qc.GRID_Y and c.nq == 2 * 65535 + 5, c
        else:
            assert c.chunk < qc.GRID_Y and c.G == qc.GRID_CAPS[c.driver], c
    got = {(c.driver, c.route): (c.chunk, c.nq) for c in qc.CASES}
    assert got[("lists", "S")] == got[("flat_lists", "S")] == got[("among", "S")] == (10, 23)
    assert got[("range_lists", "S")] == (16, 37) and got[("rerank", "S")] == (8192, 16389)


def test_every_case_stays_within_the_memory_bounds():
    for c in qc.CASES:
        assert qc.leased_bytes(c) <= qc.SCRATCH_LIMIT[c.driver], c
        assert qc.io_bytes(c) <= qc.IO_LIMIT, (c, qc.io_bytes(c))
    assert qc.SCRATCH_LIMIT["rerank"] == 64 << 20 and qc.SCRATCH_LIMIT["lists"] == 512 << 20 and qc.IO_LIMIT == 256 * 10 ** 6
    # the bounds bind: route S leases nearly all of the scratch
    assert qc.leased_bytes(qc.case("lists", "l2", "S")) > 450 << 20
    assert qc.leased_bytes(qc.case("rerank", "l2_f32", "S")) == 64 << 20


def test_the_period_divides_no_chunk():
    """a row read from or written to the same place of another chunk then belongs to another pattern"""
    assert qc.PERIOD == 7
    for c in qc.CASES:
        assert c.chunk % qc.PERIOD != 0, c
        assert c.period == qc.PERIOD or (c.period == c.nq and c.route == "S"), c
        if c.route == "Y" or c.driver == "rerank":
            assert c.period == qc.PERIOD, c
    for chunk in (10, 16, 170, 8192, 65535):
        assert chunk % qc.PERIOD != 0


def test_strides_of_the_cases_tell_the_matrices_apart():
    assert len({qc.N_PROBE, qc.P_RS, qc.B_RS, qc.N_LISTS}) == 4 and qc.P_RS > qc.N_PROBE and qc.B_RS > qc.N_PROBE


def test_logs():
    assert qc.log(qc.case("lists", "l2", "S")) == "k_adc_lists_plan x3 + k_adc_search_lists_u8 x3 + k_adc_search_merge x3"
    assert qc.log(qc.case("lists", "ip_scaled", "Y"), ip=True) == ("k_adc_lists_plan x3 + k_adc_ip_search_lists_u8 x3 + "
                                                                  "k_adc_ip_search_merge x3")
    assert qc.log(qc.case("lists", "masked", "Y")) == "k_adc_lists_plan x3 + k_adc_search_lists_masked_u8 x3 + k_adc_search_merge x3"
    assert qc.log(qc.case("lists", "residual", "S")) == ("k_adc_lists_plan x3 + k_adc_search_lists_residual_u8 x3 + "
                                                         "k_adc_search_merge x3")
    assert qc.log(qc.case("lists", "packed4", "S")) == "k_adc_lists_plan x3 + k_adc_search_lists_p4 x3 + k_adc_search_merge x3"
    assert qc.log(qc.case("flat_lists", "ip_f16", "Y"), ip=True) == ("k_adc_lists_plan x3 + k_flat_ip_search_lists x3 + "
                                                                    "k_adc_ip_search_merge x3")
    assert qc.log(qc.case("among", "residual", "S")) == "k_adc_among_residual_u8 x3 + k_adc_search_merge x3"
    assert qc.log(qc.case("among", "shared", "Y"), ip=True) == "k_adc_ip_among_u8 x3 + k_adc_ip_search_merge x3"
    assert qc.log(qc.case("range_lists", "l2", "S")) == "k_adc_lists_plan x3 + k_adc_range_lists_u8 x6 + k_adc_range_scan x3"
    assert qc.log(qc.case("range_lists", "l2", "S"), count_only=True) == ("k_adc_lists_plan x3 + k_adc_range_lists_u8 x3 + "
                                                                         "k_adc_range_scan x3")
    assert qc.log(qc.case("range_lists", "residual_ip_scaled", "Y"), ip=True) == (
        "k_adc_lists_plan x3 + k_adc_ip_range_lists_residual_u8 x6 + k_adc_range_scan x3")
    assert qc.log(qc.case("rerank", "ip_f16", "S")) == "k_rerank_dist x3 + k_rerank_select x3"
    assert qc.log(qc.case("padding", "among", "Y"), ip=True) == "k_adc_ip_search_merge x3"


def test_model_in_sync_with_the_sources():
    """the chunk expressions, the pointer offsets of every step and the kernel names of the logs, literally"""
    lists_chunk = ("const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, "
                   "(int64_t)(kListsScratchBytes / (plan_q + lists_q))}));")
    plan_q = "const size_t plan_q = ((size_t)n_probe * 2 + 1) * sizeof(int64_t);"
    lists_q = "const size_t lists_q = (size_t)G * 64 * L * (sizeof(unsigned) + sizeof(uint64_t));"
    loop = "for (int64_t q = 0; q < nq; q += chunk) {"
    nqc = "const unsigned nqc = (unsigned)std::min<int64_t>(chunk, nq - q);"
    outputs = "d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs"
    tables = "d_tables + q * (int64_t)M * K"
    cap = "const int64_t G = forced > 0 ? std::min<int64_t>(forced, %d)"

    adc = qc.src("pqhip_adc.hip")
    for text in (lists_chunk, plan_q, lists_q, loop, nqc, outputs, tables, cap % 4096, "d_probes + q * p_rs",
                 "res ? res->bias + q * res->b_rs : nullptr", "PQCHK(lease.acquire((size_t)chunk * (plan_q + lists_q)));",
                 "for (int64_t q = 0; q < nq; q += 65535) {", "const int nqp = (int)std::min<int64_t>(nq - q, 65535);",
                 "launch_search_merge(ip, L, nqp, 0, k, nullptr, nullptr, d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs, st)"):
        assert text in adc, text
    assert adc.count(loop) == 1 and adc.count(lists_chunk) == 1

    flat = qc.src("pqhip_flat_search_lists.hip")
    for text in (lists_chunk, plan_q, lists_q, loop, nqc, outputs, cap % 4096, "d_probes + q * p_rs", "d_q + q * q_rs, q_rs",
                 "PQCHK(lease.acquire((size_t)chunk * (plan_q + lists_q)));"):
        assert text in flat, text
    assert flat.count(loop) == 1

    among = qc.src("pqhip_adc_among.hip")
    for text in ("const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, "
                 "(int64_t)(kListsScratchBytes / lists_q)}));", lists_q, loop, nqc, outputs, tables, cap % 4096,
                 "d_lims ? d_lims + q : nullptr", "residual ? d_bias + q * b_rs : nullptr",
                 "PQCHK(lease.acquire((size_t)chunk * lists_q));"):
        assert text in among, text
    assert among.count(loop) == 1

    rng = qc.src("pqhip_adc_range.hip")
    for text in ("const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)65535, "
                 "(int64_t)(kListsScratchBytes / (plan_q + part_q)),\n"
                 "                                                                  kRangeScanMax / units}));",
                 "const size_t plan_q = ((size_t)std::max(n_probe, 1) * 2 + 1) * sizeof(int64_t);",
                 "const int64_t units = G * kRangeWaves;", "const size_t part_q = (size_t)units * sizeof(int64_t);",
                 loop, nqc, tables, cap % 4096, "d_probes + q * p_rs", "res ? d_bias + q * b_rs : nullptr", "d_extra, d_thr + q,",
                 "PQCHK(launch_range_scan(part, units, nqc, d_lims + q, st));", "PQCHK(lease.acquire((size_t)chunk * (plan_q + part_q)));",
                 "HIPCHK(hipMemsetAsync(d_lims, 0, sizeof(int64_t), st));"):
        assert text in rng, text
    assert rng.count(loop) == 1

    rerank = qc.src("pqhip_rerank.hip")
    for text in ("const int64_t chunk = std::min<int64_t>({nq, (int64_t)65535, "
                 "(int64_t)(kRerankScratchBytes / ((size_t)n_cand * sizeof(uint64_t)))});", loop, nqc, cap % 1024,
                 "const float* qp = d_q + q * q_rs;", "const int64_t* cp = d_cand + q * c_rs;",
                 "PQCHK(lease.acquire((size_t)chunk * n_cand * sizeof(uint64_t)));", "n_cand > kRerankMaxCand"):
        assert text in rerank, text
    assert rerank.count("d_val + q * v_rs, v_rs, d_idx + q * i_rs, i_rs") == 2 and rerank.count(loop) == 1

    # the kernel names of the logs, where the launchers write them
    text = adc + flat + among + rng + rerank + "".join(qc.src(f) for f in (
        "adc_search_u8_launch.hip.h", "pqhip_adc_packed4_lists.hip", "pqhip_adc_packed4.hip", "pqhip_adc_masked.hip"))
    for c in qc.CASES:
        for ip in (False, True):
            for name in qc.log(c, ip=ip).split(" + "):
                assert '"%s"' % name.split(" x")[0] in text, name
    # the options the GPU test forces
    ctx = qc.src("pqhip_ctx.hip")
    for driver, option in qc.OPTIONS.items():
        assert '"%s"' % option in ctx and "opt.%s.load" % option in qc.src(qc.DRIVER_FILES[driver]), option
