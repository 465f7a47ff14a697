"""ADC range search for query batches (Pq.adc_range_batch_device / adc_range_lists_batch_device: table screen at the
thresholds, exact range call among its candidates) against the unchanged plain calls (adc_range_device,
adc_ip_range_device with scales, and their list forms), in one process on the same buffers, on one MI355X.

Data and quantizer: the mixture of tools/adc_batch_time.py (1,024 centres, noise 0.35, log-normal lengths; K = 256, 8
k-means iterations on 200,000 unit rows).  For the list form the rows are stored list by list, the list of a row being the
centre it was drawn from, and a query probes the nprobe centres nearest to it.

Shapes: n rows (default 10 M) at d = 300 / M = 15 and d = 768 / M = 48; squared L2 and scaled inner product; nq in {8, 16,
32, 64, 256, 1,024}; two radii per query, taken from top-k calls: the 50th best value of the query over all rows
("narrow"), and the 1,000th best over every 5th row, about the 5,000th best overall ("wide"); image_bits 8 and 16.  Lists:
1,024 lists, nprobe 8 and 64, the same radii, the u8 image.  Rows that share a code tie: where the 50th best value is tied
among many rows the narrow radius returns all of them (rows_per_query records what a cell returned).
Every cell first compares the batch route bit for bit with the plain call, then times both in the same run: HIP events,
median of 5 after 2 warm-up calls (3 after 1 where one call takes more than a second), one block per call, not alternated.  The baseline is the plain range
call of this tree, never the new path.  Each cell records the screen's candidates as a share of n nq (lists: of the rows
the plain call returns), the screen alone, the count call of the candidate stage (capacity 0: count pass and scan) and its
filling call (count pass, scan and fill pass) -- the fill pass is the difference.
"crossover" is the smallest nq from which the batch route wins a column by more than the larger spread of the two, for
every larger nq; a cell where it does not win is listed under "findings" with its ratio.

Writes JSON (default profiles/adc_range_batch_time.json and, beside it, adc_range_lists_batch_time.json).

usage: python tools/adc_range_batch_time.py [out.json] [n_rows] [M ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reductive_amd as ra  # noqa: E402
from reductive_amd import _marshal, pq as rules  # noqa: E402
from flat_batch_time import same, timed  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adc_range_batch_time.json")
OUT_LISTS = os.path.join(os.path.dirname(os.path.abspath(OUT)), os.path.basename(OUT).replace("range_batch", "range_lists_batch"))
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
DIMS = {15: 300, 48: 768}
MS = [int(a) for a in sys.argv[3:]] or [15, 48]
K = 256
NQS = (8, 16, 32, 64, 256, 1024)
CENTRES, NOISE, LENGTH_SIGMA = 1024, 0.35, 0.25
TRAIN_ROWS, TRAIN_ITERATIONS = 200_000, 8
CHUNK = 500_000
NPROBES = (8, 64)


def draw(centres, n, gen):
    c = torch.randint(0, CENTRES, (n,), device="cuda", generator=gen)
    x = centres[c] + NOISE * torch.randn((n, centres.shape[1]), device="cuda", generator=gen)
    return x * torch.exp(LENGTH_SIGMA * torch.randn((n, 1), device="cuda", generator=gen)), c


def unit(x):
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def index(M, gen):
    """-> (pq, codes [N, M] u8 list by list, lengths [N], list_off, L2 tables, IP tables, probes [nq, 64])"""
    d = DIMS[M]
    centres = torch.randn((CENTRES, d), device="cuda", generator=gen)
    train = unit(draw(centres, TRAIN_ROWS, gen)[0])
    init = train[:K].cpu().numpy().reshape(K, M, d // M).transpose(1, 0, 2)
    books, _ = rules.kmeans_iterations(init, train, TRAIN_ITERATIONS, want_loss=False)
    pq = ra.Pq(None, books)
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(N, dtype=torch.float32, device="cuda")
    lists = torch.empty(N, dtype=torch.int64, device="cuda")
    for r0 in range(0, N, CHUNK):
        x, lists[r0:r0 + CHUNK] = draw(centres, min(CHUNK, N - r0), gen)
        lengths[r0:r0 + CHUNK] = x.norm(dim=1)
        pq.quantize_batch_device(unit(x), out=codes[r0:r0 + CHUNK])
    order = torch.argsort(lists, stable=True)
    codes, lengths = codes[order].contiguous(), lengths[order].contiguous()
    list_off = torch.zeros(CENTRES + 1, dtype=torch.int64, device="cuda")
    list_off[1:] = torch.cumsum(torch.bincount(lists, minlength=CENTRES), 0)
    q = draw(centres, max(NQS), gen)[0]
    probes = torch.topk(torch.cdist(q, centres), max(NPROBES), dim=1, largest=False)[1].contiguous()
    torch.cuda.synchronize()
    return pq, codes, lengths, list_off, pq.adc_tables_device(unit(q)), pq.adc_ip_tables_device(q.contiguous()), probes


def radii(pq, codes, t, ip, kw):
    """per query: the 50th best value over all rows, and the 1,000th best over every 5th row"""
    search = pq.adc_ip_search_device if ip else pq.adc_search_device
    among = pq.adc_ip_among_device if ip else pq.adc_among_device
    narrow = search(codes, t, 50, **kw)[0][:, 49].contiguous()
    wide = among(codes, t, torch.arange(0, N, 5, dtype=torch.int64, device="cuda"), 1000, **kw)[0][:, 999].contiguous()
    return {"narrow": narrow, "wide": wide}


def stages(pq, codes, t, thr, ip, kw, screen):
    """screen() -> (lims, ids): the screen alone, then the candidate stage's count call and its filling call"""
    out = {}
    out["screen_ms"], _ = timed(screen)
    lims, ids = screen()
    extra = kw.get("scales")
    _, nq, keep, head = pq._adc_among_head(ip, codes, t, ids, None, lims, None, None, extra, "scales")   # keep: held to the end
    cd = keep[0]
    name = "pqhip_adc_%samong_range_f32_dev" % ("ip_" if ip else "")
    cb, slot, sp = _marshal.launch(pq, cd, None)
    thd = _marshal.threshold_arg(thr, nq, cd.device)
    out_lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    out["count_call_ms"], _ = timed(lambda: _marshal.run(name, cb, slot, *head, thd.data_ptr(), out_lims.data_ptr(), None, None, 0, sp))
    total = max(int(out_lims[-1]), 1)
    val = torch.empty(total, dtype=torch.float32, device="cuda")
    idx = torch.empty(total, dtype=torch.int64, device="cuda")
    out["fill_call_ms"], _ = timed(lambda: _marshal.run(name, cb, slot, *head, thd.data_ptr(), out_lims.data_ptr(), val.data_ptr(),
                                                        idx.data_ptr(), total, sp))
    out["candidates"] = int(ids.shape[0])
    return {a: (round(b, 4) if isinstance(b, float) else b) for a, b in out.items()}


def measure(res, cell, batch, plain, label, wins):
    want = plain()
    cell["equal"] = same(batch(), want)
    assert cell["equal"], cell
    cell["rows_per_query"] = round(int(want[0][-1]) / cell["nq"], 1)
    cell["batch_ms"], cell["batch_all"] = timed(batch)
    cell["plain_ms"], cell["plain_all"] = timed(plain)
    cell["spread_ms"] = round(max(max(a) - min(a) for a in (cell["batch_all"], cell["plain_all"])), 4)
    cell["batch_over_plain"] = round(cell["batch_ms"] / cell["plain_ms"], 4)
    won = cell["plain_ms"] - cell["batch_ms"] > cell["spread_ms"]
    wins.append(won)
    if not won:
        res["findings"].append("%s nq=%d: batch %.3f ms, plain %.3f ms (x%.2f)" % (label, cell["nq"], cell["batch_ms"], cell["plain_ms"],
                                                                                  cell["batch_over_plain"]))
    res["cells"].append(cell)


def main():
    head = {"device": torch.cuda.get_device_name(0), "rows": N, "K": K, "shapes": {"M=%d" % M: {"d": DIMS[M]} for M in MS},
            "protocol": "HIP events, median of 5 after 2 warm-up calls (3 after 1 when a call takes more than a second); the batch "
                        "route and the plain call are timed in two consecutive blocks, not alternated; the fill pass is not "
                        "timed alone: fill_call_ms is count pass + scan + fill pass, count_call_ms count pass + scan; "
                        "baseline: the plain range call of the same tree"}
    res = dict(head, cells=[], crossover={}, findings=[])
    res_l = dict(head, lists=CENTRES, cells=[], crossover={}, findings=[])
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)

    def save():
        for path, r in ((OUT, res), (OUT_LISTS, res_l)):
            with open(path, "w") as f:
                json.dump(r, f, indent=1)

    for M in MS:
        pq, codes, lengths, list_off, t_l2, t_ip, probes = index(M, torch.Generator(device="cuda").manual_seed(71 + M))
        for ip, form, tables, kw in ((False, "l2", t_l2, {}), (True, "ip_scaled", t_ip, {"scales": lengths})):
            plain = pq.adc_ip_range_device if ip else pq.adc_range_device
            plain_l = pq.adc_ip_range_lists_device if ip else pq.adc_range_lists_device
            thr_all = radii(pq, codes, tables, ip, kw)
            for radius, thr_q in thr_all.items():
                for bits in (8, 16):
                    wins, label = [], "M=%d %s %s u%d" % (M, form, radius, bits)
                    for nq in NQS:
                        t, thr = tables[:nq].contiguous(), thr_q[:nq].contiguous()
                        cell = {"M": M, "form": form, "radius": radius, "image_bits": bits, "nq": nq}
                        measure(res, cell, lambda: pq.adc_range_batch_device(codes, t, thr, ip=ip, image_bits=bits, **kw),
                                lambda: plain(codes, t, thr, **kw), label, wins)
                        cell["stages"] = stages(pq, codes, t, thr, ip, kw,
                                                lambda: pq.adc_screen_device(codes, t, thr, ip=ip, image_bits=bits, **kw))
                        cell["candidate_share"] = round(cell["stages"]["candidates"] / (float(N) * nq), 6)
                        save()
                        print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
                    res["crossover"][label] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
                for nprobe in NPROBES:
                    wins, label = [], "M=%d %s %s nprobe=%d" % (M, form, radius, nprobe)
                    for nq in NQS:
                        t, thr, pr = tables[:nq].contiguous(), thr_q[:nq].contiguous(), probes[:nq, :nprobe].contiguous()
                        cell = {"M": M, "form": form, "radius": radius, "nprobe": nprobe, "nq": nq}
                        measure(res_l, cell, lambda: pq.adc_range_lists_batch_device(codes, t, list_off, pr, thr, ip=ip, **kw),
                                lambda: plain_l(codes, t, list_off, pr, thr, **kw), label, wins)
                        cell["stages"] = stages(pq, codes, t, thr, ip, kw,
                                                lambda: pq.adc_screen_lists_device(codes, t, list_off, pr, thr, ip=ip, **kw))
                        cell["candidates_per_returned_row"] = round(cell["stages"]["candidates"] / max(cell["rows_per_query"] * nq, 1), 3)
                        save()
                        print(json.dumps({a: b for a, b in cell.items() if not a.endswith("_all")}), flush=True)
                    res_l["crossover"][label] = next((NQS[i] for i in range(len(NQS)) if all(wins[i:])), None)
        del pq, codes, lengths, list_off, t_l2, t_ip, probes
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
