"""nearest_among / most_similar_among of the three matrix classes on the GPU, on the small trained fixture of
test_gpu_qmatrix_packed4.py (3,000 vectors, 16 lists).  A search among given rows is DEFINED by the filtered search: for
distinct rows it returns, torch.equal with values by their bit patterns, what nearest / most_similar return with
allow=<flags of the rows> for that query alone (all lists probed on the partitioned classes).  The pair (lims, rows) of a
range search goes in as it is; refine= re-ranks the shortlist; row numbers out of range do not fault."""
import numpy as np
import pytest

from test_gpu_qmatrix_packed4 import KINDS, N, N_LISTS, assert_equal_results, world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


def probe_kw(kind):
    return {} if kind == "flat" else {"nprobe": N_LISTS}


def filtered(m, kind, ip, q, rows, k, **kw):
    """the definition: the filtered search of one query with the flags of `rows`"""
    flags = np.zeros(N, bool)
    r = np.asarray(rows)
    flags[r[(r >= 0) & (r < N)]] = True
    search = m.most_similar if ip else m.nearest
    return search(q, k, allow=flags, **probe_kw(kind), **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", (4, 5))
def test_among_is_the_filtered_search(ra, kind, M):
    import torch
    w = world(ra, M)
    m = w.m[kind]
    rng = np.random.default_rng(8200 + M)
    qd = torch.from_numpy(w.queries).cuda()
    nq = qd.shape[0]
    # a shared list, numpy and torch, shuffled, with padding
    shared = rng.permutation(N)[:700].astype(np.int64)
    shared[5] = -1
    for k in (1, 10, 300):
        for ip, kws in ((False, [{}]), (True, [{"use_norms": True}, {"use_norms": False}])):
            among = m.most_similar_among if ip else m.nearest_among
            for kw in kws:
                got = among(qd, shared, k, **kw)
                assert tuple(got[0].shape) == (nq, k) and got[1].dtype == torch.int64
                assert_equal_results(among(qd, torch.from_numpy(shared).cuda(), k, **kw), got)
                for q in range(nq):
                    want = filtered(m, kind, ip, qd[q], shared, k, **kw)
                    assert_equal_results((got[0][q], got[1][q]), want)
                one = among(qd[3], shared, k, **kw)                        # a single query: [k]
                assert tuple(one[0].shape) == (k,)
                assert_equal_results(one, (got[0][3], got[1][3]))
    # a CSR: lengths 0, 1, 65, 1,025 and more, rows of every query distinct
    lengths = [0, 1, 65, 1025, 7, 2000, 300, 64, 1024][:nq]
    parts = [rng.permutation(N)[:n].astype(np.int64) for n in lengths]
    lims = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = np.concatenate(parts)
    for ip in (False, True):
        among = m.most_similar_among if ip else m.nearest_among
        got = among(qd, (lims, rows), 65)
        assert_equal_results(among(qd, (torch.from_numpy(lims).cuda(), torch.from_numpy(rows).cuda()), 65), got)
        for q in range(nq):
            assert_equal_results((got[0][q], got[1][q]), filtered(m, kind, ip, qd[q], parts[q], 65))
            assert int((got[1][q] >= 0).sum()) == min(65, lengths[q])


@pytest.mark.parametrize("kind", KINDS)
def test_range_result_goes_in_as_it_is(ra, kind):
    """(lims, rows) straight from within() / similar_above(): the k best of that range result"""
    import torch
    w = world(ra, 4)
    m = w.m[kind]
    qd = torch.from_numpy(w.queries).cuda()
    kw = probe_kw(kind)
    k = 10
    for ip in (False, True):
        search, rng_search, among = (m.most_similar, m.similar_above, m.most_similar_among) if ip else (m.nearest, m.within, m.nearest_among)
        edge = search(qd, 200, **kw)[0][:, -1].contiguous()               # per query: the value of the 200th row
        lims, val, idx = rng_search(qd, edge, **kw)
        counts = (lims[1:] - lims[:-1]).cpu().numpy()
        assert (counts >= 200).all()
        got = among(qd, (lims, idx), k)
        assert_equal_results(got, search(qd, k, **kw))                     # the range holds the 200 best, so its k best are the k best
        for q in range(qd.shape[0]):
            seg = val[int(lims[q]):int(lims[q + 1])]
            best = torch.sort(seg, descending=ip).values[:k]
            assert torch.equal(best.view(torch.int32), got[0][q].view(torch.int32))
            assert np.isin(got[1][q].cpu().numpy(), idx[int(lims[q]):int(lims[q + 1])].cpu().numpy()).all()


@pytest.mark.parametrize("kind", KINDS)
def test_refine_reranks_the_first_rows(ra, kind):
    import torch
    w = world(ra, 4)
    m = w.m[kind]
    qd = torch.from_numpy(w.queries).cuda()
    rows = np.random.default_rng(8210).permutation(N)[:900].astype(np.int64)
    for ip in (False, True):
        among = m.most_similar_among if ip else m.nearest_among
        _, short = among(qd, rows, 100)
        want = m.pq.rerank_device(qd, m.vectors, short, 10, ip=ip)
        assert_equal_results(among(qd, rows, 10, refine=100), want)
    with pytest.raises(ra.PanicError, match="refine must lie between k and 1024"):
        m.nearest_among(qd, rows, 10, refine=5)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_out_of_range_do_not_fault(ra, kind):
    """-1 is padding; N, -7 and 2^40 are skipped, and raise the reference's index panic with check=True"""
    import torch
    w = world(ra, 4)
    m = w.m[kind]
    qd = torch.from_numpy(w.queries).cuda()
    good = np.random.default_rng(8211).permutation(N)[:500].astype(np.int64)
    want = m.nearest_among(qd, good, 20, check=True)
    padded = np.insert(good, [0, 100, 500], -1)
    assert_equal_results(m.nearest_among(qd, padded, 20, check=True), want)
    for bad in (N, -7, 1 << 40, -(1 << 40)):
        rows = np.insert(padded, [3, 400], bad)
        assert_equal_results(m.nearest_among(qd, rows, 20), want)
        assert_equal_results(m.most_similar_among(qd, rows, 20), m.most_similar_among(qd, good, 20))
        torch.cuda.synchronize()
        for among in (m.nearest_among, m.most_similar_among):
            with pytest.raises(ra.PanicError, match="index out of bounds"):
                among(qd, rows, 20, check=True)
    # lims of the wrong length are refused before any launch
    with pytest.raises(ra.PanicError, match="one offset per query"):
        m.nearest_among(qd, (np.zeros(3, np.int64), good), 5)


@pytest.mark.parametrize("kind", KINDS)
def test_packed_matrix_raises(ra, kind):
    import torch
    w = world(ra, 4)
    p = w.m[kind].pack4()
    qd = torch.from_numpy(w.queries).cuda()
    rows = np.arange(10, dtype=np.int64)
    with pytest.raises(ra.PanicError, match=r"nearest_among\(\) does not read 4-bit packed codes: call unpack4\(\) first"):
        p.nearest_among(qd, rows, 5)
    with pytest.raises(ra.PanicError, match=r"most_similar_among\(\) does not read 4-bit packed codes: call unpack4\(\) first"):
        p.most_similar_among(qd, rows, 5)
    assert_equal_results(p.unpack4().nearest_among(qd, rows, 5), w.m[kind].nearest_among(qd, rows, 5))
