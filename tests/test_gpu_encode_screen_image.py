"""k_encode_mfma16<8, 20, *>: the f16 codebook image built once per codebook.

k_build_screen_image writes the image and max cc when a Pq handle's codebook is prepared (a training handle's in front of
the first launch that screens with it); the encode kernel copies them.  What can go
wrong is an image that is not the one the kernel would have built for itself -- another scale, another codebook's image,
a stale one -- and every such image gives wrong codes somewhere, so the codes are compared with the oracle bit for bit:

    scale edges   the scale is s = 2^e, e = floor((13 - floor(log2 max cc)) / 2).  Codebooks whose largest norm is exactly
                  2^j and one ulp below it, j = 0 (where e steps from 7 to 6) and j = 1 (where it does not); the whole
                  problem scaled by 2^-40 and 2^+40; a codebook with max cc below 2^-100, whose rows all take the exact
                  path; and a finite max cc >= 2^100.  That last codebook fails the finite-norm check of codebook creation,
                  and the dispatch gives such a Pq handle to no matrix-core kernel at all: its codes are compared, its
                  kernel name is not asserted.
    two handles   two Pq handles with different codebooks (and different scales) alive on one context, encoding
                  alternately, and one of them twice in a row
    k-means       a handle whose centroids change: kmeans_iterations on 20,000 x 60, K = 256, one iteration and three (the
                  graph path), centroids and losses against the oracle bit for bit.  The assignment step of k-means does
                  not take k_encode_mfma16 at any n: the dispatch keeps it on k_encode_mfma_lds3 because the update kernels
                  run beside it (plan_encode, beside_update), so raising n does not change the kernel; the test says which
                  one ran, and that the training handle's image, marked stale by every preparation, is never built.  The
                  trained centroids then go into a Pq handle, which does encode on k_encode_mfma16.
    training step the one place where a handle screens after its centroids moved: the OPQ training step runs a k-means
                  iteration and then encodes with the same handle on k_encode_mfma16.  Its image is built once, in front of
                  that launch, from the new centroids; centroids and cross product against the oracle bit for bit.

Shapes as in test_gpu_encode_screen_pairs.py: M = 3, dsub = 20, K = 256 and 225; n = 20,000 (rows_per_item 32) and
204,813 (rows_per_item 64, ragged end); u8 and i32 codes."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

M, DSUB = 3, 20
N_SMALL, N_BIG = 20_000, 204_813
PLANT = 77                                    # the centroid that carries the largest norm
U = np.float32(1.0 / 4096.0)
# Largest norms by construction.  Every product and every partial sum of rule 1 (eight partial sums, then p0 + p4, p1 + p5,
# p2 + p6, p3 + p7 in that order) is an integer multiple of 2^-24 that f32 holds exactly:
#   4095^2 + 90^2 + 9^2 + 3^2 = 2^24 - 1, and twice that, pairwise, is 2^25 - 2
EDGES = {
    "2^0": ([1.0], 1.0),
    "2^0-ulp": ([4095 * U, 90 * U, 9 * U, 3 * U], float(np.nextafter(np.float32(1.0), np.float32(0.0)))),
    "2^1": ([1.0, 1.0], 2.0),
    "2^1-ulp": ([4095 * U, 90 * U, 9 * U, 3 * U, 4095 * U, 90 * U, 9 * U, 3 * U], float(np.nextafter(np.float32(2.0), np.float32(0.0)))),
}
SCALES = {"2^-40": -40, "2^+40": 40, "tiny": -51, "huge": 52}


def _rows_per_item(n):
    rpi = -(-(n * M) // 16384)
    return min(1024, max(32, -(-rpi // 32) * 32))


_shared = {}


def _base(K):
    """the shared codebook (every norm below 0.9) and rows, once per K"""
    if K not in _shared:
        q = np.ascontiguousarray(synth.normalish(9101, (M, 256, DSUB))[:, :K] * np.float32(0.0625))
        if "x" not in _shared:
            _shared["x"] = synth.normalish(9102, (N_BIG, M * DSUB)) * np.float32(0.0625)
            _shared["x"].setflags(write=False)
        q.setflags(write=False)
        _shared[K] = q
    return _shared[K], _shared["x"]


def _edge_book(K, name):
    q = _base(K)[0].copy()
    coords, _ = EDGES[name]
    q[:, PLANT] = 0
    q[:, PLANT, :len(coords)] = np.array(coords, np.float32)
    return q


def _problem(K, case, n):
    """codebook and rows of a case; the rows next to the planted centroid keep it in play"""
    q0, x0 = _base(K)
    x = x0[:n].copy()
    if case in EDGES:
        q = _edge_book(K, case)
        xr = x.reshape(n, M, DSUB)
        xr[5::97] = q[:, PLANT]                                         # rows equal to the largest centroid
        xr[11::89] = (q[:, PLANT] + q[:, 3]) * np.float32(0.5)          # and midpoints with another one
        return q, x
    s = np.float32(2.0) ** np.float32(SCALES[case])
    return np.ascontiguousarray(q0 * s), x * s


_want = {}


def _reference(K, case, n):
    key = (K, case, n)
    if key not in _want:
        q, x = _problem(K, case, n)
        _want[key] = (q, x, orc.quantize_batch(q, x, n_threads=8))
    return _want[key]


def _max_cc(q):
    return max(float(orc.dot_unrolled(c, c)) for m in range(q.shape[0]) for c in q[m])


def test_edges_are_what_they_claim():
    assert _rows_per_item(N_SMALL) == 32 and _rows_per_item(N_BIG) == 64 and N_BIG % 64 != 0
    for K in (256, 225):
        assert _max_cc(_base(K)[0]) < 0.9
        for name, (_, want) in EDGES.items():
            q = _edge_book(K, name)
            for m in range(M):
                cc = np.float32(orc.dot_unrolled(q[m, PLANT], q[m, PLANT]))
                assert cc.tobytes() == np.float32(want).tobytes(), (name, m, float(cc))
                assert max(float(orc.dot_unrolled(c, c)) for j, c in enumerate(q[m]) if j != PLANT) < 0.9
        # the scaled problems: inside the screen's range, below it, and at or above 2^100 but finite
        for name, lo, hi in (("2^-40", 2.0 ** -100, 2.0 ** -79), ("2^+40", 2.0 ** 70, 2.0 ** 100),
                             ("tiny", 0.0, 2.0 ** -100), ("huge", 2.0 ** 100, 3.0e38)):
            mc = _max_cc(_problem(K, name, 64)[0])
            assert lo < mc < hi or (name == "huge" and lo <= mc < hi), (name, mc)
    # the scale's exponent steps at 2^0 and not at 2^1
    e = lambda cc: (13 - (int(np.float32(cc).view(np.uint32) >> 23) - 127)) >> 1
    assert [e(EDGES[k][1]) for k in ("2^0-ulp", "2^0", "2^1-ulp", "2^1")] == [7, 6, 6, 6]


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _encode_and_check(ra, pq, xd, want, screen=True):
    import torch
    n = want.shape[0]
    for dt in (torch.uint8, torch.int32):
        fill = 255 if dt == torch.uint8 else -1
        out = torch.full((n + 64, M), fill, dtype=dt, device=xd.device)
        pq.quantize_batch_device(xd, out=out[:n])
        torch.cuda.synchronize()
        if screen:
            assert pq.last_encode_kernel().startswith("k_encode_mfma16"), pq.last_encode_kernel()
        got = out.cpu().numpy()
        assert (got[n:] == fill).all(), "rows past n were written"
        codes = got[:n] if dt == torch.uint8 else got[:n].view(np.uint32)
        bad = np.argwhere(codes != want)
        assert bad.size == 0, (str(dt), len(bad), bad[:5].tolist(), codes[tuple(bad[0])], want[tuple(bad[0])])


CASES = [(c, N_SMALL) for c in list(EDGES) + list(SCALES)] + [("2^0-ulp", N_BIG), ("2^-40", N_BIG), ("2^+40", N_BIG)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
@pytest.mark.parametrize("case,n", CASES)
def test_scale_edges(ra, case, n, K):
    import torch
    q, x, want = _reference(K, case, n)
    pq = ra.Pq(None, q)
    _encode_and_check(ra, pq, torch.from_numpy(x).to("cuda:0"), want, screen=case != "huge")
    pq.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 225])
def test_two_handles_alternate(ra, K):
    import torch
    qa, xa, wa = _reference(K, "2^0-ulp", N_SMALL)
    qb, xb, wb = _reference(K, "2^+40", N_SMALL)
    a, b = ra.Pq(None, qa), ra.Pq(None, qb)
    xad, xbd = torch.from_numpy(xa).to("cuda:0"), torch.from_numpy(xb).to("cuda:0")
    for pq, xd, want in ((a, xad, wa), (b, xbd, wb), (a, xad, wa), (a, xad, wa), (b, xbd, wb)):
        _encode_and_check(ra, pq, xd, want)
    a.close()
    _encode_and_check(ra, b, xbd, wb)                                   # the other handle's image went with it, not this one's
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 3])
def test_kmeans_handle_whose_centroids_change(ra, iterations):
    import torch
    K = 256
    x = _base(K)[1][:N_SMALL].copy()
    q0 = np.ascontiguousarray(x[:K].reshape(K, M, DSUB).transpose(1, 0, 2))
    want_q, want_loss = orc.kmeans_iterations(q0, x, n_iterations=iterations, n_threads=8)
    xd = torch.from_numpy(x).to("cuda:0")
    ra.launch_log(reset=True)
    q, loss = ra.kmeans_iterations(q0, xd, n_iterations=iterations)
    log = ra.launch_log(reset=True)
    assert q.tobytes() == want_q.tobytes(), "centroids differ from the oracle"
    assert loss.tobytes() == want_loss.tobytes(), (loss, want_loss)
    # the assignment stays on the kernel the dispatch gives a call beside the update kernels, at every n, so the training
    # handle's image is only marked stale by its preparations and never built
    assert "k_encode_mfma_lds3<vec4>" in log and "k_encode_mfma16" not in log and "k_build_screen_image" not in log, log
    # the moved centroids in a handle of their own: the screen kernel with their image
    pq = ra.Pq(None, q)
    _encode_and_check(ra, pq, xd, orc.quantize_batch(q, x, n_threads=8))
    pq.close()


@pytest.mark.gpu
def test_training_step_screens_with_the_moved_centroids(ra):
    """the OPQ training step: one k-means iteration moves the handle's centroids, then the same handle encodes the rotated
    rows on k_encode_mfma16 -- with the image of the NEW centroids, built in front of that launch.  A stale image (the
    initial centroids') gives other codes and another cross product."""
    import torch
    K = 256
    x = _base(K)[1][:N_SMALL].copy()
    q0 = np.ascontiguousarray(x[:K].reshape(K, M, DSUB).transpose(1, 0, 2)) * np.float32(4.0)   # another scale than the result's
    P = synth.orthonormal(9103, M * DSUB)
    want_q, want_cross = orc.opq_train_step(q0, P, x, n_threads=8)
    assert want_q.tobytes() != q0.tobytes()
    xd = torch.from_numpy(x).to("cuda:0")
    for _ in range(2):                                                  # a second handle on the same context, afresh
        ra.launch_log(reset=True)
        q, cross = ra.opq_train_step(q0, P, xd)
        log = ra.launch_log(reset=True)
        assert "k_encode_mfma16" in log and log.count("k_build_screen_image") == 1 and "k_build_screen_image x" not in log, log
        assert q.tobytes() == want_q.tobytes(), "centroids differ from the oracle"
        assert cross.tobytes() == want_cross.tobytes(), "cross product differs from the oracle"
