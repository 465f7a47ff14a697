"""k_encode_mfma16<8, 20, *> on the f16 screen: codes equal to the oracle's.

The screen rounds x and c to f16 after one power-of-two scale per subquantizer, so these inputs sit on f16's edges:
components near 65504 and in and below f16's subnormal range after the scale, codebooks whose max cc forces a scale far
from 1 (and rows whose scaled norm leaves the f16 range, which take the exact path), and near-ties at 2^-10 .. 2^-12 of
xx + max cc that the round-6 bf16 screen decided and the f16 screen must not decide wrongly.  Both index widths; the
auto dispatch and variant 9 reach the screen body."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

pytestmark = pytest.mark.gpu

M, K, DSUB = 3, 256, 20


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _check(ra, q, x, dtypes=(np.uint8, np.uint32), variants=(0, 9)):
    q = np.ascontiguousarray(q, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    for dt in dtypes:
        want = orc.quantize_batch(q, x, dtype=dt)
        for v in variants:
            pq = ra.Pq(None, q)
            if v:
                pq.set_encode_variant(v)
            got = pq.quantize_batch(x, dtype=dt)
            assert pq.last_encode_kernel().startswith("k_encode_mfma16"), pq.last_encode_kernel()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (dt.__name__, v, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _rows(n, seed):
    return synth.normalish(seed, (n, M * DSUB))


@pytest.mark.parametrize("scale", [2.0 ** -45, 1e-9, 3e-3, 41.0, 1e7, 2.0 ** 45])
def test_codebook_scales(ra, scale):
    # max cc from ~2^-90 to ~2^95: the per-subquantizer scale is far from 1 in both directions
    sc = np.float32(scale)
    q = synth.normalish(7101, (M, K, DSUB)) * sc
    q[1] *= np.float32(0.01)                                  # a different scale per subquantizer
    _check(ra, q, _rows(6000 + 11, 7102) * sc)


def test_f16_range_edges(ra):
    q = synth.normalish(7103, (M, K, DSUB))
    x = _rows(8000 + 5, 7104)
    x[:1000] *= np.float32(2.0 ** -12)                         # scaled components below f16's normal range
    x[1000:2000] *= np.float32(2.0 ** -26)                     # ... and below its subnormal range
    x[2000:3000, ::2] *= np.float32(2.0 ** -20)                # mixed: half the components in the subnormal range
    # scaled components near 65504 and beyond (rows past kScreenMaxXX take the exact path)
    for i, r in enumerate(range(3000, 5000)):
        x[r] *= np.float32(2.0 ** (4 + i % 12))
    q2 = q.copy()
    q2[0, :64, 1:] *= np.float32(2.0 ** -24)                   # centroids with tiny components next to one big one
    q2[2, 100:110] = np.float32(0)
    _check(ra, q2, x)


def test_near_ties_between_the_bounds(ra):
    # midpoints of two centroids moved towards one of them by 2^-12 .. 2^-8 of xx + max cc (the round-6 screen's
    # threshold was 2^-12, the f16 screen's is 0x1.2p-9): some are decided by the screen, others must not be
    q = synth.normalish(7105, (M, K, DSUB))
    cc = (q.astype(np.float64) ** 2).sum(2).max(1)
    rng = np.random.RandomState(7106)
    rows = []
    for i in range(6000):
        r = np.empty(M * DSUB, np.float32)
        for m in range(M):
            a, b = rng.choice(K, 2, replace=False)
            mid = (q[m, a].astype(np.float64) + q[m, b]) / 2
            d = q[m, b].astype(np.float64) - q[m, a]
            e = 2.0 ** -rng.uniform(8, 13) * (float(mid @ mid) + cc[m])
            t = e / max(float(d @ d), 1e-30) / 2 * (1 if i % 2 else -1)
            r[m * DSUB:(m + 1) * DSUB] = (mid + t * d).astype(np.float32)
        rows.append(r)
    _check(ra, q, np.stack(rows))


def test_many_candidates_exact_path(ra):
    # clusters of near-identical centroids in one lane group and across lane groups: rows with more candidates than
    # the in-loop resolution takes go to the exact path
    q = synth.normalish(7107, (M, K, DSUB))
    rng = np.random.RandomState(7108)
    for m in range(M):
        for base in range(0, K, 32):
            for j in (1, 2, 3, 16, 17):
                q[m, base + j] = q[m, base] + rng.normal(0, 1e-3, DSUB).astype(np.float32)
    x = _rows(5000 + 3, 7109)
    for r in range(2500):
        m = r % M
        x[r, m * DSUB:(m + 1) * DSUB] = q[m, 32 * (r % 8)] + rng.normal(0, 1e-2, DSUB).astype(np.float32)
    _check(ra, q, x)
