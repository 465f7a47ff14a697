"""k_encode_mfma16<8, 20, *>: the bf16 screen must leave every code equal to the oracle's.

The screen decides a row on the matrix cores only when its second-best screening value is more than the error bound
above the best one; rows with two to four candidates in different lane groups are resolved with
exact arithmetic in the loop (e.g. the tie of centroids 3 and 200 below), everything else goes to the exact path after
it (e.g. the triple 0 / 128 / 255, where 0 and 128 share a lane group).  These inputs sit on and around the
bound: midpoints between two centroids nudged by ulps and by multiples of the bound, exact ties, duplicated codebooks,
rows on a centroid, subnormals, norms beside kBigNorm, widely spread centroid norms, a padded codebook (K < 256) and
the usual data distributions, at both index widths, with a ragged n and a strided row layout.  Variants 0 and 9 reach
the screen body; variant 4 (the FP32 kernel K1) is run on the same inputs as an independent device path."""
import numpy as np
import pytest

import synth
from oracle import pq_oracle as orc

pytestmark = pytest.mark.gpu

M, K, DSUB = 3, 256, 20
BIG = np.float32(1.2676506e30)   # kBigNorm = 2^100
REL = 2.0 ** -12                 # kScreenRel


@pytest.fixture(scope="module")
def ra():
    import reductive_amd
    reductive_amd.lib()
    return reductive_amd


def _check(ra, q, x, dtypes=(np.uint8, np.uint32), variants=(0, 9, 4)):
    for dt in dtypes:
        want = orc.quantize_batch(q, np.ascontiguousarray(x), dtype=dt)
        for v in variants:
            pq = ra.Pq(None, q)
            if v:
                pq.set_encode_variant(v)
            got = pq.quantize_batch(x, dtype=dt)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (dt.__name__, v, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _rows(n, seed):
    return synth.normalish(seed, (n, M * DSUB))


def test_normal_rows_normal_codebook(ra):
    _check(ra, synth.normalish(7001, (M, K, DSUB)), _rows(20_000 + 13, 7002))


def test_uniform_rows_and_codebook(ra):
    rng = np.random.RandomState(7003)
    q = rng.random_sample((M, K, DSUB)).astype(np.float32)
    x = rng.random_sample((20_000 + 7, M * DSUB)).astype(np.float32)
    _check(ra, q, x)


def test_kmeans_trained_codebook(ra):
    x = _rows(8192, 7004)
    q = synth.normalish(7005, (M, K, DSUB)) * np.float32(0.5)
    q, _ = orc.kmeans_iterations(q, x, n_iterations=3)
    _check(ra, q, _rows(10_000 + 5, 7006))


def test_midpoints_ulps_and_bound_multiples(ra):
    q = synth.normalish(7007, (M, K, DSUB))
    rng = np.random.RandomState(7008)
    rows = []
    for i in range(4000):
        r = np.empty(M * DSUB, np.float32)
        for m in range(M):
            a, b = rng.choice(K, 2, replace=False)
            mid = (q[m, a] + q[m, b]) / np.float32(2)
            d = q[m, b] - q[m, a]
            sel = i % 4
            if sel == 0:      # 0, 1, 2, ... ulps off the midpoint, towards either centroid
                steps = (i // 4) % 5
                towards = np.float32(np.inf) if (i // 20) % 2 else np.float32(-np.inf)
                for _ in range(steps):
                    mid = np.nextafter(mid, towards)
            else:             # multiples of the bound along the segment
                xx = float(mid @ mid)
                e = REL * (xx + float((q[m] ** 2).sum(1).max()))
                k = [0.25, 0.5, 1, 2, 4, 8][(i // 4) % 6] * (1 if sel == 1 else -1)
                mid = (mid + np.float32(k * e / max(float(d @ d), 1e-30) / 2) * d).astype(np.float32)
            r[m * DSUB:(m + 1) * DSUB] = mid
        rows.append(r)
    _check(ra, q, np.stack(rows))


def test_ties_duplicates_and_rows_on_centroids(ra):
    q = synth.normalish(7009, (M, K, DSUB))
    q[0, 200] = q[0, 3]
    q[1, 255] = q[1, 0]
    q[1, 128] = q[1, 0]
    q[2] = q[2, 17]                       # fully duplicated sub-codebook: index 0 must win everywhere
    x = _rows(3000 + 1, 7010)
    x[:500, :DSUB] = q[0, 3]
    x[500:1000, DSUB:2 * DSUB] = q[1, 0]
    rng = np.random.RandomState(7011)
    for r in range(1000, 2000):
        m = rng.randint(M)
        x[r, m * DSUB:(m + 1) * DSUB] = q[m, rng.randint(K)]   # D = 0 rows
    _check(ra, q, x)


def test_subnormals_and_norms_beside_kbignorm(ra):
    q = synth.normalish(7012, (M, K, DSUB))
    x = _rows(4000 + 3, 7013)
    tiny = np.float32(1e-40)
    x[:500] *= tiny                                          # subnormal components
    x[500:1000, ::3] = tiny
    for i, r in enumerate(range(1000, 3000)):               # ||x||^2 just below and above 2^100
        f = np.float32(np.sqrt(float(BIG) / max(float(x[r] @ x[r]) / M, 1e-30)))
        f = np.nextafter(f, np.float32(0 if i % 2 else np.inf))
        x[r] *= f * np.float32(1 + (i % 5 - 2) * 1e-7)
    qs = q.copy()
    qs[0, :16] *= np.float32(1e-30)                         # subnormal products
    _check(ra, qs, x)


def test_centroid_norms_spread(ra):
    rng = np.random.RandomState(7014)
    q = synth.normalish(7015, (M, K, DSUB))
    scale = np.float32(10.0) ** rng.uniform(-1.5, 3.0, (M, K, 1)).astype(np.float32)   # ||c||^2 ~ 1e-3 .. 1e6
    q = (q * scale / np.float32(np.sqrt(DSUB))).astype(np.float32)
    x = (_rows(10_000 + 9, 7016) * np.float32(10.0) ** rng.uniform(-1.5, 3.0, (10_009, 1)).astype(np.float32)
         / np.float32(np.sqrt(DSUB))).astype(np.float32)
    _check(ra, q, x)


def test_padded_codebook_and_strided_rows(ra):
    q = synth.normalish(7017, (M, 250, DSUB))                # T = 8 with 6 padding centroids
    wide = _rows(6000 + 29, 7018)
    wide = np.concatenate([wide, wide[:, :7]], axis=1)      # row stride 67 floats
    x = wide[:, :M * DSUB]
    assert not x.flags["C_CONTIGUOUS"]
    _check(ra, q, x)
    q2 = synth.normalish(7019, (M, K, DSUB))
    _check(ra, q2, x)
