"""The residual and row-term kernels on the GPU (include/pqhip.h: pqhip_residuals_f32_dev, pqhip_residual_terms_f32_dev;
Pq.residuals_device, Pq.residual_terms_device).
Residuals: exact against x - c[assign] in numpy f32 for d in {1, 3, 4, 60, 300, 301}, bases 0 / 1 / 3 floats off a 16-byte
boundary, padded row strides with guard floats between the rows, a bad list id (a zero row and the range flag).
Terms: exact, as bit patterns, against tests/residual_terms_ref.py for (M, ds) in {(1, 1), (1, 5), (15, 4), (15, 20), (16, 1),
(100, 3)} x K in {2, 3, 16, 256} x n in {1, 65, 5000}, padded code strides, codebooks and centroids with +-0 and mixed
magnitudes, a code >= K (entry 0 and the flag), a bad list id (+0 and the flag), an OPQ codebook (PQHIP_EUNSUPPORTED,
nothing written).
Agreement with the host route on the fixture of tests/test_gpu_qmatrix_add.py: |t_dev - t_host| <= 2^-23 |t_host| + 2^-40 S,
S = sum_j (r^2 + |2 c r|).  The bound is derived, not measured: each value is one f32 rounding (2^-24 relative each) of an
f64 sum of d + M terms whose accumulated error is at most (d + M) 2^-53 S; 2^-40 covers d + M <= 8,192
(tests/test_index_build.py checks it on the CPU with torch's float64 sum standing in for the host route)."""
import ctypes

import numpy as np
import pytest

import synth
from residual_terms_ref import abs_sum, ref_terms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import os
    import reductive_amd
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    reductive_amd.lib()
    return reductive_amd


@pytest.fixture(scope="module")
def pq(ra):
    return ra.Pq(None, synth.normalish(6000, (2, 16, 4)))


def strided(rows, shift, stride, fill):
    """rows [n, d] f32 on the device inside a buffer of `fill`: base `shift` floats off a 16-byte boundary, row stride
    `stride` floats -> (buffer, view)"""
    import torch
    n, d = rows.shape
    buf = torch.full((shift + n * stride + 8,), fill, dtype=torch.float32, device="cuda")
    view = buf[shift:shift + n * stride].view(n, stride)[:, :d]
    view.copy_(torch.from_numpy(rows))
    assert n == 0 or view.data_ptr() % 16 == 4 * (shift % 4)
    return buf, view


def mixed(seed, shape):
    """f32 values of mixed magnitude with some +0 and -0"""
    rng = np.random.default_rng(seed)
    v = (synth.normalish(seed, shape) * np.exp2(rng.integers(-12, 12, shape))).astype(np.float32)
    z = rng.random(shape)
    v[z < 0.03] = np.float32(0.0)
    v[z > 0.97] = np.float32(-0.0)
    return v


@pytest.mark.parametrize("d", [1, 3, 4, 60, 300, 301])
def test_residuals_are_one_subtraction(ra, pq, d):
    import torch
    n_lists = 7
    for n in (1, 17, 1000):
        for shift_x, shift_o, shift_c, pad in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 3, 0, 5), (0, 0, 1, 0), (1, 3, 2, 3), (0, 0, 0, 4)):
            seed = 6100 + d * 10 + n + shift_x + shift_o + pad
            x, cen = mixed(seed, (n, d)), mixed(seed + 1, (n_lists, d))
            assign = np.random.default_rng(seed).integers(0, n_lists, n)
            want = x - cen[assign]
            _, xd = strided(x, shift_x, d + pad, 7.0)
            obuf, od = strided(np.full((n, d), 9.0, np.float32), shift_o, d + pad, 9.0)
            cbuf = torch.zeros(shift_c + n_lists * d, dtype=torch.float32, device="cuda")
            cd = cbuf[shift_c:].view(n_lists, d)
            cd.copy_(torch.from_numpy(cen))
            out = pq.residuals_device(xd, torch.from_numpy(assign).cuda(), cd, out=od, check=True)
            assert out.data_ptr() == od.data_ptr()
            got = obuf.cpu().numpy()
            rows = got[shift_o:shift_o + n * (d + pad)].reshape(n, d + pad)
            assert rows[:, :d].tobytes() == want.tobytes(), (d, n, shift_x, shift_o, shift_c, pad)
            assert np.all(rows[:, d:] == 9.0) and np.all(got[:shift_o] == 9.0) and np.all(got[shift_o + n * (d + pad):] == 9.0)
    # without out=, and against the torch expression the host route uses
    x, cen = mixed(6190 + d, (1000, d)), mixed(6191 + d, (n_lists, d))
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cen).cuda()
    ad = torch.from_numpy(np.random.default_rng(d).integers(0, n_lists, 1000)).cuda()
    ra.launch_log(reset=True)
    got = pq.residuals_device(xd, ad, cd)
    assert "k_residuals" in ra.launch_log(reset=True)
    assert torch.equal(got.view(torch.int32), (xd - cd[ad]).view(torch.int32))
    assert tuple(pq.residuals_device(xd[:0], ad[:0], cd).shape) == (0, d)


@pytest.mark.parametrize("bad", [-1, 7])
def test_residuals_of_a_bad_list_id_are_a_zero_row_and_the_flag(ra, pq, bad):
    import torch
    n, d, n_lists = 100, 60, 7
    x, cen = mixed(6200, (n, d)), mixed(6201, (n_lists, d))
    assign = np.random.default_rng(6202).integers(0, n_lists, n)
    good = assign.copy()
    assign[41] = bad
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cen).cuda()
    out = torch.full((n, d), 9.0, device="cuda")
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        pq.residuals_device(xd, torch.from_numpy(assign).cuda(), cd, out=out, check=True)
    want = x - cen[good]
    want[41] = 0.0
    assert out.cpu().numpy().tobytes() == want.tobytes()
    pq.residuals_device(xd, torch.from_numpy(good).cuda(), cd, out=out, check=True)       # the flag is down again


def terms_case(ra, M, ds, K, seed):
    q = mixed(seed, (M, K, ds))
    q[0, 0, 0] = np.float32(-0.0)
    return ra.Pq(None, q), q


@pytest.mark.parametrize("K", [2, 3, 16, 256])
@pytest.mark.parametrize("M,ds", [(1, 1), (1, 5), (15, 4), (15, 20), (16, 1), (100, 3)])
def test_terms_equal_the_reference_bit_for_bit(ra, M, ds, K):
    import torch
    n_lists, d = 11, M * ds
    rpq, q = terms_case(ra, M, ds, K, 6300 + M * 7 + ds + K)
    cen = mixed(6301 + M + ds + K, (n_lists, d))
    cd = torch.from_numpy(cen).cuda()
    rng = np.random.default_rng(6302 + M + K)
    ra.launch_log(reset=True)
    for n, pad in ((1, 0), (65, 3), (5000, 0), (5000, 1)):
        codes = rng.integers(0, K, (n, M)).astype(np.uint8)
        assign = rng.integers(0, n_lists, n)
        cbuf = torch.full((n, M + pad), 255, dtype=torch.uint8, device="cuda")
        cv = cbuf[:, :M]
        cv.copy_(torch.from_numpy(codes))
        got = rpq.residual_terms_device(cv, torch.from_numpy(assign).cuda(), cd, check=True)
        want = ref_terms(q, codes, assign, cen)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (M, ds, K, n, pad)
    assert "k_residual_terms" in ra.launch_log(reset=True)
    # out=, and guard floats around it
    buf = torch.full((n + 8,), 9.0, device="cuda")
    rpq.residual_terms_device(cv, torch.from_numpy(assign).cuda(), cd, out=buf[4:4 + n], check=True)
    g = buf.cpu().numpy()
    assert g[4:4 + n].tobytes() == want.tobytes() and np.all(g[:4] == 9.0) and np.all(g[4 + n:] == 9.0)
    # a bad list id: +0 and the flag
    a2 = assign.copy()
    a2[0], a2[n // 2] = -1, n_lists
    with pytest.raises(ra.PanicError, match="index out of bounds"):
        rpq.residual_terms_device(cv, torch.from_numpy(a2).cuda(), cd, out=buf[4:4 + n], check=True)
    assert buf[4:4 + n].cpu().numpy().tobytes() == ref_terms(q, codes, a2, cen).tobytes()
    assert buf[4].cpu().numpy().tobytes() == np.float32(0.0).tobytes()
    # a code >= K reads entry 0 and raises the flag
    if K < 256:
        c2 = codes.copy()
        c2[3, M - 1], c2[n - 1, 0] = K, 255
        with pytest.raises(ra.PanicError, match="index out of bounds"):
            got = rpq.residual_terms_device(torch.from_numpy(c2).cuda(), torch.from_numpy(assign).cuda(), cd, out=buf[4:4 + n], check=True)
        assert buf[4:4 + n].cpu().numpy().tobytes() == ref_terms(q, c2, assign, cen).tobytes()
    assert tuple(rpq.residual_terms_device(cv[:0], torch.from_numpy(assign[:0]).cuda(), cd, check=True).shape) == (0,)


def test_terms_of_an_opq_codebook_are_unsupported_and_write_nothing(ra):
    import torch
    from reductive_amd import _lib
    M, ds, K, n = 3, 4, 16, 50
    P = np.linalg.qr(synth.normalish(6400, (M * ds, M * ds)).astype(np.float64))[0].astype(np.float32)
    opq = ra.Pq(P, synth.normalish(6401, (M, K, ds)))
    codes = torch.zeros((n, M), dtype=torch.uint8, device="cuda")
    assign = torch.zeros(n, dtype=torch.int64, device="cuda")
    cen = torch.zeros((2, M * ds), device="cuda")
    out = torch.full((n,), 9.0, device="cuda")
    z = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    trm = ra.lib().pqhip_residual_terms_f32_dev
    ra.launch_log(reset=True)
    cb = opq._cb()
    ra.launch_log(reset=True)
    assert trm(cb, 0, codes.data_ptr(), n, M, assign.data_ptr(), cen.data_ptr(), 2, out.data_ptr(), z) == _lib.EUNSUPPORTED
    assert "k_residual_terms" not in ra.launch_log(reset=True)
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    with pytest.raises(ra.PanicError, match="projection"):
        opq.residual_terms_device(codes, assign, cen)
    # the other statuses, on a plain codebook
    pq = ra.Pq(None, synth.normalish(6401, (M, K, ds)))
    cb = pq._cb()
    c, a, ce, o = codes.data_ptr(), assign.data_ptr(), cen.data_ptr(), out.data_ptr()
    assert trm(cb, 0, c, -1, M, a, ce, 2, o, z) == _lib.EINVAL
    assert trm(cb, 0, c, n, M, a, ce, 0, o, z) == _lib.EINVAL
    assert trm(cb, 7, c, n, M, a, ce, 2, o, z) == _lib.ENODEV
    assert trm(cb, 0, None, 0, M, None, None, 2, None, z) == _lib.OK
    assert trm(cb, 0, None, n, M, a, ce, 2, o, z) == _lib.EINVAL
    assert trm(cb, 0, c, n, M, a, ce, 2, None, z) == _lib.EINVAL
    assert trm(cb, 0, c, n, M - 1, a, ce, 2, o, z) == _lib.ESHAPE
    res = ra.lib().pqhip_residuals_f32_dev
    x = torch.zeros((n, M * ds), device="cuda")
    xo = torch.zeros((n, M * ds), device="cuda")
    assert res(cb, 0, x.data_ptr(), n, 0, 12, a, ce, 2, xo.data_ptr(), 12, z) == _lib.EINVAL
    assert res(cb, 7, x.data_ptr(), n, 12, 12, a, ce, 2, xo.data_ptr(), 12, z) == _lib.ENODEV
    assert res(cb, 0, x.data_ptr(), n, (1 << 20) + 1, 1 << 21, a, ce, 2, xo.data_ptr(), 1 << 21, z) == _lib.EUNSUPPORTED
    assert res(cb, 0, None, 0, 12, 12, None, ce, 2, None, 12, z) == _lib.OK
    assert res(cb, 0, None, n, 12, 12, a, ce, 2, xo.data_ptr(), 12, z) == _lib.EINVAL
    assert res(cb, 0, x.data_ptr(), n, 12, 11, a, ce, 2, xo.data_ptr(), 12, z) == _lib.ESHAPE
    assert res(cb, 0, x.data_ptr(), n, 12, 12, a, ce, 2, xo.data_ptr(), 11, z) == _lib.ESHAPE


@pytest.mark.parametrize("name", ["base", "wide"])
def test_terms_agree_with_the_host_route_within_the_derived_bound(ra, name):
    """the fixture of tests/test_gpu_qmatrix_add.py (recipe copied): the old rows' residual codes and their terms by the
    host route's helper, against the kernel on the same codes"""
    import torch
    from oracle import pq_oracle as orc
    from reductive_amd import qmatrix
    CONFIGS = {"base": (15, 4, 24), "lists300": (15, 4, 300), "wide": (15, 20, 24)}
    N, B = 30011, 4099
    M, dsub, n_lists = CONFIGS[name]
    d, seed = M * dsub, 7000 + 10 * sorted(CONFIGS).index(name)
    rq = synth.normalish(seed + 1, (M, 256, dsub)) * np.float32(0.7)
    rpq = ra.Pq(None, rq)
    centres = synth.normalish(seed + 2, (40, d)) * np.float32(3.0)
    x = (centres[np.random.default_rng(seed + 3).integers(0, 40, N + B)] + synth.normalish(seed + 4, (N + B, d))).astype(np.float32)
    centroids = np.ascontiguousarray(x[np.random.default_rng(seed + 5).choice(N, n_lists, replace=False)])
    assign = orc.cluster_assignments(centroids, x).astype(np.int64)
    xd, cd, ad = torch.from_numpy(x[:N]).cuda(), torch.from_numpy(centroids).cuda(), torch.from_numpy(assign[:N]).cuda()
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    t_host = qmatrix._residual_codes_terms(rpq, xd, cd[ad], codes).cpu().numpy().astype(np.float64)
    t_dev = rpq.residual_terms_device(codes, ad, cd, check=True).cpu().numpy()
    codes_h = codes.cpu().numpy()
    assert t_dev.tobytes() == ref_terms(rq, codes_h, assign[:N], centroids).tobytes()
    S = abs_sum(rq, codes_h, assign[:N], centroids)
    err = np.abs(t_dev.astype(np.float64) - t_host)
    bound = 2.0 ** -23 * np.abs(t_host) + 2.0 ** -40 * S
    print("max |t_dev - t_host| / bound = %.3g; rows that differ: %d of %d" % ((err / bound).max(), int((err > 0).sum()), N))
    assert (err <= bound).all()
