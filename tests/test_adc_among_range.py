"""CPU side of the ADC range search among given rows: header, EXPORTS, SIGNATURES, library and rust/pqhip_ffi.rs name
the two entry points and the option, neither name falls under the grammar of the 24 search and range symbols, a null
codebook is EINVAL, and the refusals of the Python layer are raised before the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqhip_adc_among_range_f32_dev", "pqhip_adc_ip_among_range_f32_dev")
OPTION = "adc_among_range_wgs_per_query"


@pytest.mark.parametrize("name", NAMES)
def test_the_name_is_registered_everywhere_and_a_null_codebook_is_einval(name):
    from reductive_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    assert "int32_t %s(" % name in hdr and "pub fn %s(" % name in ffi
    assert name in _lib.EXPORTS and not re.match("pqhip_adc_(ip_)?(search|range)", name)
    among = _lib.SIGNATURES[name.replace("_range", "")][1]
    assert _lib.SIGNATURES[name][1] == among[:16] + _lib.SIGNATURES["pqhip_adc_range_f32_dev"][1][-6:]
    assert '"%s"' % OPTION in hdr and '"%s"' % OPTION in ffi
    assert '{"%s", &o.%s}' % (OPTION, OPTION) in open(os.path.join(ROOT, "reductive_amd", "csrc", "pqhip_ctx.hip")).read()
    f = getattr(_lib.lib(), name)
    buf = (ctypes.c_int64 * 16)()
    p, z = ctypes.addressof(buf), ctypes.c_void_p(0)
    assert f(None, 0, None, 0, None, 1, 0, 0, None, None, 0, None, 0, None, 0, None, None, None, None, None, 0, z) == _lib.EINVAL
    assert f(None, 0, p, 1, p, 1, 4, 2, p, p, 2, None, 0, None, 0, None, p, p, p, p, 1, z) == _lib.EINVAL


def test_refusals_are_raised_before_the_library(monkeypatch):
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal, qmatrix
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    packed, tables = torch.zeros((8, 2), dtype=torch.uint8), torch.zeros((2, 3, 16))
    off, probes = torch.zeros(2, dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ra.PanicError, match="packed rows have no range call"):
        pq.adc_range_batch_device(packed, tables, 0.5)
    with pytest.raises(ra.PanicError, match="packed rows have no range call"):
        pq.adc_range_lists_batch_device(packed, tables, off, probes, 0.5)
    with pytest.raises(ra.PanicError, match="image_bits must be 8 or 16"):
        pq.adc_range_batch_device(torch.zeros((8, 3), dtype=torch.uint8), tables, 0.5, image_bits=4)
    qm = qmatrix.QuantizedMatrix(pq, np.zeros((8, 3), np.uint8), device="cpu")
    pk = qm._with_codes(qm.codes[:, :2], True)                          # what pack4() returns, without the device call
    q = np.zeros((2, 3), np.float32)
    pm = qmatrix.PartitionedMatrix.__new__(qmatrix.PartitionedMatrix)    # packed: refused before anything of it is read
    pm.packed4 = True
    for call, what, more in ((pk.within, "within", ()), (pk.similar_above, "similar_above", ()), (pm.within, "within", (2,)),
                             (pm.similar_above, "similar_above", (2,))):
        for screen in (True, "u16"):
            with pytest.raises(ra.PanicError, match=re.escape("%s(screen=True) does not read 4-bit packed codes" % what)):
                call(q, 0.5, *more, screen=screen)
    for call, what in ((pk.within_among, "within_among"), (pk.similar_above_among, "similar_above_among")):
        with pytest.raises(ra.PanicError, match=re.escape("%s() does not read 4-bit packed codes" % what)):
            call(q, np.zeros(4, np.int64), 0.5)
