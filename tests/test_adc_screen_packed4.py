"""CPU tests of the one-hot screen over 4-bit packed codes (pqhip_adc_screen_packed4_f32_dev): the name is
registered everywhere with the u8 screen's signature, a null codebook is refused, and the two refusals of the Python
layer are raised before the library."""
import os

import pytest

NAME = "pqhip_adc_screen_packed4_f32_dev"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_name_is_registered_everywhere_and_a_null_codebook_is_refused():
    from reductive_amd import _lib
    header = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    assert "int32_t %s(" % NAME in header and "pad nibble" in header
    assert NAME in _lib.EXPORTS and _lib.SIGNATURES[NAME] == _lib.SIGNATURES["pqhip_adc_screen_f32_dev"]
    assert "pub fn %s(" % NAME in open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    assert getattr(_lib.lib(), NAME)(None, 0, None, 1, None, 1, 8, 4, None, 0, None, None, None, None, 0, None) == _lib.EINVAL


def test_refusals_are_raised_before_the_library(monkeypatch):
    import numpy as np
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal, qmatrix
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    packed, tables = torch.zeros((8, 2), dtype=torch.uint8), torch.zeros((2, 3, 16))
    with pytest.raises(ra.PanicError, match="image_bits=8"):
        pq.adc_screen_device(packed, tables, 0.5, image_bits=16, packed4=True)
    with pytest.raises(ra.PanicError, match="image_bits=8"):
        pq.adc_search_batch_device(packed, tables, 1, image_bits=16, packed4=True)
    with pytest.raises(ra.PanicError, match="4-bit packed codes must be"):     # unpacked rows are not packed rows
        pq.adc_screen_device(torch.zeros((8, 3), dtype=torch.uint8), tables, 0.5, packed4=True)
    qm = qmatrix.QuantizedMatrix(pq, np.zeros((8, 3), np.uint8), device="cpu")
    with pytest.raises(ra.PanicError, match=r"pack4\(\) first"):
        qm.nearest(np.zeros(12, np.float32), 1, screen="onehot")
