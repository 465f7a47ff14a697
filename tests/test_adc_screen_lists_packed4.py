"""CPU tests of the one-hot screen over 4-bit packed codes in probed lists (pqhip_adc_screen_lists_packed4_f32_dev;
DESIGN.md §5j): the name is registered everywhere with the u8 list screen's signature, packed4 is a trailing keyword that
defaults to False, and the refusals of the Python layer are raised before the library."""
import inspect
import os

import pytest

NAME = "pqhip_adc_screen_lists_packed4_f32_dev"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_name_is_registered_everywhere_with_the_list_screens_signature():
    from reductive_amd import _lib, pq
    header = open(os.path.join(ROOT, "include", "pqhip.h")).read()
    assert "int32_t %s(" % NAME in header
    assert NAME in _lib.EXPORTS and _lib.SIGNATURES[NAME] == _lib.SIGNATURES["pqhip_adc_screen_lists_f32_dev"]
    assert "pub fn %s(" % NAME in open(os.path.join(ROOT, "rust", "pqhip_ffi.rs")).read()
    for fn in (pq.Pq.adc_screen_lists_device, pq.Pq.adc_search_lists_batch_device, pq.Pq._adc_screen_lists):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "packed4" and params[-1].default is False
    args = [None, 0, None, 1, None, 1, 8, 4, None, None, 1, None, 1, 1, 0, None, None, None, None, 0, None]
    assert getattr(_lib.lib(), NAME)(*args) == _lib.EINVAL                 # a null codebook


def test_refusals_are_raised_before_the_library(monkeypatch):
    import numpy as np
    import torch
    import reductive_amd as ra
    from reductive_amd import _marshal, qmatrix
    monkeypatch.setattr(_marshal, "run", lambda *a, **k: pytest.fail("the library was reached"))
    monkeypatch.setattr(_marshal, "launch", lambda *a, **k: pytest.fail("the library was reached"))
    pq = ra.Pq.__new__(ra.Pq)
    pq.quantized_len, pq.n_quantizer_centroids = (lambda: 3), (lambda: 16)
    tables, off, probes = torch.zeros((2, 3, 16)), torch.zeros(3, dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int64)
    unpacked = torch.zeros((8, 3), dtype=torch.uint8)
    with pytest.raises(ra.PanicError, match="4-bit packed codes must be"):     # unpacked rows are not packed rows
        pq.adc_screen_lists_device(unpacked, tables, off, probes, 0.5, packed4=True)
    with pytest.raises(ra.PanicError, match="4-bit packed codes must be"):
        pq.adc_search_lists_batch_device(unpacked, tables, off, probes, 1, packed4=True)
    pq.n_quantizer_centroids = lambda: 32                                      # K > 16 has no packed form
    with pytest.raises(ra.PanicError):
        pq.adc_screen_lists_device(torch.zeros((8, 2), dtype=torch.uint8), torch.zeros((2, 3, 32)), off, probes, 0.5, packed4=True)
    pq.n_quantizer_centroids = lambda: 16
    pm = qmatrix.PartitionedMatrix.__new__(qmatrix.PartitionedMatrix)          # an unpacked matrix: refused before a field is read
    pm.packed4 = False
    for call in (pm.nearest, pm.most_similar):
        with pytest.raises(ra.PanicError, match=r"pack4\(\) first"):
            call(np.zeros(12, np.float32), 1, 1, screen="onehot")
