"""CPU tests of the batch route of the exact list searches: its two pure rules, the names, the early argument checks."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pqhip_flat_screen_lists_f32_dev"


def test_sample_and_fallback_rules():
    from reductive_amd import pq as rules
    for n_rows, n_lists in ((1025, 7), (10_000_000, 1024), (5, 9)):
        for n_probe in (1, 3, 8, 64, 2000):
            last = 0
            for k in (1, 10, 100, 1024):
                s = rules.flat_lists_batch_sample(n_rows, n_lists, n_probe, k)
                assert 1 <= s <= n_probe and s >= last
                last = s
    assert rules.flat_lists_batch_sample(10_000_000, 1024, 64, 10) < 64
    f = rules.flat_lists_batch_fraction()
    assert 0.0 < f <= 1.0
    expected = 100 * 10_000 * 8 / 64
    assert not rules.flat_lists_batch_falls_back(int(f * expected), 10_000, 64, 8, 100)
    assert rules.flat_lists_batch_falls_back(int(f * expected) + 1, 10_000, 64, 8, 100)


def test_the_entry_point_is_named_everywhere_and_a_null_codebook_is_einval():
    import reductive_amd
    from reductive_amd import _lib
    for path in ("include/pqhip.h", "reductive_amd/_lib.py", "rust/pqhip_ffi.rs", "reductive_amd/csrc/pqhip_flat_screen_lists.hip"):
        with open(os.path.join(ROOT, path)) as f:
            assert NAME in f.read(), path
    with open(os.path.join(ROOT, "reductive_amd/csrc/Makefile")) as f:
        assert re.search(r"\bpqhip_flat_screen_lists\b", f.read())
    if not os.path.exists(reductive_amd.lib_path()):
        reductive_amd.build()
    args = [None, 0, None, 1, 4, None, 4, 8, 4, 4, None, None, 2, None, 1, 1, 0, 0, None, None, None, 0, None]
    assert getattr(_lib.lib(), NAME)(*args) == _lib.EINVAL


def test_wrappers_check_their_arguments_first_and_screen_defaults_to_false():
    import torch
    from reductive_amd import PanicError, Pq
    from reductive_amd.qmatrix import PartitionedFlatMatrix
    pq = Pq(None, np.zeros((1, 2, 2), np.float32))
    q, x = torch.zeros(2, 4), torch.zeros(8, 4)
    off, pr = torch.tensor([0, 8]), torch.zeros(2, 1, dtype=torch.int64)
    for call in (lambda: pq.flat_screen_lists_device(q, x, off, pr, 1.0),                       # CPU tensors
                 lambda: pq.flat_screen_lists_device(q, torch.zeros(8, 5), off, pr, 1.0),      # length mismatch
                 lambda: pq.flat_screen_lists_device(torch.zeros(2, 2049), torch.zeros(8, 2049), off, pr, 1.0),
                 lambda: pq.flat_screen_lists_device(q, x, off, pr[:1], 1.0),                  # one probe row per query
                 lambda: pq.flat_range_lists_batch_device(q, x, off, pr.float(), 1.0, x_exp=0),
                 lambda: pq.flat_search_lists_batch_device(q, x, off, pr, 0),
                 lambda: pq.flat_search_lists_batch_device(q, x, off, pr, 1025)):
        with pytest.raises(PanicError):
            call()
    for name in ("nearest", "most_similar", "within", "similar_above"):
        assert inspect.signature(getattr(PartitionedFlatMatrix, name)).parameters["screen"].default is False
