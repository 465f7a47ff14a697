"""reductive_amd/_marshal.py without a GPU: the row stride of small tensors, the shapes the argument normalisers accept
and refuse (with the texts the wrappers always raised), the argument grammar of the 24 search and range entry points
against the signature table, and the table against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from reductive_amd import _lib, _marshal as m
from reductive_amd.pq import PanicError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows", [0, 1, 2])
def test_row_stride(rows):
    t = torch.zeros((rows, 5))
    wide = torch.zeros((rows, 8))[:, :5]
    tall = torch.zeros((2 * rows, 5))[::2]
    assert m.row_stride(t, rows, 5) == 5
    assert m.row_stride(wide, rows, 5) == 8
    assert m.row_stride(tall, rows, 5) == (10 if rows > 1 else max(tall.stride(0), 5))
    # torch may report any stride for a single row: the width is the floor
    one = torch.zeros((1, 5)).as_strided((1, 5), (1, 1))
    assert m.row_stride(one, 1, 5) == 5
    # the count is the caller's: a matrix of two rows passed as one
    assert m.row_stride(torch.zeros((2, 3)), 1, 7) == 7 and m.row_stride(torch.zeros((2, 3)), 2, 7) == 3


def test_addresses():
    t = torch.zeros(3)
    assert m.ptr_or_none(None) is None and m.ptr_or_none(t, 0) is None
    assert m.ptr_or_none(t) == m.ptr_or_none(t, 3) == t.data_ptr()
    assert m.stand_in(t, 3, t.device) is t
    s = m.stand_in(torch.zeros(0, dtype=torch.int32), 0, t.device)
    assert s.shape == (1,) and s.dtype == torch.int32 and int(s[0]) == 0
    s = m.stand_in(torch.zeros((0, 3), dtype=torch.uint8), 0, t.device, 3)
    assert s.shape == (1, 3) and s.dtype == torch.uint8
    c = torch.zeros((4, 6)).t()
    assert m.unit_columns(c).stride(1) == 1 and m.unit_columns(c[:, :1].t()).stride(1) == 1
    r = torch.zeros((4, 9))[:, :6]
    assert m.unit_columns(r) is r


def test_tables_and_codes():
    assert m.tables_arg(torch.zeros((5, 16)), 5, 16) == (True, 1)
    assert m.tables_arg(torch.zeros((3, 5, 16)), 5, 16) == (False, 3)
    assert m.tables_arg(torch.zeros((0, 5, 16)), 5, 16) == (False, 0)
    for bad in ((5, 15), (16, 5), (3, 4, 16)):
        with pytest.raises(PanicError, match=re.escape("lookup tables must be [.., 5, 16]")):
            m.tables_arg(torch.zeros(bad), 5, 16)
    u8 = torch.zeros((7, 5), dtype=torch.uint8)
    assert m.code_width(u8, 5) == 5 and m.code_width(u8[:, :3], 5, True) == 3
    assert m.code_width(torch.zeros((7, 5), dtype=torch.int32), 5) == 5
    with pytest.raises(PanicError, match="Quantization length does not match number of subquantizers"):
        m.code_width(u8, 4)
    for bad in (u8, u8[:, :2], torch.zeros((7, 3), dtype=torch.int32)):
        with pytest.raises(PanicError, match=re.escape("4-bit packed codes must be uint8 [n, ceil(n_subquantizers / 2)]")):
            m.code_width(bad, 5, True)
    for n in (0, 1, 7):
        c, rows, stride = m.codes_arg(torch.zeros((n, 8), dtype=torch.uint8)[:, :5], 5)
        assert (rows, stride) == (n, 8) and c.shape == (n, 5)
    c, rows, stride = m.codes_arg(torch.zeros((5, 7), dtype=torch.uint8).t(), 5)
    assert (rows, stride, c.stride(1)) == (7, 5, 1)


def test_lists_arguments():
    off = torch.zeros(5, dtype=torch.int64)
    pr, n_probe, stride = m.probes_arg(torch.zeros((3, 6), dtype=torch.int64)[:, :2], off, 3)
    assert (n_probe, stride) == (2, 6)
    pr, n_probe, stride = m.probes_arg(torch.zeros(2, dtype=torch.int64), off, 1)
    assert pr.shape == (1, 2) and (n_probe, stride) == (2, 2)
    pr, n_probe, stride = m.probes_arg(torch.zeros((2, 3), dtype=torch.int64).t(), off, 3)
    assert pr.is_contiguous() and (n_probe, stride) == (2, 2)
    text = "one probe row of at least one list id per query and n_lists \\+ 1 offsets expected"
    for probes, offsets, nq in ((torch.zeros((2, 2)), off, 3), (torch.zeros((3, 0)), off, 3), (torch.zeros((3, 2)), off[:0], 3)):
        with pytest.raises(PanicError, match=text):
            m.probes_arg(probes, offsets, nq)
    threshold = m.threshold_arg(0.5, 3, "cpu")
    assert threshold.tolist() == [0.5] * 3 and threshold.is_contiguous() and threshold.dtype == torch.float32
    assert m.threshold_arg(np.float64(2), 1, "cpu").tolist() == [2.0]
    assert m.threshold_arg(np.array([1, 2, 3]), 3, "cpu").tolist() == [1.0, 2.0, 3.0]
    assert m.threshold_arg(torch.tensor([[1.0], [2.0]], dtype=torch.float64), 2, "cpu").tolist() == [1.0, 2.0]
    with pytest.raises(PanicError, match=re.escape("one threshold, or one per query (3), expected")):
        m.threshold_arg([1.0, 2.0], 3, "cpu")


class OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the device: the normalisers below assert that first"""
    is_cuda = True


def test_per_row_mask_and_bias():
    dev = lambda t: t.as_subclass(OnDevice)
    scales = dev(torch.zeros(7))
    assert m.per_row_arg(None, 7, "scales") is None and m.per_row_arg(scales, 7, "scales") is scales
    for what in ("scales", "row_terms"):
        with pytest.raises(PanicError, match="%s must hold one value per code row" % what):
            m.per_row_arg(scales, 6, what)
    with pytest.raises(AssertionError):
        m.per_row_arg(dev(torch.zeros(14)[::2]), 7, "scales")
    codes = torch.zeros((37, 5), dtype=torch.uint8)
    words = dev(torch.zeros(2, dtype=torch.int32))
    assert m.mask_words(words, codes) is words and m.mask_arg(words, codes, False) == (words.data_ptr(),)
    none = m.mask_words(dev(torch.zeros(0, dtype=torch.int32)), codes[:0])        # a non-NULL mask stays a mask
    assert none.shape == (1,) and none.dtype == torch.int32
    for bad, rows in ((words, 65), (words, 32), (words[:1], 37)):
        with pytest.raises(PanicError, match=re.escape("the row mask must hold ceil(n / 32) words for the n code rows")):
            m.mask_words(bad, torch.zeros((rows, 5), dtype=torch.uint8))
    pb, stride = m.bias_arg(dev(torch.zeros((3, 4))[:, :2]), 3, 2)
    assert pb.shape == (3, 2) and stride == 4
    pb, stride = m.bias_arg(dev(torch.zeros(2)), 1, 2)
    assert pb.shape == (1, 2) and stride == 2
    pb, stride = m.bias_arg(dev(torch.zeros((2, 3)).t()), 3, 2)
    assert pb.is_contiguous() and stride == 2
    for bad, nq in ((torch.zeros((3, 1)), 3), (torch.zeros((2, 2)), 3), (torch.zeros(2), 3)):
        with pytest.raises(PanicError, match="one probe bias per query and probe slot expected"):
            m.bias_arg(dev(bad), nq, 2)


def test_search_head_follows_the_signature_table():
    """search_head and mask_arg give as many leading arguments, pointers where the table has pointers, as each of the 24
    signatures has before its outputs"""
    vp = ctypes.c_void_p
    tables, codes = torch.zeros((3, 5, 16)), torch.zeros((7, 5), dtype=torch.uint8)
    off, pr, pb = torch.zeros(5, dtype=torch.int64), torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2))
    seen = set()
    for ip in ("", "ip_"):
        for where, lists, bias in (("", (), ()), ("_lists", (off, pr, 2, 2), ()), ("_lists_residual", (off, pr, 2, 2), (pb, 2))):
            last = (pb.data_ptr(),) if ip or bias else ()
            for form, packed4, mask in (("search%s_", False, ()), ("search%s_masked_", False, (None,)),
                                        ("search%s_packed4_", True, (None,)), ("range%s_", False, (None,))):
                name = "pqhip_adc_%s%sf32_dev" % (ip, form % where)
                head = m.search_head(vp(1), 0, tables, 3, codes, 7, 5, packed4, mask, lists, bias, last)
                argtypes = _lib.SIGNATURES[name][1]
                assert len(head) == len(argtypes) - 6, name
                for a, t in zip(head, argtypes):
                    assert (t is vp) == (a is None or isinstance(a, vp) or a > 1 << 16), (name, a, t)
                seen.add(name)
    assert len(seen) == 24 and seen == {s for s in _lib.SIGNATURES if re.match("pqhip_adc_(ip_)?(search|range)", s)}
    assert m.mask_arg(None, codes, False) == () and m.mask_arg(None, codes, True) == (None,)


def test_signature_table_and_header_name_the_same_symbols():
    with open(os.path.join(ROOT, "include", "pqhip.h")) as f:
        declared = set(re.findall(r"\b(pqhip_[a-z0-9_]+)\s*\(", f.read())) - {"pqhip_status"}
    assert declared == set(_lib.SIGNATURES) == set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
