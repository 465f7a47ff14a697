"""What every `*_device` wrapper of pq.py does between its torch tensors and the C ABI (include/pqhip.h): the launch
context, call-and-raise, the range check, strides and addresses of small tensors, the argument normalisers and the
leading arguments of the 24 ADC search and range entry points.  Plumbing only -- no compute here.

The normalisers carry the PanicError checks; the bare dtype asserts stay in the wrappers, in the order they always had.
tests/test_gpu_device_call_trace.py pins what the wrappers hand to the library."""
import ctypes

import numpy as np

from . import _lib
from ._lib import PanicError

RANGE_PANIC = {_lib.ECODE_RANGE: "ndarray: index out of bounds"}                      # primitives.rs:146
WIDTH_PANIC = {_lib.EINDEX_WIDTH: "Cannot store centroids in quantizer index type"}


def launch(pq, tensor, stream):
    """(cb, slot, stream pointer) of a call on the device of `tensor`: torch's current stream there unless `stream` (a
    raw hipStream_t int) is given."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return pq._cb(), pq._slot_for(tensor), ctypes.c_void_p(stream)


def run(name, *args, panics=None):
    """Call the library's `name`; a status other than OK raises PqHipError, or the PanicError `panics` maps it to."""
    rc = getattr(_lib.lib(), name)(*args)
    if rc != _lib.OK:
        if panics and rc in panics:
            raise PanicError(panics[rc])
        raise _lib.PqHipError(rc, name)


def check_range(cb, slot, stream_ptr):
    """The `check=True` epilogue: synchronise the stream and raise the reference's index panic if its range flag is up."""
    run("pqhip_check_codes_dev", cb, slot, stream_ptr, panics=RANGE_PANIC)


def row_stride(t, rows, width):
    """Row stride of `t` as the C calls want it: torch reports any stride for a dimension of at most one row, the library
    wants one of at least `width`.  `rows` is the count the call passes, which is not always t.shape[0]."""
    return t.stride(0) if rows > 1 else max(t.stride(0), width)


def ptr_or_none(t, n=1):
    """Address of `t`, NULL for None or when the call has no element of it to touch (an empty tensor may have no address)."""
    return t.data_ptr() if t is not None and n else None


def stand_in(t, n, device, width=None):
    """`t`, or one zero element ([1, width]) of its dtype when n = 0, for the C calls that want an address even then."""
    if n > 0:
        return t
    import torch
    return torch.zeros(1 if width is None else (1, width), dtype=t.dtype, device=device)


def unit_columns(t):
    """`t` with unit column stride, by a copy if need be."""
    return t if t.stride(1) == 1 else t.contiguous()


# ---- argument normalisers: the tensor to pass and the integers the C call needs ---------------------------------------
def tables_arg(tables, M, K):
    """tables [M, K] or [nq, M, K] -> (single, nq)"""
    single = tables.dim() == 2
    if tuple(tables.shape[-2:]) != (M, K):
        raise PanicError("lookup tables must be [.., %d, %d]" % (M, K))
    return single, 1 if single else tables.shape[0]


def code_width(codes, M, packed4=False):
    """The row width the searches expect of `codes`: M elements, or ceil(M / 2) bytes of 4-bit packed rows."""
    if not packed4:
        if codes.shape[1] != M:
            raise PanicError("Quantization length does not match number of subquantizers")
        return M
    import torch
    if codes.dtype != torch.uint8 or codes.shape[1] != (M + 1) // 2:
        raise PanicError("4-bit packed codes must be uint8 [n, ceil(n_subquantizers / 2)]")
    return (M + 1) // 2


def codes_arg(codes, W):
    """codes [n, W] -> (codes with unit column stride, n, row stride)"""
    codes = unit_columns(codes)
    n = codes.shape[0]
    return codes, n, row_stride(codes, n, W)


def per_row_arg(t, n, what):
    """scales / row_terms: None or contiguous float32 [n] -> the same"""
    if t is not None:
        import torch
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        if tuple(t.shape) != (n,):
            raise PanicError("%s must hold one value per code row" % what)
    return t


def mask_words(allow, codes):
    """The words tensor of a search's `allow=`: CUDA int32 [ceil(n / 32)] on the device of the codes."""
    import torch
    assert allow.is_cuda and allow.dtype == torch.int32 and allow.dim() == 1 and allow.is_contiguous()
    if allow.device != codes.device or allow.shape[0] != (codes.shape[0] + 31) // 32:
        raise PanicError("the row mask must hold ceil(n / 32) words for the n code rows")
    # a non-NULL mask must stay a mask (n = 0 reads no word)
    return stand_in(allow, allow.shape[0], codes.device)


def mask_arg(allow, codes, required):
    """The mask argument of an entry point as a tuple: () where the plain form has none, else the address or NULL."""
    if allow is None:
        return (None,) if required else ()
    return (mask_words(allow, codes).data_ptr(),)


def vector_mask_words(allow, n):
    """The words tensor of flat_search_device's `allow=`: None, or int32 [ceil(n / 32)] for the n rows of the vectors.
    Shape and dtype only: the wrapper checks devices after everything a host tensor can get wrong."""
    if allow is None:
        return None
    import torch
    if not hasattr(allow, "is_cuda") or allow.dtype != torch.int32 or allow.dim() != 1 or not allow.is_contiguous():
        raise PanicError("allow must be the int32 mask words of pack_row_mask_device")
    if allow.shape[0] != (n + 31) // 32:
        raise PanicError("the row mask must hold ceil(n / 32) words for the n rows")
    return allow


def vector_lists_arg(list_off, probes, nq):
    """The lists of flat_search_lists_device: list_off int64 [n_lists + 1] contiguous, probes int64 [nq, n_probe]
    ([n_probe] for one query) with at least one column -> (pr with unit column stride, n_lists, n_probe, row stride).
    Shape and dtype only, as vector_mask_words: the wrapper checks devices afterwards."""
    import torch
    for t, what in ((list_off, "list_off"), (probes, "probes")):
        if not hasattr(t, "is_cuda"):
            raise PanicError("%s must be a torch tensor" % what)
    if list_off.dtype != torch.int64 or list_off.dim() != 1 or list_off.shape[0] < 1 or not list_off.is_contiguous():
        raise PanicError("list_off must be the int64 offsets of the lists, [n_lists + 1]")
    if probes.dtype != torch.int64 or probes.dim() not in (1, 2):
        raise PanicError("probes must be int64 list ids, [n_probe] or [nq, n_probe]")
    pr = probes[None] if probes.dim() == 1 else probes
    if pr.shape[0] != nq or pr.shape[1] < 1:
        raise PanicError("one probe row of at least one list id per query expected")
    if pr.shape[1] >= 1 << 24:
        raise PanicError("fewer than 2^24 probes per query are served")
    pr = unit_columns(pr)
    n_probe = pr.shape[1]
    return pr, list_off.shape[0] - 1, n_probe, row_stride(pr, nq, n_probe)


def assert_lists(list_off, probes):
    import torch
    assert list_off.is_cuda and list_off.dtype == torch.int64 and list_off.dim() == 1 and list_off.is_contiguous()
    assert probes.is_cuda and probes.dtype == torch.int64 and probes.dim() in (1, 2)


def probes_arg(probes, list_off, nq):
    """probes [nq, n_probe] ([n_probe] for one query) -> (pr with unit column stride, n_probe, row stride)"""
    pr = probes[None] if probes.dim() == 1 else probes
    if pr.shape[0] != nq or pr.shape[1] < 1 or list_off.shape[0] < 1:
        raise PanicError("one probe row of at least one list id per query and n_lists + 1 offsets expected")
    pr = unit_columns(pr)
    n_probe = pr.shape[1]
    return pr, n_probe, row_stride(pr, nq, n_probe)


def bias_arg(probe_bias, nq, n_probe):
    """probe_bias [nq, n_probe] ([n_probe] for one query) -> (pb with unit column stride, row stride)"""
    import torch
    assert probe_bias.is_cuda and probe_bias.dtype == torch.float32 and probe_bias.dim() in (1, 2)
    pb = probe_bias[None] if probe_bias.dim() == 1 else probe_bias
    if tuple(pb.shape) != (nq, n_probe):
        raise PanicError("one probe bias per query and probe slot expected")
    pb = unit_columns(pb)
    return pb, row_stride(pb, nq, n_probe)


def threshold_arg(threshold, nq, device):
    """a scalar or one value per query (float, numpy or tensor) -> contiguous float32 [nq] on `device`"""
    import torch
    if hasattr(threshold, "is_cuda"):
        thr = threshold.to(device, torch.float32).reshape(-1)
    else:
        thr = torch.from_numpy(np.asarray(threshold, dtype=np.float32).reshape(-1).copy()).to(device)
    if thr.shape[0] == 1 and nq != 1:
        thr = thr.expand(nq)
    if thr.shape[0] != nq:
        raise PanicError("one threshold, or one per query (%d), expected" % nq)
    return thr.contiguous()


def search_head(cb, slot, tables, nq, codes, n, c_rs, packed4=False, mask=(), lists=(), bias=(), last=()):
    """The leading arguments of the 24 ADC search and range entry points, by the grammar of _lib.SIGNATURES: no code_bytes
    for packed4; mask from mask_arg; lists (list_off, pr, n_probe, stride); bias (pb, stride); last (scales or row terms
    address,).  The caller appends the outputs."""
    head = (cb, slot, tables.data_ptr(), nq, codes.data_ptr()) if packed4 else \
           (cb, slot, tables.data_ptr(), nq, codes.data_ptr(), codes.element_size())
    if lists:
        list_off, pr, n_probe, p_rs = lists
        lists = (list_off.data_ptr(), list_off.shape[0] - 1, pr.data_ptr(), n_probe, p_rs)
    if bias:
        bias = (bias[0].data_ptr(), bias[1])
    return head + (n, c_rs) + mask + lists + bias + last
