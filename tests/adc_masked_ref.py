"""Reference of the masked ADC searches (include/pqhip.h: pqhip_adc_*search*_masked_f32_dev, pqhip_pack_row_mask_dev),
by their definition: the result is what the unmasked search returns on the matrix with every disallowed row removed,
indices mapped back.  So each function restricts the values to the allowed rows, calls the reference of the unmasked
search (test_gpu_adc_search.ref_search, adc_ip_ref.ref_ip_search, adc_lists_ref.ref_lists_search,
adc_residual_ref.ref_residual_search) and maps the indices back; the list forms rebuild list_off over the compressed
rows.  Numpy only."""
import numpy as np

from adc_ip_ref import ref_ip_search
from adc_lists_ref import ref_lists_search
from adc_residual_ref import ref_residual_search
from test_gpu_adc_search import ref_search


def pack_ref(allow, perm=None):
    """the mask words, uint32 [ceil(n / 32)]: bit p & 31 of word p >> 5 is allow[perm[p]] (allow[p] without perm), the
    tail bits of the last word 0"""
    a = np.asarray(allow).astype(bool)
    if perm is not None:
        a = a[np.asarray(perm, np.int64)]
    b = np.packbits(a, bitorder="little")
    b = np.concatenate([b, np.zeros((-b.size) % 4, np.uint8)])
    return b.view("<u4").astype(np.uint32)


def unpack_ref(words, n):
    """bool [n]: the flags that `words` holds for rows 0 .. n-1 (bits at or beyond n are ignored)"""
    b = np.ascontiguousarray(np.asarray(words).astype("<u4")).view(np.uint8)
    return np.unpackbits(b, bitorder="little")[:n].astype(bool)


def _map_back(idx, rows):
    return np.where(idx < 0, -1, rows[np.clip(idx, 0, max(rows.size - 1, 0))] if rows.size else -1).astype(np.int64)


def ref_masked_search(values, allow, k, ip=False):
    """values [n] or [nq, n] f32 (distances, or scores with ip=True) of every row; allow bool [n] -> (value, idx)
    [nq, k]: the unmasked reference over the allowed rows alone, indices mapped back"""
    v2 = np.atleast_2d(np.asarray(values, np.float32))
    rows = np.flatnonzero(np.asarray(allow, bool))
    sub = np.ascontiguousarray(v2[:, rows])
    v, i = ref_ip_search(sub, k) if ip else ref_search(sub, k)
    return v, _map_back(i, rows)


def compressed_offsets(list_off, allow):
    """list_off over the matrix with the disallowed rows removed: the number of allowed rows before each offset
    (offsets clamped to [0, n] first, as the searches clamp them)"""
    a = np.asarray(allow, bool)
    before = np.concatenate([[0], np.cumsum(a)]).astype(np.int64)
    return before[np.clip(np.asarray(list_off, np.int64), 0, a.size)]


def ref_masked_lists_search(values, allow, list_off, probes, k, ip=False):
    """the list searches: values [nq, n] of every row, list_off / probes as for adc_lists_ref.ref_lists_search"""
    v2 = np.atleast_2d(np.asarray(values, np.float32))
    rows = np.flatnonzero(np.asarray(allow, bool))
    v, i = ref_lists_search(np.ascontiguousarray(v2[:, rows]), compressed_offsets(list_off, allow), probes, k, ip=ip)
    return v, _map_back(i, rows)


def ref_masked_residual_search(s, allow, list_off, probes, bias, k, terms=None, scales=None, ip=False):
    """the residual list searches: s [nq, n] the scan over the inner-product tables, the rest as for
    adc_residual_ref.ref_residual_search; terms / scales of disallowed rows never enter"""
    s2 = np.atleast_2d(np.asarray(s, np.float32))
    rows = np.flatnonzero(np.asarray(allow, bool))
    v, i = ref_residual_search(np.ascontiguousarray(s2[:, rows]), compressed_offsets(list_off, allow), probes, bias, k,
                               terms=None if terms is None else np.asarray(terms, np.float32)[rows],
                               scales=None if scales is None else np.asarray(scales, np.float32)[rows], ip=ip)
    return v, _map_back(i, rows)
