"""Reference of the row compaction (include/pqhip.h: pqhip_rows_compact_dev), by its definition: output row j is the j-th kept
row, and the offset of list l moves to the number of kept rows before it.  Pure numpy; pinned against ivf_layout by
tests/test_rows_compact.py."""
import numpy as np


def pack_words(keep_bits, tail=0):
    """bool [n] -> the mask words, uint32 [ceil(n / 32)]: bit i & 31 of word i >> 5 = keep_bits[i]; the bits of the last word
    at or beyond n are taken from `tail` (the kernel must ignore them)"""
    keep_bits = np.asarray(keep_bits, dtype=bool)
    n = keep_bits.size
    padded = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    padded[:n] = keep_bits
    words = (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    if n % 32:
        words[-1] |= np.uint32(tail) & ~np.uint32((1 << (n % 32)) - 1)
    return words


def unpack_words(words, n):
    """the inverse of pack_words: the first n bits as bool [n]"""
    words = np.asarray(words).view(np.uint32)
    return ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:n]


def ref_compact(keep_bits, rows, off=None):
    """keep_bits bool [n], rows [n, ...] or None, off [L + 1] (valid list offsets of the rows) or None
    -> (out [c, ...] or None, off_out [L + 1] or None, src_rows int64 [c], c)"""
    keep_bits = np.asarray(keep_bits, dtype=bool)
    n = keep_bits.size
    src = np.flatnonzero(keep_bits).astype(np.int64)        # s_0 < s_1 < .. : the kept rows in ascending order
    out = None
    if rows is not None:
        assert rows.shape[0] == n
        out = rows[src] if src.size else rows[:0]
    off_out = None
    if off is not None:
        off = np.asarray(off, dtype=np.int64)
        assert off[0] == 0 and off[-1] == n and np.all(off[1:] >= off[:-1])
        before = np.zeros(n + 1, np.int64)                  # before[i] = kept rows below i
        np.cumsum(keep_bits, out=before[1:])
        off_out = before[off]
    return out, off_out, src, int(src.size)
