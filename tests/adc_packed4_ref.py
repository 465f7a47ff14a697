"""Reference of the 4-bit packed code format (include/pqhip.h, "4-bit packed codes"), written from its definition and
independent of reductive_amd.pack_codes4 / unpack_codes4: a row of M codes < K <= 16 is ceil(M / 2) bytes, code m lives in
byte m >> 1, the low nibble holds even m and the high nibble odd m; the high nibble of the last byte of an odd M is
written as 0 and ignored by every reader.  A packed search is, by definition, the existing search on the unpacked codes,
so there is no packed search reference: unpack_ref feeds the existing ones.  Numpy only, one element at a time."""
import numpy as np


def pack_ref(codes, K=16):
    c = np.asarray(codes)
    assert c.ndim == 2 and K <= 16
    n, M = c.shape
    out = np.zeros((n, (M + 1) // 2), np.uint8)
    for i in range(n):
        for m in range(M):
            v = int(c[i, m])
            if not 0 <= v < K:
                raise ValueError("code %d at (%d, %d) is not below %d" % (v, i, m, K))
            out[i, m >> 1] |= v << (4 * (m & 1))
    return out


def unpack_ref(packed, M):
    p = np.asarray(packed)
    assert p.ndim == 2 and p.dtype == np.uint8 and p.shape[1] == (M + 1) // 2
    out = np.zeros((p.shape[0], M), np.uint8)
    for i in range(p.shape[0]):
        for m in range(M):
            out[i, m] = (int(p[i, m >> 1]) >> (4 * (m & 1))) & 0xf
    return out
