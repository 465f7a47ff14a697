"""numpy reference of pqhip_topk_merge_f32_dev (include/pqhip.h): the definition, written as directly as numpy allows.

order_key is adc_order_key of csrc/adc_key.hip.h; ref_merge sorts the present entries of every query by (key, part, rank)
with np.lexsort and pads; canonical() is what the header says of returned values (a NaN as the canonical quiet NaN, a zero
as +0, everything else bit for bit).  SPECIAL_VALUES is the value set of the tests: multiples of 0.25 in [-2, 2] plus
-0, +-Inf and NaN, so that ties and special values are the rule."""
import numpy as np

QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
SPECIAL_VALUES = np.concatenate([np.arange(-8, 9, dtype=np.float32) * np.float32(0.25),
                                 np.array([-0.0, np.inf, -np.inf, np.nan], np.float32)])


def order_key(v):
    """uint32 keys of float32 values: -0 -> +0, every NaN 0xffffffff (above +Inf), otherwise the usual monotone map"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000))
    key[nan] = np.uint32(0xFFFFFFFF)
    return key


def canonical(v):
    """values as the library returns them"""
    v = np.array(v, dtype=np.float32, copy=True)
    v[np.isnan(v)] = QNAN
    v[v == 0] = np.float32(0.0)
    return v


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def ref_merge(val, idx, k, largest=False, offsets=None):
    """val float32 / idx int64 [P, nq, k_in] -> (val [nq, k], idx [nq, k], part int32 [nq, k])"""
    val = np.asarray(val, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    P, nq, k_in = val.shape
    out_v = np.full((nq, k), -np.inf if largest else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    out_p = np.full((nq, k), -1, np.int32)
    part = np.repeat(np.arange(P), k_in)
    rank = np.tile(np.arange(k_in), P)
    for q in range(nq):
        v = val[:, q, :].reshape(-1)
        i = idx[:, q, :].reshape(-1)
        here = np.flatnonzero(i >= 0)
        key = order_key(-v[here] if largest else v[here])
        order = here[np.lexsort((rank[here], part[here], key))][:k]
        c = order.size
        out_v[q, :c] = canonical(v[order])
        out_i[q, :c] = i[order] + (0 if offsets is None else np.asarray(offsets, dtype=np.int64)[part[order]])
        out_p[q, :c] = part[order]
    return out_v, out_i, out_p


def brute_topk(values, k, largest=False):
    """values float32 [nq, n]: the k best rows of every query in the library's order, ties to the smaller row ->
    (val [nq, k], idx [nq, k]) with padding (+-Inf, -1) past n"""
    values = np.asarray(values, dtype=np.float32)
    nq, n = values.shape
    out_v = np.full((nq, k), -np.inf if largest else np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        key = order_key(-values[q] if largest else values[q])
        order = np.lexsort((np.arange(n), key))[:k]
        out_v[q, :order.size] = canonical(values[q, order])
        out_i[q, :order.size] = order
    return out_v, out_i
