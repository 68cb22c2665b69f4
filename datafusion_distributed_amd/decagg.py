"""decagg.py — exact model of partial aggregation with decimal sums.

Like dictgc.py and views.py this is a numpy / Python-int statement of semantics, not a
compute path: nothing here touches the device. It extends oracle/reduce_ref.py's model
(whose grouping it reuses, so group identity is the same by construction) with the op
"sum_dec128": the exact sum of a dec128 column's non-null values as a 128-bit two's
complement integer that wraps modulo 2^128.

Result shape, as reduce_ref's: {(key_bits_tuple, keynull_mask): [entry per aggregate]} with
entry = {"op", "value": signed Python int or None, "nn": non-null input count}. The narrow
ops keep reduce_ref's entries unchanged.
"""

import numpy as np

from oracle import reduce_ref as rr

M128 = (1 << 128) - 1
_SIGN128 = 1 << 127
_M64 = (1 << 64) - 1


def to_signed128(v):
    """A Python int modulo 2^128, read as two's complement."""
    v &= M128
    return v - (1 << 128) if v & _SIGN128 else v


def dec_ints(col):
    """The values of a dec128 column dict as signed Python ints (NULL rows included: their
    bytes are whatever the column holds)."""
    data = np.asarray(col["data"])
    if data.dtype != np.uint64 or data.ndim != 2:
        data = np.ascontiguousarray(data).reshape(-1).view(np.uint8).view(np.uint64)
    words = data.reshape(-1, 2).tolist()
    return [to_signed128(lo | (hi << 64)) for lo, hi in words]


def dec_words(values):
    """Signed Python ints -> u64 (n, 2) = [lo, hi], two's complement modulo 2^128."""
    out = np.zeros((len(values), 2), dtype=np.uint64)
    for i, v in enumerate(values):
        v &= M128
        out[i, 0] = v & _M64
        out[i, 1] = v >> 64
    return out


def _sum_dec_segments(values, ok, order, starts, n):
    """Per segment of the sorted rows: {"op", "value", "nn"} over the non-null values."""
    bounds = list(starts.tolist()) + [n]
    order = order.tolist()
    out = []
    for i in range(len(starts)):
        tot, nn = 0, 0
        for j in order[bounds[i]:bounds[i + 1]]:
            if ok[j]:
                tot += values[j]
                nn += 1
        out.append({"op": "sum_dec128", "value": to_signed128(tot) if nn else None, "nn": nn})
    return out


def reduce_dec_ref(cols, key_idx, aggs):
    """Exact grouped aggregation of `cols` by key columns `key_idx`. aggs: (col index or
    None, op name) as api.partial_reduce takes them; "sum_dec128" is summed with Python
    ints modulo 2^128, every other op is reduce_ref's."""
    keys, keynull = rr.key_bits(cols, key_idx)
    order, starts = rr._segments(keys, keynull)
    n = len(keynull)
    narrow = [(g, a) for g, a in enumerate(aggs) if a[1] != "sum_dec128"]
    narrow_res = rr.reduce_ref(cols, key_idx, [a for _, a in narrow]) if narrow else {}
    per_agg = [None] * len(aggs)
    for g, (ci, op) in enumerate(aggs):
        if op != "sum_dec128":
            continue
        col = cols[ci]
        ok = (np.asarray(col["valid"]).astype(bool).tolist() if col.get("valid") is not None
              else [True] * n)
        per_agg[g] = _sum_dec_segments(dec_ints(col), ok, order, starts, n) if n else []
    out = {}
    ks = keys[order][starts].tolist() if len(starts) else []
    kn = keynull[order][starts].tolist() if len(starts) else []
    for i in range(len(starts)):
        gid = (tuple(ks[i]), kn[i])
        entries = [None] * len(aggs)
        for j, (g, _) in enumerate(narrow):
            entries[g] = narrow_res[gid][j]
        for g in range(len(aggs)):
            if per_agg[g] is not None:
                entries[g] = per_agg[g][i]
        out[gid] = entries
    return out


def final_merge_dec(res, ops):
    """Final aggregate over partial rows (api.partial_reduce's return value, or any dict
    with its "keys", "keynull", "aggs", "aggs_hi" and "nn"): rows merge by (keys, keynull).
    A "sum_dec128" sums (lo, hi) modulo 2^128 over the partials and sums nn; the value is
    None when the total nn is 0. Every other op is reduce_ref.final_merge's."""
    keys = np.asarray(res["keys"], dtype=np.uint64)
    keynull = np.asarray(res["keynull"], dtype=np.uint32)
    order, starts = rr._segments(keys, keynull)
    n = len(keynull)
    narrow = [g for g, op in enumerate(ops) if op != "sum_dec128"]
    narrow_res = {}
    if narrow:
        sub = {"keys": keys, "keynull": keynull,
               "aggs": np.ascontiguousarray(np.asarray(res["aggs"])[:, narrow]),
               "nn": np.ascontiguousarray(np.asarray(res["nn"])[:, narrow])}
        narrow_res = rr.final_merge(sub, [ops[g] for g in narrow])
    lo_all = np.ascontiguousarray(res["aggs"], dtype=np.float64).view(np.uint64)
    hi_all = np.asarray(res["aggs_hi"], dtype=np.uint64)
    nn_all = np.asarray(res["nn"], dtype=np.uint64)
    bounds = list(starts.tolist()) + [n]
    order_l = order.tolist()
    out = {}
    ks = keys[order][starts].tolist() if len(starts) else []
    kn = keynull[order][starts].tolist() if len(starts) else []
    dec = {}
    for g, op in enumerate(ops):
        if op == "sum_dec128":
            dec[g] = (lo_all[:, g].tolist(), hi_all[:, g].tolist(), nn_all[:, g].tolist())
    for i in range(len(starts)):
        gid = (tuple(ks[i]), kn[i])
        entries = [None] * len(ops)
        for j, g in enumerate(narrow):
            entries[g] = narrow_res[gid][j]
        rows = order_l[bounds[i]:bounds[i + 1]]
        for g, (lo, hi, nn) in dec.items():
            tot = sum(lo[r] | (hi[r] << 64) for r in rows)
            cnt = sum(nn[r] for r in rows)
            entries[g] = {"op": "sum_dec128", "value": to_signed128(tot) if cnt else None,
                          "nn": cnt}
        out[gid] = entries
    return out
