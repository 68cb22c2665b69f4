"""oracle/reduce_ref.py — exact reference model of partial aggregation and its final merge.

TEST INFRASTRUCTURE ONLY (like the rest of oracle/): imported by tests, never by the
product path. Pure Python/numpy; needs no device.

Contract restated (include/dd_shuffle.h, "partial aggregation"):
  * group identity = (canonical u64 key bits per key column, keynull bitmask); a NULL key
    component has bits 0; float keys are canonicalised by pyref._value_bits; a dict32 key
    groups by its index.
  * count counts every row. Every other op skips NULL inputs and is NULL (None) when no
    non-null input exists.
  * sum_i64 wraps modulo 2^64; sum_f64 is compared against math.fsum with a derived bound;
    min_i64 / max_i64 are signed; min_f64 / max_f64 follow IEEE-754 totalOrder and are
    reported as u64 bit patterns so -0.0 / +0.0 / NaN payloads stay distinguishable.

Result shape (reduce_ref, final_merge, merge_dict_by_value):
  {(key_bits_tuple, keynull_mask): [entry per aggregate]} with
  entry = {"op": name, "value": exact result or None, "nn": non-null input count}
  and, for sum_f64, "terms" (the addends still unrounded on the merge side), "abs_sum"
  and "n_nonnull" (reference side: inputs to the summation error bound).
"""

import math

import numpy as np

from oracle import pyref

OPS = ("sum_f64", "count", "sum_i64", "min_f64", "max_f64", "min_i64", "max_i64")
INT_OPS = ("count", "sum_i64", "min_i64", "max_i64")

_SIGN = 1 << 63
_MAG = _SIGN - 1
_M64 = (1 << 64) - 1
_I64_MAX = np.iinfo(np.int64).max
_I64_MIN = np.iinfo(np.int64).min


# ---------------- IEEE-754 totalOrder on f64 bit patterns ----------------

def total_order_key(bits):
    """Sort key of one f64 bit pattern under totalOrder: all sign-set patterns come first,
    larger magnitude earlier; then all sign-clear patterns, larger magnitude later."""
    bits = int(bits)
    mag = bits & _MAG
    return (0, -mag) if bits & _SIGN else (1, mag)


def total_order_rank(bits):
    """Vectorised totalOrder: u64 bit patterns -> int64 ranks with the same ordering as
    total_order_key (sign-clear: magnitude; sign-set: -magnitude - 1)."""
    bits = np.asarray(bits, dtype=np.uint64)
    mag = (bits & np.uint64(_MAG)).astype(np.int64)
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, -mag - 1, mag)


def rank_to_bits(rank):
    """Inverse of total_order_rank for one rank (Python int) -> u64 bit pattern."""
    rank = int(rank)
    return rank if rank >= 0 else (_SIGN | (-rank - 1))


def to_signed64(v):
    v &= _M64
    return v - (1 << 64) if v & _SIGN else v


def fsum_ext(xs):
    """math.fsum extended to non-finite inputs with IEEE semantics: any NaN, or both
    infinities, -> NaN; one infinity -> that infinity. Finite inputs whose exact sum
    overflows -> the correctly signed infinity."""
    pinf = ninf = False
    for x in xs:
        if x != x:
            return math.nan
        if x == math.inf:
            pinf = True
        elif x == -math.inf:
            ninf = True
    if pinf or ninf:
        if pinf and ninf:
            return math.nan
        return math.inf if pinf else -math.inf
    try:
        return math.fsum(xs)
    except OverflowError:
        return math.copysign(math.inf, math.fsum(x / 4.0 for x in xs))


# ---------------- grouping ----------------

def _segments(keys, keynull):
    """Sort rows by (keys..., keynull); return (order, starts) of the equal-identity runs."""
    n = len(keynull)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cols = [keys[:, k] for k in range(keys.shape[1])] + [keynull.astype(np.uint64)]
    order = np.lexsort(cols[::-1])
    change = np.zeros(n, dtype=bool)
    change[0] = True
    for c in cols:
        cs = c[order]
        change[1:] |= cs[1:] != cs[:-1]
    return order, np.flatnonzero(change)


def key_bits(cols, key_idx):
    """(keys u64[n, nk], keynull u32[n]) — the canonical group identity per input row."""
    n = len(cols[key_idx[0]]["data"])
    keys = np.zeros((n, len(key_idx)), dtype=np.uint64)
    keynull = np.zeros(n, dtype=np.uint32)
    for k, ci in enumerate(key_idx):
        col = cols[ci]
        if col["dtype"] == "dict32":
            bits = np.asarray(col["data"], dtype=np.int32).view(np.uint32).astype(np.uint64)
        else:
            bits = pyref._value_bits(col)
        if col.get("valid") is not None:
            isnull = ~np.asarray(col["valid"]).astype(bool)
            bits = np.where(isnull, np.uint64(0), bits)
            keynull |= isnull.astype(np.uint32) << np.uint32(k)
        keys[:, k] = bits
    return keys, keynull


def _sum_i64_segments(vals_i64, starts):
    """Exact Python-int sums per segment (32-bit halves summed without overflow)."""
    hi = np.add.reduceat(vals_i64 >> 32, starts).tolist()
    lo = np.add.reduceat(vals_i64 & 0xFFFFFFFF, starts).tolist()
    return [(h << 32) + l for h, l in zip(hi, lo)]


def _fsum_segments(vals, ok, nn):
    """Per segment: (fsum, fsum of |x|, addend list) over the non-null values."""
    compact = vals[ok].tolist()
    off = np.concatenate([[0], np.cumsum(nn)]).tolist()
    out = []
    for i in range(len(nn)):
        xs = compact[off[i]:off[i + 1]]
        out.append((fsum_ext(xs), fsum_ext([abs(x) for x in xs]), xs))
    return out


def _reduce_segments(op, vals, ok, starts, keep_terms):
    """One aggregate over sorted rows. vals: values in row-sorted order (f64 bit-compatible
    for *_f64, int64 for *_i64, ignored for count); ok: non-null mask; -> entry list."""
    ng = len(starts)
    nn = np.add.reduceat(ok.astype(np.int64), starts).tolist()
    if op == "count":
        return [{"op": op, "value": c, "nn": c} for c in nn]
    if op == "sum_i64":
        sums = _sum_i64_segments(np.where(ok, vals, 0), starts)
        return [{"op": op, "value": to_signed64(sums[i]) if nn[i] else None, "nn": nn[i]}
                for i in range(ng)]
    if op in ("min_i64", "max_i64"):
        if op == "min_i64":
            r = np.minimum.reduceat(np.where(ok, vals, _I64_MAX), starts).tolist()
        else:
            r = np.maximum.reduceat(np.where(ok, vals, _I64_MIN), starts).tolist()
        return [{"op": op, "value": r[i] if nn[i] else None, "nn": nn[i]}
                for i in range(ng)]
    if op in ("min_f64", "max_f64"):
        rank = total_order_rank(vals.view(np.uint64))
        if op == "min_f64":
            r = np.minimum.reduceat(np.where(ok, rank, _I64_MAX), starts).tolist()
        else:
            r = np.maximum.reduceat(np.where(ok, rank, _I64_MIN), starts).tolist()
        return [{"op": op, "value": rank_to_bits(r[i]) if nn[i] else None, "nn": nn[i]}
                for i in range(ng)]
    if op == "sum_f64":
        segs = _fsum_segments(vals, ok, nn)
        out = []
        for i in range(ng):
            s, a, xs = segs[i]
            e = {"op": op, "value": s if nn[i] else None, "nn": nn[i],
                 "abs_sum": a, "n_nonnull": nn[i]}
            if keep_terms:
                e["terms"] = xs
            out.append(e)
        return out
    raise ValueError(op)


def _assemble(keys, keynull, order, starts, per_agg):
    ks = keys[order][starts].tolist() if len(starts) else []
    kn = keynull[order][starts].tolist() if len(starts) else []
    return {(tuple(ks[i]), kn[i]): [a[i] for a in per_agg] for i in range(len(starts))}


# ---------------- the model ----------------

def reduce_ref(cols, key_idx, aggs):
    """Exact grouped aggregation of `cols` (pyref column dicts) by key columns `key_idx`.
    aggs: list of (col_index_or_None, op name) as api.partial_reduce takes them."""
    keys, keynull = key_bits(cols, key_idx)
    order, starts = _segments(keys, keynull)
    n = len(keynull)
    per_agg = []
    for ci, op in aggs:
        if op == "count":
            vals, ok = None, np.ones(n, dtype=bool)
        else:
            col = cols[ci]
            want = np.float64 if op.endswith("f64") else np.int64
            vals = np.ascontiguousarray(col["data"], dtype=want)[order]
            ok = (np.asarray(col["valid"]).astype(bool)[order]
                  if col.get("valid") is not None else np.ones(n, dtype=bool))
        per_agg.append(_reduce_segments(op, vals, ok, starts, keep_terms=False)
                       if n else [])
    return _assemble(keys, keynull, order, starts, per_agg)


def final_merge(res, ops):
    """Op-aware final aggregate over partial rows (api.partial_reduce's return value).
    Sums merge exactly (math.fsum / Python ints mod 2^64), min/max merge under signed /
    totalOrder comparison and skip rows with nn == 0, nn is summed, total nn == 0 -> None."""
    keys = np.asarray(res["keys"], dtype=np.uint64)
    keynull = np.asarray(res["keynull"], dtype=np.uint32)
    order, starts = _segments(keys, keynull)
    n = len(keynull)
    aggs = np.ascontiguousarray(res["aggs"], dtype=np.float64)
    nn_all = np.asarray(res["nn"], dtype=np.uint64).astype(np.int64)
    per_agg = []
    for g, op in enumerate(ops):
        if n == 0:
            per_agg.append([])
            continue
        nn = nn_all[order, g]
        nn_tot = np.add.reduceat(nn, starts).tolist()
        col = np.ascontiguousarray(aggs[:, g])[order]
        if op == "count":
            # each partial's count is its value; nn must mirror it (checked by callers)
            tot = _sum_i64_segments(col.view(np.int64), starts)
            ent = [{"op": op, "value": tot[i], "nn": nn_tot[i]} for i in range(len(starts))]
        else:
            vals = col if op.endswith("f64") else col.view(np.int64)
            ent = _reduce_segments(op, vals, nn > 0, starts, keep_terms=True)
            for i, e in enumerate(ent):
                e["nn"] = nn_tot[i]
                e.pop("abs_sum", None)
                e.pop("n_nonnull", None)
        per_agg.append(ent)
    return _assemble(keys, keynull, order, starts, per_agg)


def _merge_entry(a, b):
    op = a["op"]
    assert op == b["op"]
    out = {"op": op, "nn": a["nn"] + b["nn"]}
    va, vb = a["value"], b["value"]
    if op == "sum_f64":
        for f in ("abs_sum", "n_nonnull"):
            if f in a and f in b:
                out[f] = a[f] + b[f]
        if "terms" in a and "terms" in b:
            out["terms"] = a["terms"] + b["terms"]
            out["value"] = fsum_ext(out["terms"]) if out["nn"] else None
            return out
    if va is None or vb is None:
        out["value"] = vb if va is None else va
    elif op == "count":
        out["value"] = va + vb
    elif op == "sum_i64":
        out["value"] = to_signed64(va + vb)
    elif op == "sum_f64":
        out["value"] = fsum_ext([va, vb])
    elif op in ("min_i64", "max_i64"):
        out["value"] = min(va, vb) if op == "min_i64" else max(va, vb)
    else:
        pick = min if op == "min_f64" else max
        out["value"] = pick(va, vb, key=total_order_key)
    return out


def merge_dict_by_value(groups, dict_values):
    """Re-key groups whose dict32 key components are dictionary INDICES by the value
    bytes instead, merging groups that collapse (duplicate dictionary values under
    different indices). dict_values: {key position: list of value bytes}. A NULL
    component stays bits 0 (its keynull bit tells it apart from a value)."""
    out = {}
    for (bits, mask), entries in groups.items():
        nb = list(bits)
        for pos, values in dict_values.items():
            if not (mask >> pos) & 1:
                nb[pos] = bytes(values[bits[pos]])
        gid = (tuple(nb), mask)
        if gid in out:
            out[gid] = [_merge_entry(a, b) for a, b in zip(out[gid], entries)]
        else:
            out[gid] = [dict(e) for e in entries]
    return out
