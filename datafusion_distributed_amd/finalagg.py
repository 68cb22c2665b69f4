"""finalagg.py — exact model of the final aggregation above the shuffle.

Like decagg.py this is a numpy / Python-int statement of semantics, not a compute path:
nothing here touches the device. The input is a batch of PARTIAL STATES (column dicts) plus
a segment layout; rows of all segments with one partition id form a partition, groups are
formed within a partition, and the merge of one partition is decagg.final_merge_dec over
its rows, so group identity (oracle.reduce_ref.key_bits) and every merge rule are the
models the partial aggregate is already held to.

table_slots and home_slot restate the claim table's arithmetic (dd_final.hip), so a test
can aim rows at one slot.
"""

import numpy as np

from datafusion_distributed_amd import decagg
from oracle import pyref
from oracle import reduce_ref as rr

MIN_SLOTS = 64


def table_slots(rows_p):
    """Slots of the claim-table region of a partition holding rows_p rows:
    max(64, next_pow2(2 * rows_p)). The load never passes 0.5."""
    slots = MIN_SLOTS
    while slots < 2 * rows_p:
        slots <<= 1
    return slots


def home_slot(h, slots):
    """Home slot of a row with row hash h (pyref.hash_cols) in a region of `slots` slots:
    the HIGH log2(slots) bits of mix64(h). Every row of a shuffled partition shares
    h % P_total, so low bits of h would pile a partition onto a few slots."""
    lg = int(slots).bit_length() - 1
    assert slots == 1 << lg and slots >= MIN_SLOTS, "slots must be a power of two >= 64"
    if isinstance(h, np.ndarray):
        return (pyref.mix64_np(h) >> np.uint64(64 - lg)).astype(np.int64)
    return pyref.mix64_scalar(int(h)) >> (64 - lg)


def check_layout(n_rows, seg_offsets, seg_part, n_parts):
    """Raise ValueError unless (seg_offsets, seg_part, n_parts) is a well-formed layout of
    n_rows rows; returns them as (int64[S + 1], int32[S], int)."""
    off = np.asarray(seg_offsets, dtype=np.int64)
    part = np.asarray(seg_part, dtype=np.int32)
    if len(part) < 1 or len(off) != len(part) + 1 or n_parts < 1:
        raise ValueError("segment layout: seg_offsets must have one entry more than seg_part")
    if off[0] != 0 or off[-1] != n_rows or (np.diff(off) < 0).any():
        raise ValueError("segment layout: seg_offsets must be non-decreasing from 0 to n_rows")
    if (part < 0).any() or (part >= n_parts).any():
        raise ValueError("segment layout: seg_part outside [0, n_parts)")
    return off, part, int(n_parts)


def partition_rows(seg_offsets, seg_part, n_parts):
    """Per partition: the input row indices of its segments, in segment order."""
    rows = [[] for _ in range(n_parts)]
    for s, p in enumerate(np.asarray(seg_part).tolist()):
        rows[p].append(np.arange(seg_offsets[s], seg_offsets[s + 1], dtype=np.int64))
    return [np.concatenate(r) if r else np.zeros(0, dtype=np.int64) for r in rows]


def _state_words(col, op, idx):
    """(lo u64, hi u64) of a state column's rows idx."""
    if op == "sum_dec128":
        data = np.asarray(col["data"])
        if data.dtype != np.uint64 or data.ndim != 2:
            data = np.ascontiguousarray(data).reshape(-1).view(np.uint8).view(np.uint64)
        words = data.reshape(-1, 2)[idx]
        return words[:, 0].copy(), words[:, 1].copy()
    want = np.float64 if op.endswith("f64") else np.int64
    lo = np.ascontiguousarray(col["data"], dtype=want)[idx].view(np.uint64)
    return lo, np.zeros(len(idx), dtype=np.uint64)


def final_merge_ref(cols, key_idx, aggs, seg_offsets=None, seg_part=None, n_parts=1):
    """Exact final aggregation of the partial states in `cols` (column dicts).

    aggs: 1..8 of (state_col, op, nn_col) with op in api.AGG_OPS; nn_col is the i64 column
    of non-null input counts (None for "count", whose nn is the merged count). Validity
    buffers of state and nn columns are ignored. Returns [{gid: entries} per partition]
    with gid = (key_bits_tuple, keynull_mask) and entries as decagg.final_merge_dec's."""
    n = len(np.asarray(cols[key_idx[0]]["data"]))
    if seg_offsets is None:
        seg_offsets, seg_part, n_parts = [0, n], [0], 1  # a plain global group-by
    off, part, n_parts = check_layout(n, seg_offsets, seg_part, n_parts)
    keys, keynull = rr.key_bits(cols, key_idx)
    ops = [op for _, op, _ in aggs]
    out = []
    for idx in partition_rows(off, part, n_parts):
        m = len(idx)
        lo = np.zeros((m, len(aggs)), dtype=np.uint64)
        hi = np.zeros((m, len(aggs)), dtype=np.uint64)
        nn = np.zeros((m, len(aggs)), dtype=np.uint64)
        for g, (sc, op, nc) in enumerate(aggs):
            lo[:, g], hi[:, g] = _state_words(cols[sc], op, idx)
            if op == "count":
                nn[:, g] = lo[:, g]
            else:
                nn[:, g] = np.ascontiguousarray(cols[nc]["data"], dtype=np.int64)[idx].view(
                    np.uint64)
            if op == "sum_dec128":
                # final_merge_dec adds every partial's words, trusting the (0, 0) that
                # partial_reduce writes at nn == 0; here the rule is stated outright: such
                # a partial is skipped, whatever its words hold
                lo[nn[:, g] == 0, g] = 0
                hi[nn[:, g] == 0, g] = 0
        res = {"keys": keys[idx], "keynull": keynull[idx], "aggs": lo.view(np.float64),
               "aggs_hi": hi, "nn": nn}
        out.append(decagg.final_merge_dec(res, ops) if m else {})
    return out


# ---------------- partial states as columns ----------------

_KEY_NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.uint16, "i32": np.uint32,
           "f32": np.uint32, "i64": np.uint64, "f64": np.uint64}
_KEY_VIEW = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32,
             "f32": np.float32, "i64": np.int64, "f64": np.float64}


def partial_state_cols(res, key_dtypes, ops):
    """Lay partial rows (api.partial_reduce's return value, or any dict with its "keys",
    "keynull", "aggs", "aggs_hi" and "nn") out as the columns the shuffle carries and
    final_merge reads: one key column per key (dtype from key_dtypes, validity from
    keynull, None when no row is NULL), then per aggregate its state column (i64, f64 or
    dec128) followed, for every op but "count", by its i64 nn column.
    Returns (cols, key_idx, aggs) with aggs as final_merge takes them."""
    keys = np.asarray(res["keys"], dtype=np.uint64).reshape(-1, len(key_dtypes))
    keynull = np.asarray(res["keynull"], dtype=np.uint32)
    lo = np.ascontiguousarray(res["aggs"], dtype=np.float64).view(np.uint64)
    hi = np.asarray(res["aggs_hi"], dtype=np.uint64)
    nn = np.asarray(res["nn"], dtype=np.uint64)
    cols = []
    for k, dt in enumerate(key_dtypes):
        isnull = ((keynull >> np.uint32(k)) & np.uint32(1)).astype(bool)
        data = np.ascontiguousarray(keys[:, k].astype(_KEY_NP[dt])).view(_KEY_VIEW[dt])
        cols.append({"dtype": dt, "data": data,
                     "valid": (~isnull).astype(np.uint8) if isnull.any() else None})
    aggs = []
    for g, op in enumerate(ops):
        sc = len(cols)
        if op == "sum_dec128":
            cols.append({"dtype": "dec128", "valid": None,
                         "data": np.ascontiguousarray(np.stack([lo[:, g], hi[:, g]], axis=1))})
        elif op.endswith("f64"):
            cols.append({"dtype": "f64", "valid": None,
                         "data": np.ascontiguousarray(lo[:, g]).view(np.float64)})
        else:
            cols.append({"dtype": "i64", "valid": None,
                         "data": np.ascontiguousarray(lo[:, g]).view(np.int64)})
        if op == "count":
            aggs.append((sc, op, None))
            continue
        cols.append({"dtype": "i64", "valid": None,
                     "data": np.ascontiguousarray(nn[:, g]).view(np.int64)})
        aggs.append((sc, op, sc + 1))
    return cols, list(range(len(key_dtypes))), aggs


def groups_as_partials(groups_list, n_keys, ops, poison=None):
    """Model results ({gid: entries} dicts, e.g. decagg.reduce_dec_ref over blocks of rows)
    as partial rows in api.partial_reduce's shape, one row per group per dict, in order.
    A group whose aggregate saw no non-null input (value None, nn 0) gets the value bits
    poison[op] (default 0): whatever they are, a merge must never read them."""
    poison = poison or {}
    keys, keynull, lo, hi, nn = [], [], [], [], []
    for groups in groups_list:
        for (bits, mask), entries in groups.items():
            keys.append(bits)
            keynull.append(mask)
            rlo, rhi, rnn = [], [], []
            for e in entries:
                v, op = e["value"], e["op"]
                h = 0
                if v is None:
                    w = poison.get(op, 0)
                    if op == "sum_dec128":
                        w, h = w & ((1 << 64) - 1), (w >> 64) & ((1 << 64) - 1)
                elif op == "sum_dec128":
                    w, h = (int(x) for x in decagg.dec_words([v])[0])
                elif op == "sum_f64":
                    w = int(np.float64(v).view(np.uint64))
                else:  # integers as their i64 bits; min_f64 / max_f64 are bit patterns already
                    w = int(v) & ((1 << 64) - 1)
                rlo.append(w)
                rhi.append(h)
                rnn.append(e["nn"])
            lo.append(rlo)
            hi.append(rhi)
            nn.append(rnn)
    na = len(ops)
    return {"keys": np.array(keys, dtype=np.uint64).reshape(-1, n_keys),
            "keynull": np.array(keynull, dtype=np.uint32),
            "aggs": np.array(lo, dtype=np.uint64).reshape(-1, na).view(np.float64),
            "aggs_hi": np.array(hi, dtype=np.uint64).reshape(-1, na),
            "nn": np.array(nn, dtype=np.uint64).reshape(-1, na)}
