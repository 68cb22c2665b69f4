"""sortref.py — exact model of the per-partition sort / top-k above the shuffle.

Like finalagg.py this is a numpy statement of semantics, not a compute path: nothing here
touches the device. ordered_words restates the ordered words of dd_sort.hip (the null rank
bit and the unsigned ordered value of a key), so the model and the kernel cannot disagree
about an order; sort_ref sorts by them.

A row sorts by the tuple (partition; null rank_1, value_1; ...; null rank_n, value_n; input
rank), every component unsigned and ascending. The input rank is the row index, so the sort
is stable and every bit of the result is determined.
"""

import numpy as np

from datafusion_distributed_amd import finalagg

KEY_DTYPES = ("u8", "bool", "i16", "i32", "i64", "f32", "f64", "dec128")
MAX_KEYS = 4

_SIGN64 = np.uint64(1 << 63)
_UINT = {"i16": np.uint16, "i32": np.uint32, "i64": np.uint64, "f32": np.uint32,
         "f64": np.uint64}
_SRC = {"i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32,
        "f64": np.float64}


def _dec_words(col):
    data = np.asarray(col["data"])
    if data.dtype != np.uint64 or data.ndim != 2:
        data = np.ascontiguousarray(data).reshape(-1).view(np.uint8).view(np.uint64)
    return data.reshape(-1, 2)


def ordered_words(col, descending=False, nulls_first=False):
    """(null_rank u8[n], [value words u64[n], most significant first]) of a key column dict.

    Null rank, 0 sorts first: nulls_first -> NULL 0, valid 1; otherwise NULL 1, valid 0.
    Ordered value (unsigned order == key order): u8 / bool the value; signed integers the
    value with the sign bit flipped at the dtype's own width; floats the totalOrder key of
    the RAW bit pattern (sign set -> ~bits, sign clear -> bits | sign; nothing canonicalised);
    dec128 two words (hi with the sign flipped, lo). All complemented at the dtype's width
    when descending. A NULL's value is 0 and its value bytes are never looked at."""
    dt = col["dtype"]
    if dt not in KEY_DTYPES:
        raise ValueError(f"sort: a {dt} column is not a sort key")
    if dt in ("u8", "bool"):
        words = [np.ascontiguousarray(col["data"], dtype=np.uint8).astype(np.uint64)]
        width = 8
    elif dt == "dec128":
        w = _dec_words(col)
        words = [w[:, 1] ^ _SIGN64, w[:, 0].copy()]
        width = 64
    else:
        u = _UINT[dt]
        width = 8 * np.dtype(u).itemsize
        bits = np.ascontiguousarray(col["data"], dtype=_SRC[dt]).view(u)
        sign = u(1 << (width - 1))
        if dt in ("f32", "f64"):
            key = np.where((bits & sign) != 0, ~bits, bits | sign)
        else:
            key = bits ^ sign
        words = [key.astype(np.uint64)]
    if descending:
        mask = np.uint64((1 << width) - 1)
        words = [~w & mask for w in words]
    n = len(words[0])
    valid = col.get("valid")
    isnull = np.zeros(n, dtype=bool) if valid is None else np.asarray(valid) == 0
    words = [np.where(isnull, np.uint64(0), w) for w in words]
    rank = (isnull != bool(nulls_first)).astype(np.uint8)
    return rank, words


def check_keys(keys, n_cols):
    """Raise ValueError unless keys is 1..4 of (col, descending, nulls_first) within n_cols;
    returns them as a list of (int, bool, bool)."""
    keys = [(int(c), bool(d), bool(nf)) for c, d, nf in keys]
    if not 1 <= len(keys) <= MAX_KEYS:
        raise ValueError("sort: 1..4 sort keys")
    for c, _, _ in keys:
        if not 0 <= c < n_cols:
            raise ValueError("sort: key column index out of range")
    return keys


def _n_rows(col):
    if col["dtype"] == "dec128":
        return len(_dec_words(col))
    return len(np.asarray(col["data"]))


def _take(col, perm):
    data = _dec_words(col) if col["dtype"] == "dec128" else np.asarray(col["data"])
    out = {"dtype": col["dtype"], "data": np.ascontiguousarray(data[perm])}
    if col.get("valid") is not None:
        out["valid"] = np.ascontiguousarray(np.asarray(col["valid"], dtype=np.uint8)[perm])
    return out


def sort_ref(cols, keys, layout=None, fetch=None, proj=None):
    """Exact per-partition stable sort / top-k of column dicts.

    keys: 1..4 of (col, descending, nulls_first). layout: {"seg_offsets", "seg_part",
    "n_parts"} (default one segment, one partition). fetch: None keeps all rows, k >= 0 the
    first min(k, rows_p) of each partition. proj: column indices to gather (default all).
    Returns {"perm": u32[n_out] source row of each output row, "seg_offsets": i64[n_parts +
    1] (one segment per partition, partition-major), "cols": the gathered column dicts}."""
    keys = check_keys(keys, len(cols))
    if fetch is not None and fetch < 0:
        raise ValueError("sort: fetch must be None or >= 0")
    n = _n_rows(cols[0])
    if layout is None:
        layout = {"seg_offsets": [0, n], "seg_part": [0], "n_parts": 1}
    off, part, n_parts = finalagg.check_layout(n, layout["seg_offsets"], layout["seg_part"],
                                               layout["n_parts"])
    pid = np.repeat(part.astype(np.int64), np.diff(off))
    # np.lexsort: the LAST key is the primary one; the input rank closes the tuple
    order = [np.arange(n, dtype=np.int64)]
    for c, desc, nf in reversed(keys):
        rank, words = ordered_words(cols[c], desc, nf)
        order.extend(reversed(words))
        order.append(rank)
    order.append(pid)
    perm = np.lexsort(order) if n else np.zeros(0, dtype=np.int64)
    rows_p = np.bincount(pid, minlength=n_parts).astype(np.int64)
    keep_p = rows_p if fetch is None else np.minimum(rows_p, fetch)
    in_off = np.concatenate([[0], np.cumsum(rows_p)])
    seg_offsets = np.concatenate([[0], np.cumsum(keep_p)]).astype(np.int64)
    kept = [perm[in_off[p]:in_off[p] + keep_p[p]] for p in range(n_parts)]
    perm = (np.concatenate(kept) if kept else perm).astype(np.uint32)
    if proj is None:
        proj = range(len(cols))
    return {"perm": perm, "seg_offsets": seg_offsets,
            "cols": [_take(cols[c], perm) for c in proj]}


def collapsed_layout(n_rows):
    """The one-partition layout over n_rows rows: sort_topk over a sorted result with this
    layout and the same fetch is the SortPreservingMergeExec(fetch) above the partitions (its
    stable tie order is partition order, the order a merge takes ties in)."""
    return {"seg_offsets": np.array([0, n_rows], dtype=np.int64),
            "seg_part": np.zeros(1, dtype=np.int32), "n_parts": 1}
