"""hashjoin.py — exact model of the partitioned hash join above two shuffles.

Like finalagg.py this is a plain Python / numpy statement of semantics, not a compute path:
nothing here touches the device. Two batches (column dicts), each with a segment layout in
the §18.1 form; partition p of the build side joins partition p of the probe side and
nothing else. Key identity is oracle.reduce_ref.key_bits (the raw value of an integer key),
and a row with a NULL in any key component matches nothing.

The output follows the EMITTING side (probe for inner / right_*, build for left_*): its row
order, and its segments with new offsets. hash_join_ref returns, per segment of that side,
the list of (build_row, probe_row) pairs (inner; a probe row's matches adjacent, here in
ascending build row, which the kernels do not promise) or of row ids (semi / anti).

The outer joins (left, right, full) have a model of their own,
outer_join_ref: their output has two sections of segments and pairs with an absent side.
"""

import numpy as np

from datafusion_distributed_amd import finalagg
from oracle import reduce_ref as rr

JOIN_TYPES = ("inner", "left_semi", "left_anti", "right_semi", "right_anti")
OUTER_JOIN_TYPES = ("left", "right", "full")  # outer_join_ref, DESIGN.md §20
KEY_DTYPES = ("u8", "bool", "i16", "i32", "i64")


def n_rows_of(cols):
    """Rows of a batch of fixed-width column dicts."""
    data = np.asarray(cols[0]["data"])
    return len(data.reshape(-1, 2)) if cols[0]["dtype"] == "dec128" and data.ndim != 2 \
        else len(data)


def default_layout(n):
    """One segment, one partition: a plain hash join."""
    return {"seg_offsets": np.array([0, n], dtype=np.int64),
            "seg_part": np.zeros(1, dtype=np.int32), "n_parts": 1}


def _side(cols, keys, layout):
    n = n_rows_of(cols)
    layout = layout or default_layout(n)
    off, part, n_parts = finalagg.check_layout(n, layout["seg_offsets"], layout["seg_part"],
                                               layout["n_parts"])
    for k in keys:
        if cols[k]["dtype"] not in KEY_DTYPES:
            raise ValueError(f"hash join: a {cols[k]['dtype']} key is not supported")
    bits, keynull = rr.key_bits(cols, list(keys))
    ident = [None if m else tuple(b) for b, m in zip(bits.tolist(), keynull.tolist())]
    return n, off, part, n_parts, ident


def hash_join_ref(build_cols, build_keys, probe_cols, probe_keys, join_type="inner",
                  build_layout=None, probe_layout=None):
    """The join's pairs or row ids, one list per segment of the emitting side, in the
    specified order. See the module docstring."""
    if join_type not in JOIN_TYPES:
        raise ValueError(f"hash join: unknown or unsupported join type {join_type!r}")
    if not 1 <= len(build_keys) <= 4 or len(build_keys) != len(probe_keys):
        raise ValueError("hash join: 1..4 key columns per side")
    for b, p in zip(build_keys, probe_keys):
        if build_cols[b]["dtype"] != probe_cols[p]["dtype"]:
            raise ValueError("hash join: key dtypes differ pairwise")
    _, boff, bpart, bparts, bid = _side(build_cols, build_keys, build_layout)
    _, poff, ppart, pparts, pid = _side(probe_cols, probe_keys, probe_layout)
    if bparts != pparts:
        raise ValueError("hash join: n_parts of the two sides differ")

    # per partition: key identity -> build rows, in row order
    tables = []
    for rows in finalagg.partition_rows(boff, bpart, bparts):
        t = {}
        for r in rows.tolist():
            if bid[r] is not None:
                t.setdefault(bid[r], []).append(r)
        tables.append(t)

    out = []
    if join_type in ("inner", "right_semi", "right_anti"):
        for s, p in enumerate(ppart.tolist()):
            seg = []
            for r in range(int(poff[s]), int(poff[s + 1])):
                hits = tables[p].get(pid[r], ()) if pid[r] is not None else ()
                if join_type == "inner":
                    seg.extend((b, r) for b in hits)
                elif bool(hits) == (join_type == "right_semi"):
                    seg.append(r)
            out.append(seg)
        return out

    # left_semi / left_anti: which build rows have a probe row with their key
    seen = [set() for _ in range(bparts)]
    for p, rows in enumerate(finalagg.partition_rows(poff, ppart, pparts)):
        seen[p].update(pid[r] for r in rows.tolist() if pid[r] is not None)
    for s, p in enumerate(bpart.tolist()):
        seg = []
        for r in range(int(boff[s]), int(boff[s + 1])):
            hit = bid[r] is not None and bid[r] in seen[p]
            if hit == (join_type == "left_semi"):
                seg.append(r)
        out.append(seg)
    return out


def outer_join_ref(build_cols, build_keys, probe_cols, probe_keys, join_type,
                   build_layout=None, probe_layout=None):
    """The outer joins of DESIGN.md §20: one list per OUTPUT segment of
    (build_row | None, probe_row | None).

    Section 1, the probe side's segments: per probe row, in row order, its inner pairs (in
    ascending build row, which the kernels do not promise) or, for right / full, one
    (None, row) when it has none. Section 2, left / full only, the build side's segments:
    the build rows no probe row matched, in row order, as (row, None). A NULL-key row is a
    row without a match."""
    if join_type not in OUTER_JOIN_TYPES:
        raise ValueError(f"outer join: unknown or unsupported join type {join_type!r} "
                         "(hash_join_ref serves the others)")
    if not 1 <= len(build_keys) <= 4 or len(build_keys) != len(probe_keys):
        raise ValueError("outer join: 1..4 key columns per side")
    for b, p in zip(build_keys, probe_keys):
        if build_cols[b]["dtype"] != probe_cols[p]["dtype"]:
            raise ValueError("outer join: key dtypes differ pairwise")
    _, boff, bpart, bparts, bid = _side(build_cols, build_keys, build_layout)
    _, poff, ppart, pparts, pid = _side(probe_cols, probe_keys, probe_layout)
    if bparts != pparts:
        raise ValueError("outer join: n_parts of the two sides differ")

    tables = []
    for rows in finalagg.partition_rows(boff, bpart, bparts):
        t = {}
        for r in rows.tolist():
            if bid[r] is not None:
                t.setdefault(bid[r], []).append(r)
        tables.append(t)

    keep_probe = join_type in ("right", "full")
    matched = set()
    out = []
    for s, p in enumerate(ppart.tolist()):
        seg = []
        for r in range(int(poff[s]), int(poff[s + 1])):
            hits = tables[p].get(pid[r], ()) if pid[r] is not None else ()
            seg.extend((b, r) for b in hits)
            matched.update(hits)
            if not hits and keep_probe:
                seg.append((None, r))
        out.append(seg)
    if join_type in ("left", "full"):
        for s in range(len(bpart)):
            out.append([(r, None) for r in range(int(boff[s]), int(boff[s + 1]))
                        if r not in matched])
    return out


def seg_offsets_of(segments):
    """The output seg_offsets the model's per-segment lists imply."""
    off = np.zeros(len(segments) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in segments], out=off[1:])
    return off
