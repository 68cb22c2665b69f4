"""views.py — Utf8View / BinaryView columns: host models and the pyarrow boundary.

ingest_ref / emit_ref are the pure-numpy statement of DESIGN.md §15 (what dd_view_ingest_run
and dd_view_emit_run compute on the device); the GPU tests compare the kernels with them bit
for bit. from_arrow / to_arrow move between pyarrow view arrays and the (views, valid,
buffers) triple of the C ABI. Arrow view layout, little-endian, 16 bytes per row: i32
length; length <= 12: the value, zero-padded; else a 4-byte prefix, i32 buffer_index, i32
offset into that data buffer.
"""

import numpy as np

INLINE_MAX = 12
INT32_MAX = 2**31 - 1


def _views_u8(views):
    v = np.ascontiguousarray(views, dtype=np.uint8)
    if v.ndim != 2 or v.shape[1] != 16:
        v = v.reshape(-1, 16)
    return v


def ingest_ref(views, valid, bufs):
    """Model of dd_view_ingest_run: (offsets i32[n+1], bytes u8). A null row has length 0
    and its view is never looked at. A valid row with a negative length, or a long row that
    points outside its data buffer, raises ValueError (the device returns
    DD_ERR_INVALID)."""
    v = _views_u8(views)
    n = len(v)
    words = v.view(np.int32).reshape(n, 4)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    bufs = [np.asarray(b, dtype=np.uint8) for b in bufs]
    lens = np.where(ok, words[:, 0], 0).astype(np.int64)
    if (lens < 0).any():
        raise ValueError("ingest_ref: negative length on a valid row")
    parts = []
    for i in np.flatnonzero(lens > 0):
        ln = int(lens[i])
        if ln <= INLINE_MAX:
            parts.append(v[i, 4:4 + ln])
            continue
        bi, off = int(words[i, 2]), int(words[i, 3])
        if not 0 <= bi < len(bufs) or off < 0 or off + ln > len(bufs[bi]):
            raise ValueError(f"ingest_ref: row {i} points outside its data buffer")
        parts.append(bufs[bi][off:off + ln])
    total = int(lens.sum())
    if total > INT32_MAX:
        raise ValueError("ingest_ref: value bytes exceed INT32_MAX")
    offsets = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=offsets[1:])
    data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return offsets, np.ascontiguousarray(data, dtype=np.uint8)


def emit_ref(lengths, valid, data, row_off, byte_off, W):
    """Model of dd_view_emit_run over a partitioner's utf8 output: lengths u32[n]
    (partition-major), valid u8[n] or None, data u8 (partition p's bytes start at
    byte_off[p], rows back to back), row_off / byte_off i64[P+1].
    Returns {"views": u8[n,16], "long_byte_off": i64[W+1], "bytes": [u8 per window]}."""
    row_off = np.asarray(row_off, dtype=np.int64)
    byte_off = np.asarray(byte_off, dtype=np.int64)
    P = len(row_off) - 1
    if W <= 0 or P % W != 0:
        raise ValueError("emit_ref: n_windows must be > 0 and divide the partition count")
    lengths = np.asarray(lengths).astype(np.int64)
    data = np.asarray(data, dtype=np.uint8)
    n = len(lengths)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    start = np.zeros(n, dtype=np.int64)
    for p in range(P):
        r0, r1 = int(row_off[p]), int(row_off[p + 1])
        if r1 > r0:
            start[r0:r1] = byte_off[p] + np.cumsum(lengths[r0:r1]) - lengths[r0:r1]
    views = np.zeros((n, 16), dtype=np.uint8)
    words = views.view(np.int32).reshape(n, 4)
    ppw = P // W
    long_off = np.zeros(W + 1, dtype=np.int64)
    bufs = []
    for w in range(W):
        r0, r1 = int(row_off[w * ppw]), int(row_off[(w + 1) * ppw])
        parts, pos = [], 0
        for i in range(r0, r1):
            if not ok[i]:
                continue
            ln, s = int(lengths[i]), int(start[i])
            words[i, 0] = ln
            if ln <= INLINE_MAX:
                views[i, 4:4 + ln] = data[s:s + ln]
            else:
                views[i, 4:8] = data[s:s + 4]
                words[i, 2] = 0
                words[i, 3] = pos
                parts.append(data[s:s + ln])
                pos += ln
        if pos > INT32_MAX:
            raise ValueError(f"emit_ref: window {w} holds more than INT32_MAX long bytes")
        bufs.append(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8))
        long_off[w + 1] = long_off[w] + pos
    return {"views": views, "long_byte_off": long_off, "bytes": bufs}


def from_arrow(arr):
    """(views u8[n,16], valid u8[n] or None, [data buffers u8]) of a pa.string_view() /
    pa.binary_view() array. Honours arr.offset; the validity bitmap is unpacked."""
    import pyarrow as pa

    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if not (pa.types.is_string_view(arr.type) or pa.types.is_binary_view(arr.type)):
        raise TypeError(f"from_arrow: not a view array: {arr.type}")
    bufs = arr.buffers()
    n, off = len(arr), arr.offset
    if n and bufs[1] is not None:
        views = np.frombuffer(bufs[1], dtype=np.uint8)[off * 16:(off + n) * 16]
        views = views.reshape(n, 16).copy()
    else:
        views = np.zeros((n, 16), dtype=np.uint8)
    valid = None
    if bufs[0] is not None and arr.null_count:
        bits = np.unpackbits(np.frombuffer(bufs[0], dtype=np.uint8), bitorder="little")
        valid = np.ascontiguousarray(bits[off:off + n], dtype=np.uint8)
    data = [np.frombuffer(b, dtype=np.uint8) if b is not None and b.size
            else np.zeros(0, dtype=np.uint8) for b in bufs[2:]]
    return views, valid, data


def to_arrow(views, valid, buffer, binary=False):
    """A pa.string_view() (or pa.binary_view()) array over views u8[n,16], valid u8[n] or
    None and ONE data buffer (what emit produces: buffer_index is always 0)."""
    import pyarrow as pa

    v = _views_u8(views)
    n = len(v)
    vbuf = None
    if valid is not None:
        vbuf = pa.py_buffer(np.packbits(np.asarray(valid).astype(bool),
                                        bitorder="little").tobytes())
    bufs = [vbuf, pa.py_buffer(v.tobytes())]
    buffer = np.asarray(buffer, dtype=np.uint8)
    if buffer.size:
        bufs.append(pa.py_buffer(buffer.tobytes()))
    typ = pa.binary_view() if binary else pa.string_view()
    return pa.Array.from_buffers(typ, n, bufs)
