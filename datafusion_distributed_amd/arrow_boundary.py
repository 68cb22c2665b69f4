"""arrow_boundary.py — materialize per-partition Arrow RecordBatches at the host boundary.

This is the boundary conversion DESIGN.md §4 specifies: inside the device path validity is
unpacked u8 and var-width data is (lengths, bytes, partition byte offsets); at the consumer
boundary those become real Arrow arrays — validity re-packed to bitmaps, offsets rebuilt per
partition — exactly what the Rust shim's `streams_from_partitioner` does in INTEGRATION.md.
`batch_size` slicing mirrors RepartitionExec's output coalescing
(src/distributed_planner/distributed_config.rs:39-45): partitions are emitted as
<= batch_size row batches.
"""

import numpy as np


def _arrow():
    import pyarrow as pa

    return pa


_PA_TYPE = {
    "u8": "uint8", "i16": "int16", "i32": "int32", "i64": "int64",
    "f32": "float32", "f64": "float64", "bool": "uint8",
}


def _validity_mask(valid_u8):
    return valid_u8.astype(bool) if valid_u8 is not None else None


def _utf8_values(pa, offsets, data):
    # Rebuild values from the raw offsets/bytes buffers: the device path hashes/moves raw
    # bytes, so round-tripping through str would silently mutate (or mask) non-UTF8
    # dictionary bytes.
    doff = np.asarray(offsets, dtype=np.int32)
    dbuf = np.asarray(data, dtype=np.uint8)
    return pa.StringArray.from_buffers(
        len(doff) - 1, pa.py_buffer(doff.tobytes()), pa.py_buffer(dbuf.tobytes()), None)


def partition_batches(part, lo, hi, batch_size=8192, gc=None, views=None):
    """Arrow RecordBatches for partitions [lo, hi) of a run Partitioner (downloads the
    partition-major buffers once and slices views). Yields (partition, RecordBatch).

    gc: optional {col: DictGC} run with n_windows == part.nparts (one dictionary per
    partition, the reference's per-batch granularity, worker_service.rs:363-433): those
    columns' DictionaryArrays use the remapped indices and the partition's compacted
    dictionary. Without it every batch carries the full input dictionary.

    views: optional {col: ViewEmit} run with n_windows == part.nparts: those utf8 columns
    come out as pa.string_view() arrays over the partition's compact data buffer (every
    batch of a partition shares that one buffer: slicing at batch_size copies nothing).
    Without it they are pa.string() arrays, as before."""
    pa = _arrow()
    gc = gc or {}
    views = views or {}
    ve_views, ve_bufs = {}, {}
    for i, e in views.items():
        if e.n_windows != part.nparts or e.part is not part or e.col != i:
            raise ValueError("partition_batches: ViewEmit must be run on this partitioner "
                             "and column with n_windows == part.nparts")
        ve_views[i] = e.views()
    gc_idx = {}
    for i, g in gc.items():
        if g.n_windows != part.nparts or g.part is not part:
            raise ValueError("partition_batches: DictGC must be run on this partitioner "
                             "with n_windows == part.nparts")
        gc_idx[i] = g.indices()
    roff = part.row_offsets()
    cols_meta = part.batch.cols
    fixed = {}
    lens = {}
    var_bytes = {}
    var_boff = {}
    valid = {}
    for i, c in enumerate(cols_meta):
        out = part.col_out(i)
        if i in views:
            pass  # the emit object holds this column's views and buffers
        elif c["dtype"] in ("utf8", "utf8view"):
            lens[i] = out["lengths"]
            var_bytes[i] = out["data"]
            var_boff[i] = part.byte_offsets(i)
        else:
            fixed[i] = out["data"]
        if "valid" in out:
            valid[i] = out["valid"]

    for p in range(lo, hi):
        r0, r1 = int(roff[p]), int(roff[p + 1])
        pdict = {}  # this partition's compacted dictionaries (gc columns)
        # one empty batch for an empty partition (the reference emits empty streams)
        slices = [(r0, r0)] if r1 == r0 else [
            (b0, min(b0 + batch_size, r1)) for b0 in range(r0, r1, batch_size)]
        for b0, b1 in slices:
            arrays, names = [], []
            for i, c in enumerate(cols_meta):
                name = c.get("name", f"c{i}")
                mask = None
                if i in valid:
                    mask = ~_validity_mask(valid[i][b0:b1])
                if i in views:
                    if ve_bufs.get(i, (None,))[0] != p:  # one partition's buffer at a time
                        ve_bufs[i] = (p, pa.py_buffer(views[i].window_bytes(p).tobytes()))
                    arr = pa.Array.from_buffers(
                        pa.string_view(), b1 - b0,
                        [pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
                         if mask is not None else None,
                         pa.py_buffer(ve_views[i][b0:b1].tobytes()), ve_bufs[i][1]])
                elif c["dtype"] in ("utf8", "utf8view"):
                    seg_lens = lens[i][b0:b1].astype(np.int64)
                    start = int(var_boff[i][p]) + int(
                        lens[i][r0:b0].astype(np.int64).sum())
                    nbytes = int(seg_lens.sum())
                    offsets = np.zeros(len(seg_lens) + 1, dtype=np.int32)
                    np.cumsum(seg_lens, out=offsets[1:])
                    arr = pa.StringArray.from_buffers(
                        b1 - b0,
                        pa.py_buffer(offsets.tobytes()),
                        pa.py_buffer(var_bytes[i][start:start + nbytes].tobytes()),
                        pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
                        if mask is not None else None,
                    )
                elif c["dtype"] == "dict32" and i in gc:
                    idx = pa.array(gc_idx[i][b0:b1], type=pa.int32(), mask=mask)
                    if i not in pdict:
                        pdict[i] = _utf8_values(pa, *gc[i].window_dict(p))
                    arr = pa.DictionaryArray.from_arrays(idx, pdict[i])
                elif c["dtype"] == "dict32":
                    idx = pa.array(fixed[i][b0:b1], type=pa.int32(), mask=mask)
                    values = _utf8_values(pa, c["dict_offsets"], c["dict_bytes"])
                    arr = pa.DictionaryArray.from_arrays(idx, values)
                elif c["dtype"] == "dec128":
                    # the partition-major buffer is already Arrow's value buffer; precision
                    # and scale come from the schema (the column dict), DESIGN.md §16
                    arr = pa.Array.from_buffers(
                        pa.decimal128(c.get("precision", 38), c.get("scale", 0)), b1 - b0,
                        [pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
                         if mask is not None else None,
                         pa.py_buffer(fixed[i][b0:b1].tobytes())])
                elif c["dtype"] == "bool":
                    arr = pa.array(fixed[i][b0:b1].astype(bool), type=pa.bool_(), mask=mask)
                else:
                    arr = pa.array(fixed[i][b0:b1], type=getattr(pa, _PA_TYPE[c["dtype"]])(),
                                   mask=mask)
                arrays.append(arr)
                names.append(name)
            yield p, pa.RecordBatch.from_arrays(arrays, names=names)
