"""dictgc.py — host-side model of the per-window dictionary GC. No GPU.

Reference: before a batch goes on the wire, src/protocol/grpc/worker_service.rs:363-433
compacts every dictionary column to the values that batch references
(garbage_collect_arrays -> arrow_select::dictionary::garbage_collect_any_dictionary) and
resends the compacted dictionary with it (DictionaryHandling::Resend). Mirrored semantics,
per window of contiguous partitions of the partitioner's partition-major output:

  - used(w) = dictionary indices referenced by a VALID row of the window
  - compacted dictionary = the values of used(w) in ascending original-index order, moved
    as raw bytes (empty and non-UTF-8 values survive; equal bytes at different indices
    stay two entries: GC is not dedup)
  - remapped index = rank of the old index within used(w); 0 for a null row
  - on the consumer, the producers' dictionaries are concatenated in producer-rank order
    and producer r's indices are rebased by the values received from producers < r

These two functions are the models the GPU tests compare the kernels with, bit for bit.
"""

import numpy as np


def gc_windows_ref(idx, valid, row_off, dict_offsets, dict_bytes, n_windows):
    """numpy statement of the GC semantics.

    idx: i32[n] partition-major dictionary indices; valid: u8[n] or None; row_off:
    i64[P+1] partition row offsets (P % n_windows == 0); dict_offsets/dict_bytes: the
    utf8 value list. Returns {"indices": i32[n], "val_off": i64[W+1], "byte_off":
    i64[W+1], "offsets": [W x i32[nvals_w+1]], "bytes": [W x u8[...]], "used": [W x
    i64[nvals_w]] (surviving original indices, ascending)}. Raises ValueError when a
    valid row's index is outside [0, dict_n)."""
    idx = np.asarray(idx, dtype=np.int32)
    row_off = np.asarray(row_off, dtype=np.int64)
    doff = np.asarray(dict_offsets, dtype=np.int64)
    dbytes = np.asarray(dict_bytes, dtype=np.uint8)
    dict_n = len(doff) - 1
    nparts = len(row_off) - 1
    if n_windows <= 0 or nparts % n_windows:
        raise ValueError("n_windows must be > 0 and divide the partition count")
    ok = np.ones(len(idx), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    if ((idx[ok] < 0) | (idx[ok] >= dict_n)).any():
        raise ValueError("a valid row's index is outside [0, dict_n)")
    ppw = nparts // n_windows
    out = np.zeros(len(idx), dtype=np.int32)
    val_off = np.zeros(n_windows + 1, dtype=np.int64)
    byte_off = np.zeros(n_windows + 1, dtype=np.int64)
    offsets, chunks, used_all = [], [], []
    for w in range(n_windows):
        r0, r1 = int(row_off[w * ppw]), int(row_off[(w + 1) * ppw])
        wi, wok = idx[r0:r1], ok[r0:r1]
        used = np.unique(wi[wok]).astype(np.int64)  # ascending original-index order
        out[r0:r1] = np.where(wok, np.searchsorted(used, wi), 0)
        lens = doff[used + 1] - doff[used]
        off = np.zeros(len(used) + 1, dtype=np.int32)
        np.cumsum(lens, out=off[1:])
        # byte gather: output byte b of value r comes from dict byte doff[used[r]] + b
        src = (np.arange(int(off[-1]), dtype=np.int64)
               + np.repeat(doff[used] - off[:-1].astype(np.int64), lens))
        offsets.append(off)
        chunks.append(dbytes[src])
        used_all.append(used)
        val_off[w + 1] = val_off[w] + len(used)
        byte_off[w + 1] = byte_off[w] + int(off[-1])
    return {"indices": out, "val_off": val_off, "byte_off": byte_off,
            "offsets": offsets, "bytes": chunks, "used": used_all}


def merge_producers_ref(producers):
    """Consumer-side model: `producers` is a list, in producer-rank order, of
    (indices i32[n_r], valid u8[n_r] or None, offsets i32[nvals_r+1], bytes u8[...]).

    Dictionaries are concatenated (duplicates across producers stay, as Arrow allows),
    every index of producer r is rebased by the values received from producers < r
    (null rows included: their slot is never decoded), and one zero-based i32 offsets
    array of total_vals + 1 entries is rebuilt. Returns {"indices", "valid" (None when
    no producer carries validity), "offsets", "bytes", "vals_per_producer"}."""
    idx_parts, valid_parts, off_parts, byte_parts, vals = [], [], [], [], []
    vbase = bbase = 0
    any_valid = any(p[1] is not None for p in producers)
    for indices, valid, offsets, data in producers:
        indices = np.asarray(indices, dtype=np.int32)
        offsets = np.asarray(offsets, dtype=np.int64)
        nv = len(offsets) - 1
        idx_parts.append(indices + np.int32(vbase))
        valid_parts.append(np.ones(len(indices), dtype=np.uint8) if valid is None
                           else np.asarray(valid, dtype=np.uint8))
        off_parts.append(offsets[:-1] + bbase)
        byte_parts.append(np.asarray(data, dtype=np.uint8)[:int(offsets[-1])])
        vals.append(nv)
        vbase += nv
        bbase += int(offsets[-1])
    if bbase > np.iinfo(np.int32).max:
        raise ValueError("received dictionary bytes exceed INT32_MAX")
    cat = lambda parts, dt: (np.concatenate(parts).astype(dt) if parts
                             else np.zeros(0, dtype=dt))
    offsets = np.append(cat(off_parts, np.int64), bbase).astype(np.int32)
    return {"indices": cat(idx_parts, np.int32),
            "valid": cat(valid_parts, np.uint8) if any_valid else None,
            "offsets": offsets, "bytes": cat(byte_parts, np.uint8),
            "vals_per_producer": np.asarray(vals, dtype=np.int64)}


def decode(indices, valid, offsets, data):
    """Materialize a dictionary column as a list of bytes / None (test helper)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    raw = np.asarray(data, dtype=np.uint8).tobytes()
    ok = np.ones(len(indices), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    return [raw[offsets[k]:offsets[k + 1]] if v else None for k, v in zip(indices, ok)]
