#!/usr/bin/env python3
"""bench_sort.py — measure the per-partition sort / top-k above the shuffle:

  (a) q3's shape: --rows-a rows in a P=128 partitioner layout, keys (dec128 DESC, i32 ASC),
      payload i64 + i32; run with fetch=10 and without
  (b) the pass-rate shape: --rows-b rows, one partition, one uniformly random i64 key (all 8
      passes run), a 4-byte payload

Per shape, alternately in one process, --reps runs after --warmup:

  gpu      api.sort_topk over the device batch: per-group hipEvent ms (encode + census,
           passes, segment output, gather), passes planned / run, and the wall time of the
           whole call
  host     the path a user had before: copy the same columns device-to-host, then pyarrow
           sort_indices + take, per partition for (a); copy and sort timed separately

A pass reads 12 B/row for the histogram, reads 12 B again and writes 12 B in the scatter
(8-byte word + 4-byte row id): bytes moved per pass are set against the practical streaming
ceiling of profiles/r02_patmax.txt. Medians with min-max. Prints one JSON document; --out also
writes it to a file. Needs a GPU (no fallback)."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from datafusion_distributed_amd import api  # noqa: E402

STREAM_CEILING_TBPS = 5.79  # profiles/r02_patmax.txt
PASS_BYTES_PER_ROW = 36


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def host_path(pa, pc, batch, cols, names, sort_keys, seg_offsets, fetch):
    """Device-to-host copy of every column, then per partition pyarrow sort_indices + take:
    (copy ms, sort ms, output rows)."""
    n = batch.n_rows
    t0 = time.perf_counter()
    host = [api._d2h(batch.desc.cols[i].data, n * api.ELEM_SIZE[c["dtype"]],
                     api.FIXED_NP[c["dtype"]]) for i, c in enumerate(cols)]
    t1 = time.perf_counter()
    arrays = []
    for c, h in zip(cols, host):
        if c["dtype"] == "dec128":
            arrays.append(pa.Array.from_buffers(pa.decimal128(38, 2), n,
                                                [None, pa.py_buffer(h)]))
        else:
            arrays.append(pa.array(h))
    table = pa.table(arrays, names=names)
    rows = 0
    for p in range(len(seg_offsets) - 1):
        part = table.slice(int(seg_offsets[p]), int(seg_offsets[p + 1] - seg_offsets[p]))
        idx = pc.sort_indices(part, sort_keys=sort_keys)
        if fetch is not None:
            idx = idx.slice(0, fetch)
        rows += part.take(idx).num_rows
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, rows


def measure(pa, pc, name, cols, names, keys, sort_keys, layout, fetch, warmup, reps):
    batch = api.DeviceBatch(cols)
    n = batch.n_rows
    groups = ("encode_census", "passes", "seg_out", "gather")
    ms = {k: [] for k in groups + ("kernels", "gpu_wall", "d2h_copy", "pyarrow_sort",
                                   "host_total")}
    info, out_rows, host_rows = {}, 0, 0
    try:
        for it in range(warmup + reps):
            t0 = time.perf_counter()
            s = api.sort_topk(batch, keys, layout, fetch)
            wall = (time.perf_counter() - t0) * 1e3
            kms, info, out_rows = s.kernel_ms(), s.info(), s.n_rows
            s.destroy()
            copy, srt, host_rows = host_path(pa, pc, batch, cols, names, sort_keys,
                                             layout["seg_offsets"], fetch)
            if it < warmup:
                continue
            for k, v in zip(groups, kms):
                ms[k].append(v)
            for k, v in (("kernels", sum(kms)), ("gpu_wall", wall), ("d2h_copy", copy),
                         ("pyarrow_sort", srt), ("host_total", copy + srt)):
                ms[k].append(v)
    finally:
        batch.free()
    assert out_rows == host_rows, (out_rows, host_rows)
    doc = {"rows": n, "n_parts": layout["n_parts"], "fetch": fetch, "out_rows": out_rows,
           "info": info, "ms": {k: stats(v) for k, v in ms.items()}}
    run = info["passes_run"]
    if run:
        per_pass = doc["ms"]["passes"]["median"] / run
        tbps = PASS_BYTES_PER_ROW * n / per_pass / 1e9
        doc["ms_per_pass"] = round(per_pass, 4)
        doc["pass_TBps"] = round(tbps, 3)
        doc["pass_fraction_of_stream_ceiling"] = round(tbps / STREAM_CEILING_TBPS, 3)
    doc["host_total_over_gpu_wall"] = round(
        doc["ms"]["host_total"]["median"] / doc["ms"]["gpu_wall"]["median"], 2)
    print(f"# {name}: done", file=sys.stderr, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-a", type=int, default=6_000_000)
    ap.add_argument("--rows-b", type=int, default=30_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_sort needs a GPU (no CPU fallback by design)")
    import pyarrow as pa
    import pyarrow.compute as pc

    rng = np.random.default_rng(42)
    doc = {"warmup": a.warmup, "reps": a.reps, "stream_ceiling_TBps": STREAM_CEILING_TBPS,
           "pass_bytes_per_row": PASS_BYTES_PER_ROW}

    n, P = a.rows_a, 128
    rev = rng.integers(90_000, 10_494_951_00, n, dtype=np.int64)  # revenue, scale 2
    words = np.empty((n, 2), dtype=np.uint64)
    words[:, 0] = rev.view(np.uint64)
    words[:, 1] = (rev >> 63).view(np.uint64)
    cols = [{"dtype": "dec128", "data": words, "valid": None},
            {"dtype": "i32", "data": rng.integers(8000, 10500, n).astype(np.int32),
             "valid": None},
            {"dtype": "i64", "data": rng.integers(1, 1 << 40, n, dtype=np.int64), "valid": None},
            {"dtype": "i32", "data": rng.integers(0, 2, n).astype(np.int32), "valid": None}]
    off = np.concatenate([[0], np.cumsum(rng.multinomial(n, np.full(P, 1.0 / P)))])
    layout = {"seg_offsets": off.astype(np.int64), "seg_part": np.arange(P, dtype=np.int32),
              "n_parts": P}
    names = ["revenue", "o_orderdate", "l_orderkey", "o_shippriority"]
    keys = [(0, True, True), (1, False, False)]
    sort_keys = [("revenue", "descending"), ("o_orderdate", "ascending")]
    for fetch in (10, None):
        doc["a_fetch10" if fetch else "a_all"] = measure(
            pa, pc, f"a fetch={fetch}", cols, names, keys, sort_keys, layout, fetch,
            a.warmup, a.reps)
    del cols, words, rev

    n = a.rows_b
    cols = [{"dtype": "i64", "valid": None,
             "data": rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)},
            {"dtype": "i32", "data": np.arange(n, dtype=np.int32), "valid": None}]
    layout = {"seg_offsets": np.array([0, n], dtype=np.int64),
              "seg_part": np.zeros(1, dtype=np.int32), "n_parts": 1}
    doc["b"] = measure(pa, pc, "b", cols, ["k", "payload"], [(0, False, False)],
                       [("k", "ascending")], layout, None, a.warmup, a.reps)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
