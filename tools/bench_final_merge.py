#!/usr/bin/env python3
"""bench_final_merge.py — measure the final aggregation above the shuffle
on the partials of the two shapes of §17.7:

  (a) q1: --rows rows, u8 + bool keys, 6 groups, the six-state plan -> a few thousand
      partial rows
  (b) the same decimal columns under one i32 key of 100 000 groups -> almost as many
      partial rows as rows: all the real grouping falls to the final aggregate

The partials come from api.partial_reduce in this process and are laid out as the columns
the shuffle carries (finalagg.partial_state_cols): keys, five dec128 sums each with its i64
nn, one i64 count; one partition. Per shape, alternately, --reps runs after --warmup:

  gpu      api.final_merge over the device batch: per-kernel hipEvent ms (claim, scan,
           merge), and the wall time of the whole call, result fetch included
  host     the path a user had before: copy the same columns device-to-host, then pyarrow
           group_by over them; the copy and the group-by are timed separately

Medians with min-max; input GB/s over the kernel time. Prints one JSON document; --out also
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

from datafusion_distributed_amd import api, finalagg  # noqa: E402

OPS = ["sum_dec128"] * 5 + ["count"]


def money(rng, n, lo, hi):
    v = rng.integers(lo, hi, n, dtype=np.int64)
    words = np.empty((n, 2), dtype=np.uint64)
    words[:, 0] = v.view(np.uint64)
    words[:, 1] = (v >> 63).view(np.uint64)
    return words


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def partials(cols, key_idx, first_dec):
    batch = api.DeviceBatch(cols)
    try:
        return api.partial_reduce(batch, key_idx, [(first_dec + i, "sum_dec128")
                                                   for i in range(5)] + [(None, "count")])
    finally:
        batch.free()


def host_path(pa, batch, pcols, key_names):
    """Device-to-host copy of every column, then pyarrow group_by: (copy ms, group-by ms,
    groups)."""
    n = batch.n_rows
    t0 = time.perf_counter()
    host = []
    for i, c in enumerate(pcols):
        nbytes = n * api.ELEM_SIZE[c["dtype"]]
        host.append(api._d2h(batch.desc.cols[i].data, nbytes, api.FIXED_NP[c["dtype"]]))
    t1 = time.perf_counter()
    arrays, names, aggs = [], [], []
    for i, c in enumerate(pcols):
        name = key_names[i] if i < len(key_names) else f"c{i}"
        if c["dtype"] == "dec128":
            arrays.append(pa.Array.from_buffers(pa.decimal128(38, 2), n,
                                                [None, pa.py_buffer(host[i])]))
        else:
            arrays.append(pa.array(host[i]))
        names.append(name)
        if i >= len(key_names):
            aggs.append((name, "sum"))
    out = pa.table(arrays, names=names).group_by(key_names).aggregate(aggs)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out.num_rows


def measure(pa, name, res, key_dtypes, warmup, reps):
    pcols, pkeys, paggs = finalagg.partial_state_cols(res, key_dtypes, OPS)
    n = len(res["keynull"])
    bpr = sum(api.ELEM_SIZE[c["dtype"]] for c in pcols)
    batch = api.DeviceBatch(pcols)
    ms = {k: [] for k in ("claim", "scan", "merge", "kernels", "gpu_wall", "d2h_copy",
                          "pyarrow_group_by", "host_total")}
    groups = host_groups = 0
    try:
        for it in range(warmup + reps):
            t0 = time.perf_counter()
            out = api.final_merge(batch, pkeys, paggs)
            wall = (time.perf_counter() - t0) * 1e3
            groups = len(out["keynull"])
            copy, gb, host_groups = host_path(pa, batch, pcols, [f"k{i}" for i in pkeys])
            if it < warmup:
                continue
            c, s, m = out["kernel_ms"]
            for k, v in (("claim", c), ("scan", s), ("merge", m), ("kernels", c + s + m),
                         ("gpu_wall", wall), ("d2h_copy", copy), ("pyarrow_group_by", gb),
                         ("host_total", copy + gb)):
                ms[k].append(v)
    finally:
        batch.free()
    assert groups == host_groups, (groups, host_groups)
    doc = {"partial_rows": n, "groups": groups, "input_bytes_per_row": bpr,
           "table_slots": finalagg.table_slots(n), "ms": {k: stats(v) for k, v in ms.items()}}
    doc["input_GBps_over_kernels"] = round(bpr * n / doc["ms"]["kernels"]["median"] / 1e6, 1)
    doc["host_total_over_gpu_wall"] = round(
        doc["ms"]["host_total"]["median"] / doc["ms"]["gpu_wall"]["median"], 2)
    doc["host_total_over_kernels"] = round(
        doc["ms"]["host_total"]["median"] / doc["ms"]["kernels"]["median"], 2)
    print(f"# {name}: done", file=sys.stderr, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_final_merge needs a GPU (no CPU fallback by design)")
    import pyarrow as pa

    n = a.rows
    rng = np.random.default_rng(42)
    rf = rng.integers(0, 3, n).astype(np.uint8)
    ls = rng.integers(0, 2, n).astype(np.uint8)
    k100k = rng.integers(0, 100_000, n).astype(np.int32)
    ranges = [(100, 5001), (90_000, 10_494_951), (80_000_00, 10_494_951_00),
              (80_000_0000, 11_400_000_0000), (0, 11)]  # qty, price, disc_price, charge, disc
    decs = [{"dtype": "dec128", "data": money(rng, n, lo, hi), "valid": None}
            for lo, hi in ranges]
    res_a = partials([{"dtype": "u8", "data": rf, "valid": None},
                      {"dtype": "bool", "data": ls, "valid": None}] + decs, [0, 1], 2)
    res_b = partials([{"dtype": "i32", "data": k100k, "valid": None}] + decs, [0], 1)
    del decs
    doc = {"rows": n, "warmup": a.warmup, "reps": a.reps, "layout": "one segment, one partition",
           "a": measure(pa, "a", res_a, ["u8", "bool"], a.warmup, a.reps),
           "b": measure(pa, "b", res_b, ["i32"], a.warmup, a.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
