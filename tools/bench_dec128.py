#!/usr/bin/env python3
"""bench_dec128.py — measure the shuffle of a TPC-H lineitem projection with native
Decimal128 columns against the split form a user could already run:

  dec128  [l_orderkey i64 (key), l_quantity, l_extendedprice, l_discount dec128,
           l_shipdate i32]                                  5 columns, 60 B/row
  split   the same bytes with every decimal de-interleaved on the host into its two i64
          halves: i64 key + six i64 + i32                   8 columns, 60 B/row

Both partitioners live in one process on one build and are run alternately; the medians,
minima and maxima of kernel_ms() (K1 hash+count, K2 scans, K3 scatter) over --reps runs
after --warmup are reported with each one's plan (Partitioner.info()). The acceptance
figure is k3_ratio = K3(dec128) / K3(split), bound 1.15 (the measured cost of the generic
column loop against the compile-time-column-count form the split batch gets).
Prints one JSON document; --out also writes it to a file. Needs a GPU (no fallback).
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from datafusion_distributed_amd import api  # noqa: E402


def make_lineitem(n, seed):
    """(dec128 form, split form) of the same rows. Decimals are sign-extended 128-bit
    values of TPC-H's ranges at scale 2: quantity 1..50, price up to 104 949.50, discount
    0..0.10, one row in sixteen negated so that the high halves are not all zero."""
    rng = np.random.default_rng(seed)
    key = rng.integers(1, 4 * max(n, 1), n, dtype=np.int64)
    ship = rng.integers(8036, 10562, n, dtype=np.int64).astype(np.int32)

    def decimal(lo, hi):
        v = rng.integers(lo, hi, n, dtype=np.int64)
        v = np.where(rng.integers(0, 16, n) == 0, -v, v)
        words = np.empty((n, 2), dtype=np.uint64)
        words[:, 0] = v.view(np.uint64)
        words[:, 1] = (v >> 63).view(np.uint64)  # sign extension
        return words

    decs = [decimal(100, 5001), decimal(90_000, 10_494_951), decimal(0, 11)]
    native = [{"dtype": "i64", "data": key, "valid": None}]
    split = [{"dtype": "i64", "data": key, "valid": None}]
    for w in decs:
        native.append({"dtype": "dec128", "data": w, "valid": None, "precision": 15,
                       "scale": 2})
        for h in range(2):
            split.append({"dtype": "i64", "valid": None,
                          "data": np.ascontiguousarray(w[:, h]).view(np.int64)})
    native.append({"dtype": "i32", "data": ship, "valid": None})
    split.append({"dtype": "i32", "data": ship, "valid": None})
    return native, split


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--parts", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_dec128 needs a GPU (no CPU fallback by design)")

    native, split = make_lineitem(a.rows, 42)
    forms = {}
    for name, cols in (("dec128", native), ("split", split)):
        batch = api.DeviceBatch(cols)
        part = api.Partitioner(batch, [0], a.parts)
        forms[name] = {"batch": batch, "part": part, "ms": [], "info": part.info(),
                       "k1_spec": part.k1_spec(), "n_cols": len(cols)}
    for it in range(a.warmup + a.reps):
        for name in ("dec128", "split"):  # alternated run by run
            part = forms[name]["part"]
            part.run()
            part.sync()
            if it >= a.warmup:
                forms[name]["ms"].append(part.kernel_ms())

    # the two forms must have routed the rows alike (same key, same hash)
    same = bool((forms["dec128"]["part"].row_offsets() ==
                 forms["split"]["part"].row_offsets()).all())
    res = {"rows": a.rows, "parts": a.parts, "bytes_per_row": 60, "warmup": a.warmup,
           "reps": a.reps, "row_offsets_equal": same, "forms": {}}
    for name, f in forms.items():
        ms = f["ms"]
        k = {k: stats([r[i] for r in ms]) for i, k in enumerate(("k1", "k2", "k3"))}
        total = statistics.median([sum(r) for r in ms])
        res["forms"][name] = {
            "n_cols": f["n_cols"], "info": f["info"], "k1_spec": f["k1_spec"],
            "kernel_ms": k, "total_ms_median": round(total, 4),
            # read 60 B/row in K3 + 8 B key in K1 + pid write/read, write 60 B/row
            "GBps_payload": round(2 * 60 * a.rows / total / 1e6, 1)}
        f["part"].destroy()
        f["batch"].free()
    d, s = res["forms"]["dec128"]["kernel_ms"], res["forms"]["split"]["kernel_ms"]
    res["k3_ratio"] = round(d["k3"]["median"] / s["k3"]["median"], 4)
    res["k3_bound"] = 1.15
    res["k3_within_bound"] = res["k3_ratio"] <= 1.15
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
