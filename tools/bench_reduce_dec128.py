#!/usr/bin/env python3
"""bench_reduce_dec128.py — measure the wide partial-reduce kernel on the
q1 partial aggregate over native decimals:

  (a) q1 shape: --rows rows, u8 + bool keys, 6 groups, the six-state plan (five
      sum_dec128 + count), 82 B/row of input
  (b) the same decimal columns under one i32 key of 100 000 groups, 84 B/row

Both settings of DD_REDUCE_WAVEAGG are run on both shapes, and on (a) also the
predecessor: what a user could run before, the same six states over f64 casts as two
k_partial_reduce launches (4 + 2 aggregates, 2 x 2 + 40 = 44 B/row read). All forms live in
one process and are run alternately; medians, minima and maxima of dd_reducer_kernel_ms
over --reps runs after --warmup are reported with input GB/s. The document also states the
default DD_REDUCE_WAVEAGG that follows from the rule of §17.7: on only if it is faster on
(a) by more than the larger min-max spread of the two forms there, and on (b) not slower
by more than that shape's spread.
Prints one JSON document; --out also writes it to a file. Needs a GPU (no fallback).
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from datafusion_distributed_amd import api  # noqa: E402


def money(rng, n, lo, hi):
    """Sign-extended 128-bit values of an i64 range (TPC-H decimals at scale 2 .. 6)."""
    v = rng.integers(lo, hi, n, dtype=np.int64)
    words = np.empty((n, 2), dtype=np.uint64)
    words[:, 0] = v.view(np.uint64)
    words[:, 1] = (v >> 63).view(np.uint64)
    return v, words


def run_plan(batch, key_idx, aggs, waveagg=None):
    """One dd_partial_reduce_run without fetching the partials:
    (kernel_ms, output rows, kernel, waveagg)."""
    if waveagg is None:
        os.environ.pop("DD_REDUCE_WAVEAGG", None)
    else:
        os.environ["DD_REDUCE_WAVEAGG"] = str(waveagg)
    L = api.lib()
    nk, na = len(key_idx), len(aggs)
    keysc = (ctypes.c_int32 * nk)(*key_idx)
    aggc = (ctypes.c_int32 * na)(*[c if c is not None else 0 for c, _ in aggs])
    opsc = (ctypes.c_int32 * na)(*[api.AGG_OPS[o] for _, o in aggs])
    h = ctypes.c_void_p()
    api._check(L.dd_partial_reduce_run(ctypes.byref(batch.desc), keysc, nk, aggc, opsc, na,
                                       None, ctypes.byref(h)))
    try:
        return (float(L.dd_reducer_kernel_ms(h)), int(L.dd_reducer_n_rows(h)),
                int(L.dd_reducer_kernel(h)), int(L.dd_reducer_waveagg(h)))
    finally:
        L.dd_reducer_destroy(h)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_reduce_dec128 needs a GPU (no CPU fallback by design)")

    n = a.rows
    rng = np.random.default_rng(42)
    rf = rng.integers(0, 3, n).astype(np.uint8)
    ls = rng.integers(0, 2, n).astype(np.uint8)
    k100k = rng.integers(0, 100_000, n).astype(np.int32)
    ranges = [(100, 5001), (90_000, 10_494_951), (80_000_00, 10_494_951_00),
              (80_000_0000, 11_400_000_0000), (0, 11)]  # qty, price, disc_price, charge, disc
    ints, decs = zip(*[money(rng, n, lo, hi) for lo, hi in ranges])

    def dcol(w):
        return {"dtype": "dec128", "data": w, "valid": None}

    batch_a = api.DeviceBatch([{"dtype": "u8", "data": rf, "valid": None},
                               {"dtype": "bool", "data": ls, "valid": None}]
                              + [dcol(w) for w in decs])
    batch_b = api.DeviceBatch([{"dtype": "i32", "data": k100k, "valid": None}]
                              + [dcol(w) for w in decs])
    batch_f = api.DeviceBatch([{"dtype": "u8", "data": rf, "valid": None},
                               {"dtype": "bool", "data": ls, "valid": None}]
                              + [{"dtype": "f64", "data": v.astype(np.float64), "valid": None}
                                 for v in ints])
    plan_a = [(2 + i, "sum_dec128") for i in range(5)] + [(None, "count")]
    plan_b = [(1 + i, "sum_dec128") for i in range(5)] + [(None, "count")]
    pred_1 = [(2 + i, "sum_f64") for i in range(4)]
    pred_2 = [(6, "sum_f64"), (None, "count")]

    ms = {"a_waveagg0": [], "a_waveagg1": [], "a_predecessor": [], "b_waveagg0": [],
          "b_waveagg1": []}
    rows = {}
    for it in range(a.warmup + a.reps):
        for wa in (0, 1):  # forms alternated run by run
            t, r, kern, got = run_plan(batch_a, [0, 1], plan_a, wa)
            assert kern == 1 and got == wa
            rows[f"a_waveagg{wa}"] = r
            if it >= a.warmup:
                ms[f"a_waveagg{wa}"].append(t)
        t1, r1, kern1, _ = run_plan(batch_f, [0, 1], pred_1)
        t2, r2, kern2, _ = run_plan(batch_f, [0, 1], pred_2)
        assert kern1 == 0 and kern2 == 0
        rows["a_predecessor"] = r1 + r2
        if it >= a.warmup:
            ms["a_predecessor"].append(t1 + t2)
        for wa in (0, 1):
            t, r, kern, got = run_plan(batch_b, [0], plan_b, wa)
            assert kern == 1 and got == wa
            rows[f"b_waveagg{wa}"] = r
            if it >= a.warmup:
                ms[f"b_waveagg{wa}"].append(t)
    _, _, _, default = run_plan(batch_a, [0, 1], plan_a, None)

    bpr = {"a_waveagg0": 82, "a_waveagg1": 82, "a_predecessor": 44, "b_waveagg0": 84,
           "b_waveagg1": 84}
    res = {"rows": n, "warmup": a.warmup, "reps": a.reps,
           "geometry_a": api.partial_reduce_plan_geometry(n, 2, [o for _, o in plan_a]),
           "geometry_b": api.partial_reduce_plan_geometry(n, 1, [o for _, o in plan_b]),
           "forms": {}}
    for name, xs in ms.items():
        s = stats(xs)
        res["forms"][name] = {"kernel_ms": s, "input_bytes_per_row": bpr[name],
                              "input_GBps": round(bpr[name] * n / s["median"] / 1e6, 1),
                              "partial_rows": rows[name]}
    f = res["forms"]
    spread_a = max(f["a_waveagg0"]["kernel_ms"]["spread"], f["a_waveagg1"]["kernel_ms"]["spread"])
    spread_b = max(f["b_waveagg0"]["kernel_ms"]["spread"], f["b_waveagg1"]["kernel_ms"]["spread"])
    gain_a = f["a_waveagg0"]["kernel_ms"]["median"] - f["a_waveagg1"]["kernel_ms"]["median"]
    loss_b = f["b_waveagg1"]["kernel_ms"]["median"] - f["b_waveagg0"]["kernel_ms"]["median"]
    res["waveagg_rule"] = {
        "a_gain_ms": round(gain_a, 4), "a_spread_ms": round(spread_a, 4),
        "b_loss_ms": round(loss_b, 4), "b_spread_ms": round(spread_b, 4),
        "default_by_rule": int(gain_a > spread_a and loss_b <= spread_b),
        "default_in_build": default}
    best = f[f"a_waveagg{default}"]
    res["vs_predecessor"] = {
        "wide_input_GBps": best["input_GBps"],
        "predecessor_input_GBps": f["a_predecessor"]["input_GBps"],
        "bandwidth_ratio": round(best["input_GBps"] / f["a_predecessor"]["input_GBps"], 3),
        "time_ratio": round(best["kernel_ms"]["median"]
                            / f["a_predecessor"]["kernel_ms"]["median"], 3)}
    for b in (batch_a, batch_b, batch_f):
        b.free()
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
