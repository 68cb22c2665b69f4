#!/usr/bin/env python3
"""bench_dictgc.py — measure the dictionary-GC kernels on the committed
dictkey_shuffle shape: 30 M rows, dict32 over 100k utf8 values, P=128.

For W in {1, 8, 128} and both tiers (DD_GC_LDS=1/0, alternated inside one process so both
see the same partitioner output) it reports, as medians over --reps runs after --warmup:
  - mark / rank / compact / remap ms (dd_dict_gc_kernel_ms, hipEvents)
  - achieved GB/s of the two row-rate kernels against their algorithmic bytes
    (mark: 4 B index [+1 B validity] per row; remap: the same + 4 B written) and the
    fraction of the project's measured streaming ceiling (5.79 TB/s, profiles/r02_patmax.txt)
  - total GC time over the same process's partitioner time (dd_partitioner_kernel_ms)
  - dictionary bytes shipped per window after GC against the full dictionary
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

import bench  # noqa: E402  (make_dictkey: the committed workload generator)
from datafusion_distributed_amd import api  # noqa: E402

STREAM_CEILING_GBPS = 5790.0  # profiles/r02_patmax.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--parts", type=int, default=128)
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 8, 128])
    ap.add_argument("--null-frac", type=float, default=0.0,
                    help="add a validity buffer to the dict column with this null fraction")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_dictgc needs a GPU (no CPU fallback by design)")

    cols, keys = bench.make_dictkey(a.rows, 42)
    if a.null_frac > 0:
        rng = np.random.default_rng(43)
        cols[0]["valid"] = (rng.random(a.rows) >= a.null_frac).astype(np.uint8)
    has_valid = cols[0].get("valid") is not None
    dict_n = len(cols[0]["dict_offsets"]) - 1
    full_dict_bytes = int(cols[0]["dict_offsets"][-1]) + 4 * (dict_n + 1)
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, keys, a.parts)
    pms = []
    for _ in range(a.warmup + 3):
        part.run()
        part.sync()
        pms.append(sum(part.kernel_ms()))
    part_ms = statistics.median(pms[a.warmup:])

    mark_bytes = a.rows * (4 + has_valid)
    remap_bytes = a.rows * (8 + has_valid)
    res = {"rows": a.rows, "parts": a.parts, "dict_n": dict_n, "has_validity": has_valid,
           "full_dict_bytes": full_dict_bytes, "partitioner_ms": round(part_ms, 4),
           "warmup": a.warmup, "reps": a.reps, "cases": []}
    for W in a.windows:
        runs = {"1": [], "0": []}
        shipped = None
        for it in range(a.warmup + a.reps):
            for tier in ("1", "0"):  # alternate the tiers run by run
                os.environ["DD_GC_LDS"] = tier
                g = api.DictGC(part, keys[0], W)
                if it >= a.warmup:
                    runs[tier].append(g.kernel_ms())
                if shipped is None:
                    v, b = g.counts()
                    shipped = (np.diff(b) + 4 * (np.diff(v) + 1)).astype(np.int64)
                g.destroy()
        for tier in ("1", "0"):
            med = [statistics.median(r[k] for r in runs[tier]) for k in range(4)]
            lo = [min(r[k] for r in runs[tier]) for k in range(4)]
            hi = [max(r[k] for r in runs[tier]) for k in range(4)]
            total = sum(med)
            mark_gbps = mark_bytes / med[0] / 1e6
            remap_gbps = remap_bytes / med[3] / 1e6
            res["cases"].append({
                "W": W, "tier": "lds" if tier == "1" else "global",
                "ms": dict(zip(("mark", "rank", "compact", "remap"),
                               (round(x, 4) for x in med))),
                "ms_min": [round(x, 4) for x in lo], "ms_max": [round(x, 4) for x in hi],
                "gc_total_ms": round(total, 4),
                "mark_GBps": round(mark_gbps, 1), "remap_GBps": round(remap_gbps, 1),
                "mark_frac_of_stream": round(mark_gbps / STREAM_CEILING_GBPS, 3),
                "remap_frac_of_stream": round(remap_gbps / STREAM_CEILING_GBPS, 3),
                "gc_over_partitioner": round(total / part_ms, 3),
                "dict_bytes_per_window_mean": int(shipped.mean()),
                "dict_bytes_per_window_max": int(shipped.max()),
                "dict_bytes_vs_full": round(float(shipped.mean()) / full_dict_bytes, 4),
            })
    os.environ.pop("DD_GC_LDS", None)
    part.destroy()
    batch.free()
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
