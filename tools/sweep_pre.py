"""Interleaved one-box A/B of the K1 / K3 variants on a bench shape.

Sequential per-config blocks measured ±4-5% within-box drift (clock/thermal), swamping
the ~3-6% deltas under test. This sweep creates every config's partitioner up-front
(env knobs are read at create time; outputs stay resident — 288 GB HBM), then runs the
configs ROUND-ROBIN and reports per-kernel MEDIANS, so drift hits all configs equally.
Usage: python tools/sweep_pre.py [rows] [reps] [workload] [configs] [partitions]
  workload: a bench.py workload name (default tpch_sf10_lineitem_shuffle; the multikey and
            q1 shapes are tpch_sf10_multikey_shuffle / tpch_sf1_q1_repartition);
            rows = 0 takes the workload's own row count
  configs:  comma-separated subset of the CONFIGS names (default: all)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np

import bench
from datafusion_distributed_amd import api

WORKLOAD = sys.argv[3] if len(sys.argv) > 3 else "tpch_sf10_lineitem_shuffle"
N = int(sys.argv[1]) if len(sys.argv) > 1 and int(sys.argv[1]) > 0 \
    else bench.WORKLOADS[WORKLOAD][1]
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 21
P = int(sys.argv[5]) if len(sys.argv) > 5 else bench.PARTS_PER_RANK

CONFIGS = [
    ("seg", {"DD_PRE_LAYOUT": "seg", "DD_PRE_XCD": "0"}),
    ("round", {"DD_PRE_LAYOUT": "round", "DD_PRE_XCD": "0"}),
    ("round+xcd", {"DD_PRE_LAYOUT": "round", "DD_PRE_XCD": "1"}),
    ("hl", {"DD_K3_PRE": "0"}),
    ("seg+xcd", {"DD_PRE_LAYOUT": "seg", "DD_PRE_XCD": "1"}),
    ("pre-rpb1", {"DD_PRE_RPB": "1"}),
    ("pre-rpb4", {"DD_PRE_RPB": "4"}),
    ("plain", {"DD_K3_PRE": "0", "DD_K3_HL": "0"}),
    ("spec", {}),                       # the default: K1 with its compile-time key signature
    ("generic", {"DD_K1_SPEC": "0"}),   # K1 with the run-time key loop
    ("narrow", {"DD_PRE_WIDE": "0"}),   # 4096-row rounds
    ("wide", {"DD_PRE_WIDE": "1"}),     # 8192-row rounds in two column passes
    ("wide-rpb1", {"DD_PRE_WIDE": "1", "DD_PRE_RPB": "1"}),
    ("wide-rpb2", {"DD_PRE_WIDE": "1", "DD_PRE_RPB": "2"}),
    ("wide-rpb1-xcd0", {"DD_PRE_WIDE": "1", "DD_PRE_RPB": "1", "DD_PRE_XCD": "0"}),
    ("wide-rpb1-xcd1", {"DD_PRE_WIDE": "1", "DD_PRE_RPB": "1", "DD_PRE_XCD": "1"}),
    ("wide-rpb4", {"DD_PRE_WIDE": "1", "DD_PRE_RPB": "4"}),
    ("wide-xcd0", {"DD_PRE_WIDE": "1", "DD_PRE_XCD": "0"}),
    ("wide-xcd1", {"DD_PRE_WIDE": "1", "DD_PRE_XCD": "1"}),
]
if len(sys.argv) > 4:
    CONFIGS = [c for c in CONFIGS if c[0] in sys.argv[4].split(",")]

KNOBS = ["DD_K3_PRE", "DD_K3_HL", "DD_PID8", "DD_PRE_NT", "DD_PRE_RPB", "DD_PRE_GMAX",
         "DD_PRE_WPB", "DD_PRE_LAYOUT", "DD_PRE_XCD", "DD_K1_SPEC", "DD_PRE_WIDE",
         "DD_PRE_WIDE_MIN_ROWS"]


def main():
    cols, key_idx = bench.WORKLOADS[WORKLOAD][0](N, 42)
    batch = api.DeviceBatch(cols)
    row_bytes = float(sum(bench.FIXED_SIZE[c["dtype"]] for c in cols))
    parts = []
    for name, env in CONFIGS:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        part = api.Partitioner(batch, key_idx, P)
        parts.append((name, part))
        print(name, "plan", json.dumps({**part.info(), "pre_layout": part.pre_layout(),
                                        "k1_spec": part.k1_spec(),
                                        "pre_wide": part.pre_wide()}),
              flush=True)
    samples = {name: [] for name, _ in CONFIGS}
    for r in range(REPS + 2):
        # forward and backward passes alternate, so no config always runs behind the same
        # neighbour's cache state
        for name, part in (parts if r % 2 == 0 else parts[::-1]):
            part.run()
            part.sync()
            if r >= 2:
                samples[name].append(part.kernel_ms())
    results = {}
    for name, part in parts:
        ks = np.median(np.array(samples[name]), axis=0)
        # the step is the median of per-run sums, not the sum of per-kernel medians
        step_ms = float(np.median(np.array(samples[name]).sum(axis=1)))
        results[name] = {"k1": round(float(ks[0]), 4), "k2": round(float(ks[1]), 4),
                         "k3": round(float(ks[2]), 4), "step_ms": round(step_ms, 4),
                         "GBps": round(N * row_bytes / step_ms / 1e6, 1)}
        print(name, json.dumps(results[name]), flush=True)
        part.destroy()
    batch.free()
    print("SWEEP", json.dumps({"workload": WORKLOAD, "rows": N, "P": P, "reps": REPS,
                               "results": results}))


if __name__ == "__main__":
    main()
