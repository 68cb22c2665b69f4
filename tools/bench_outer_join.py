"""bench_outer_join.py — the outer joins (left, right, full) on the device against the path a
user had before them: copy every column of both shuffled sides to the host and run one
pyarrow.Table.join over the whole tables (pyarrow's best case: no partition loop).
DESIGN.md §20 records the results.

Shapes (both sides go through api.Partitioner and are joined via partitioned_batch):
  a      §19.4's (a): 1.5 M unique i64 build keys + two i32 payloads; 6 M probe rows (i64 key
         + two f64), about half of them matching; P = 16
  b      §19.4's (b): the same at 15 M x 60 M, P = 128
  q13    q13-like: 1.5 M unique build keys (customers), 15 M probe rows (orders: key + one
         i64) that reach two thirds of the build keys; P = 16; projection = build key, probe
         payload, as q13's
  a_all  shape a with every probe key drawn from the build keys. Under "right" every probe
         row matches, so the output IS the inner join's, and api.hash_join(..., "inner")
         runs alternately in the same process: what storing head[] costs in count and buys
         in emit, measured, not asserted.

A case is shape:type. Per case the paths alternate in one process; medians of --runs after
--warmup with min and max. Needs a GPU; prints one JSON line per case and, with --out,
writes the document to a file."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datafusion_distributed_amd import api  # noqa: E402

PA_TYPE = {"left": "left outer", "right": "right outer", "full": "full outer"}
NAMES = ("build", "count", "scan", "emit", "gather")


def shape(name, rng):
    if name == "q13":
        nb, npr, P = 1_500_000, 15_000_000, 16
        bkey = rng.permutation(nb).astype(np.int64)
        pkey = rng.integers(0, nb * 2 // 3, npr, dtype=np.int64)  # a third has no order
        build = [{"dtype": "i64", "data": bkey, "valid": None}]
        probe = [{"dtype": "i64", "data": pkey, "valid": None},
                 {"dtype": "i64", "data": np.arange(npr, dtype=np.int64), "valid": None}]
        return build, probe, P, [0], [1]
    nb, npr, P = (15_000_000, 60_000_000, 128) if name == "b" else (1_500_000, 6_000_000, 16)
    bkey = rng.permutation(nb).astype(np.int64) * 2
    pkey = rng.integers(0, 2 * nb, npr, dtype=np.int64)  # even values match
    if name == "a_all":
        pkey &= ~np.int64(1)
    build = [{"dtype": "i64", "data": bkey, "valid": None},
             {"dtype": "i32", "data": rng.integers(0, 1 << 30, nb).astype(np.int32), "valid": None},
             {"dtype": "i32", "data": rng.integers(0, 1 << 30, nb).astype(np.int32), "valid": None}]
    probe = [{"dtype": "i64", "data": pkey, "valid": None},
             {"dtype": "f64", "data": rng.random(npr), "valid": None},
             {"dtype": "f64", "data": rng.random(npr), "valid": None}]
    return build, probe, P, None, None


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def kernel_stats(samples):
    out = {nm: stats([ms[i] for _, ms in samples]) for i, nm in enumerate(NAMES)}
    out["total"] = stats([sum(ms) for _, ms in samples])
    out["count_plus_emit"] = stats([ms[1] + ms[3] for _, ms in samples])
    return out


def run_case(name, join_type, runs, warmup, host_runs):
    import pyarrow as pa

    rng = np.random.default_rng(11)
    build, probe, P, bproj, pproj = shape(name, rng)
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    bp, pp = api.Partitioner(bb, [0], P), api.Partitioner(pb, [0], P)
    for part in (bp, pp):
        part.run()
        part.sync()
    bview, blay = api.partitioned_batch(bp)
    pview, play = api.partitioned_batch(pp)
    with_inner = name == "a_all" and join_type == "right"

    def device(fn, jt):
        t0 = time.perf_counter()
        j = fn(bview, [0], pview, [0], jt, blay, play, bproj, pproj)  # synchronous
        wall = (time.perf_counter() - t0) * 1e3
        ms, n = j.kernel_ms(), j.n_rows
        j.destroy()
        return wall, ms, n

    def host():
        t0 = time.perf_counter()
        tb = pa.table({f"b{i}": bp.col_out(i)["data"] for i in range(len(build))})
        tp = pa.table({f"p{i}": pp.col_out(i)["data"] for i in range(len(probe))})
        t1 = time.perf_counter()
        j = tb.join(tp, keys="b0", right_keys="p0", join_type=PA_TYPE[join_type])
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, j.num_rows

    dev, inner, hst, n_out = [], [], [], None
    for it in range(warmup + runs):
        wall, ms, n = device(api.outer_join, join_type)
        timed = it >= warmup
        if timed:
            dev.append((wall, ms))
        if with_inner:
            iwall, ims, inn = device(api.hash_join, "inner")
            assert inn == n, f"inner join gives {inn} rows, right join {n}"
            if timed:
                inner.append((iwall, ims))
        if it == 0 or (timed and len(hst) < host_runs):  # one warm-up of the host path
            copy_ms, join_ms, hn = host()
            assert hn == n, f"host join gives {hn} rows, device {n}"
            if timed:
                hst.append((copy_ms, join_ms))
        n_out = n
    for h in (bp, pp):
        h.destroy()
    bb.free()
    pb.free()

    wall = stats([w for w, _ in dev])
    host_total = stats([c + j for c, j in hst])
    res = {
        "shape": name, "join_type": join_type, "build_rows": len(build[0]["data"]),
        "probe_rows": len(probe[0]["data"]), "n_parts": P, "out_rows": int(n_out),
        "runs": runs, "warmup": warmup, "host_runs": len(hst),
        "kernel_ms": kernel_stats(dev), "wall_ms": wall,
        "host_copy_ms": stats([c for c, _ in hst]), "host_join_ms": stats([j for _, j in hst]),
        "host_total_ms": host_total, "host_over_wall": host_total["median"] / wall["median"],
    }
    if with_inner:
        res["inner_kernel_ms"] = kernel_stats(inner)
        res["inner_wall_ms"] = stats([w for w, _ in inner])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", default="a:right,a:left,a:full,a_all:right,q13:left",
                    help="comma list of shape:type; shapes a, b, q13, a_all")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=None,
                    help="timed runs of the host path (default: --runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_outer_join needs a GPU: there is no CPU fallback")
    host_runs = args.runs if args.host_runs is None else args.host_runs
    doc = {"tool": "tools/bench_outer_join.py", "results": []}
    for case in args.cases.split(","):
        name, join_type = case.strip().split(":")
        res = run_case(name, join_type, args.runs, args.warmup, host_runs)
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
        if args.out:  # after every case: a later case that fails loses nothing
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
