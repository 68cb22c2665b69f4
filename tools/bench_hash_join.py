"""bench_hash_join.py — the partitioned hash join on the device against the path a user had
before it: copy both shuffled sides to the host and run one pyarrow.Table.join over the
whole tables (pyarrow's best case: no partition loop). DESIGN.md §19 records the results.

Shapes (both sides go through api.Partitioner and are joined via partitioned_batch):
  a  PK/FK small: 1.5 M unique i64 build keys + two i32 payloads; 6 M probe rows (i64 key +
     two f64), about half of them matching; P = 16
  b  the same at 15 M x 60 M, P = 128 (the SF10 scale of the headline)
  c  duplicate-heavy: 1 M build rows over 10 000 keys, 100 000 probe rows, ~10 M output rows

Per shape the two paths alternate in one process; medians of --runs after --warmup with
min and max. Needs a GPU; prints one JSON document and, with --out, writes it to a file."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datafusion_distributed_amd import api  # noqa: E402

COPY_CEILING_TBS = 5.79  # the device copy ceiling


def shape(name, rng):
    if name in ("a", "b"):
        nb, npr, P = (1_500_000, 6_000_000, 16) if name == "a" else (15_000_000, 60_000_000, 128)
        bkey = rng.permutation(nb).astype(np.int64) * 2
        pkey = rng.integers(0, 2 * nb, npr, dtype=np.int64)  # even values match
    else:
        nb, npr, P = 1_000_000, 100_000, 16
        bkey = rng.integers(0, 10_000, nb, dtype=np.int64)
        pkey = rng.integers(0, 10_000, npr, dtype=np.int64)
    build = [{"dtype": "i64", "data": bkey, "valid": None},
             {"dtype": "i32", "data": rng.integers(0, 1 << 30, nb).astype(np.int32), "valid": None},
             {"dtype": "i32", "data": rng.integers(0, 1 << 30, nb).astype(np.int32), "valid": None}]
    probe = [{"dtype": "i64", "data": pkey, "valid": None},
             {"dtype": "f64", "data": rng.random(npr), "valid": None},
             {"dtype": "f64", "data": rng.random(npr), "valid": None}]
    return build, probe, P


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def run_shape(name, runs, warmup, host_runs):
    import pyarrow as pa

    rng = np.random.default_rng(11)
    build, probe, P = shape(name, rng)
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    bp, pp = api.Partitioner(bb, [0], P), api.Partitioner(pb, [0], P)
    for part in (bp, pp):
        part.run()
        part.sync()
    bview, blay = api.partitioned_batch(bp)
    pview, play = api.partitioned_batch(pp)

    def device():
        t0 = time.perf_counter()
        j = api.hash_join(bview, [0], pview, [0], "inner", blay, play)  # synchronous
        wall = (time.perf_counter() - t0) * 1e3
        ms, n = j.kernel_ms(), j.n_rows
        j.destroy()
        return wall, ms, n

    def host():
        t0 = time.perf_counter()
        tb = pa.table({f"b{i}": bp.col_out(i)["data"] for i in range(3)})
        tp = pa.table({f"p{i}": pp.col_out(i)["data"] for i in range(3)})
        t1 = time.perf_counter()
        j = tb.join(tp, keys="b0", right_keys="p0", join_type="inner")
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, j.num_rows

    dev, hst, n_out = [], [], None
    for it in range(warmup + runs):
        wall, ms, n = device()
        timed = it >= warmup
        if timed:
            dev.append((wall, ms))
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

    names = ("build", "count", "scan", "emit", "gather")
    kernel = {nm: stats([ms[i] for _, ms in dev]) for i, nm in enumerate(names)}
    kernel_total = stats([sum(ms) for _, ms in dev])
    wall = stats([w for w, _ in dev])
    host_copy = stats([c for c, _ in hst])
    host_join = stats([j for _, j in hst])
    host_total = stats([c + j for c, j in hst])
    # bytes the gather moves: per output row and side one u32 index read, and per column
    # one read and one write of its width (i64 + 2 x i32 build side, i64 + 2 x f64 probe)
    g_build, g_probe = n_out * (4 + 2 * 16), n_out * (4 + 2 * 24)
    g_tbs = (g_build + g_probe) / (kernel["gather"]["median"] * 1e-3) / 1e12 if n_out else 0.0
    return {
        "shape": name, "build_rows": len(build[0]["data"]), "probe_rows": len(probe[0]["data"]),
        "n_parts": P, "out_rows": int(n_out), "runs": runs, "warmup": warmup,
        "host_runs": len(hst),
        "kernel_ms": kernel, "kernel_total_ms": kernel_total, "wall_ms": wall,
        "host_copy_ms": host_copy, "host_join_ms": host_join, "host_total_ms": host_total,
        "gather_bytes": {"build_side_random": g_build, "probe_side_monotone": g_probe},
        "gather_TBps": g_tbs, "gather_share_of_copy_ceiling": g_tbs / COPY_CEILING_TBS,
        "host_over_wall": host_total["median"] / wall["median"],
        "host_over_kernel": host_total["median"] / kernel_total["median"],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="a,c", help="comma list out of a, b, c")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=None,
                    help="timed runs of the host path (default: --runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_hash_join needs a GPU: there is no CPU fallback")
    host_runs = args.runs if args.host_runs is None else args.host_runs
    doc = {"tool": "tools/bench_hash_join.py", "copy_ceiling_TBps": COPY_CEILING_TBS,
           "results": []}
    for name in args.shapes.split(","):
        res = run_shape(name.strip(), args.runs, args.warmup, host_runs)
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
