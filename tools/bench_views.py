#!/usr/bin/env python3
"""bench_views.py — measure view ingest and emit on the committed
clickbench_userid_shuffle shape (20 M rows, Zipf i64 key, 16..111 B URL column, P=128) with
the URL column presented as Arrow views:
  one_buffer   every value long, all in one data buffer (views in row order)
  four_buffers about 30 % of the values cut to <= 12 bytes (inline), the rest left in the
               byte buffer, which is cut into 4 data buffers by row quarter (the inline
               rows' bytes stay behind as garbage, which is what gc() exists to drop)
For each layout and both copy tiers (DD_VIEW_LDS=1 / 0, alternated run by run in one
process) it reports medians, minima and maxima over --reps runs after --warmup of
  - ingest len / scan / copy ms and emit scan / build / copy ms (hipEvents)
  - achieved GB/s against the algorithmic bytes (ingest: 16 B/row + value bytes read +
    value bytes written; emit: 4 B/row + bytes read + 16 B/row + long bytes written) and
    the fraction of the measured streaming ceiling (5.79 TB/s, profiles/r02_patmax.txt)
  - the partitioner's kernel time in the same process
  - what a user must do today instead: arr.cast(pa.string()) on the host plus the pageable
    upload of the cast's offsets and bytes, timed on the same box
Prints one JSON document; --out also writes it to a file. Needs a GPU (no fallback).
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (make_clickbench_userid: the committed workload generator)
from datafusion_distributed_amd import api  # noqa: E402

STREAM_CEILING_GBPS = 5790.0  # profiles/r02_patmax.txt


def make_views(off, data, inline_frac, n_bufs, seed):
    """(views u8[n,16], [data buffers]) over the utf8 column (off, data)."""
    n = len(off) - 1
    rng = np.random.default_rng(seed)
    lens = np.diff(off).astype(np.int32)
    if inline_frac > 0:
        short = rng.random(n) < inline_frac
        lens = np.where(short, rng.integers(0, 13, n).astype(np.int32), lens)
    start = off[:-1].astype(np.int64)
    views = np.zeros((n, 16), dtype=np.uint8)
    words = views.view(np.int32).reshape(n, 4)
    words[:, 0] = lens
    inline = lens <= 12
    for j in range(12):  # prefix (every row has >= 16 source bytes) and inline bytes
        m = (lens > j) & (inline | (j < 4))
        views[m, 4 + j] = data[start[m] + j]
    row_cut = [(n * q) // n_bufs for q in range(n_bufs + 1)]
    cut = [int(off[r]) for r in row_cut]
    bidx = np.searchsorted(np.asarray(row_cut[1:-1], dtype=np.int64),
                           np.arange(n, dtype=np.int64), side="right")
    lng = ~inline
    words[lng, 2] = bidx[lng].astype(np.int32)
    words[lng, 3] = (start[lng] - np.asarray(cut, dtype=np.int64)[bidx[lng]]).astype(np.int32)
    bufs = [data[cut[q]:cut[q + 1]] for q in range(n_bufs)]
    return views, bufs, lens


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def host_baseline(views, bufs, n, reps):
    """Today's path: cast the view array to utf8 on the host, upload offsets + bytes."""
    import pyarrow as pa

    arr = pa.Array.from_buffers(
        pa.string_view(), n,
        [None, pa.py_buffer(views.reshape(-1))] +
        [pa.py_buffer(np.ascontiguousarray(b)) for b in bufs])
    cast_ms, up_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s = arr.cast(pa.string())
        t1 = time.perf_counter()
        ob, db = s.buffers()[1], s.buffers()[2]
        o = np.frombuffer(ob, dtype=np.uint8)
        d = np.frombuffer(db, dtype=np.uint8) if db is not None else np.zeros(0, np.uint8)
        po, pd = api._dev_alloc(o.nbytes), api._dev_alloc(d.nbytes)
        api._check(api.lib().dd_device_sync())
        t2 = time.perf_counter()
        api._h2d(po, o)
        if d.nbytes:
            api._h2d(pd, d)
        api._check(api.lib().dd_device_sync())
        t3 = time.perf_counter()
        api.lib().dd_dev_free(po)
        api.lib().dd_dev_free(pd)
        cast_ms.append((t1 - t0) * 1e3)
        up_ms.append((t3 - t2) * 1e3)
        del s
    return {"cast_ms": stats(cast_ms), "upload_ms": stats(up_ms),
            "total_ms_median": round(statistics.median(cast_ms) +
                                     statistics.median(up_ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--parts", type=int, default=128)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if api.device_count() == 0:
        raise SystemExit("bench_views needs a GPU (no CPU fallback by design)")

    cols, keys = bench.make_clickbench_userid(a.rows, 42)
    off, data = cols[1]["offsets"], cols[1]["data"]
    n = a.rows
    res = {"rows": n, "parts": a.parts, "windows": a.windows, "warmup": a.warmup,
           "reps": a.reps, "tile_rows": api.view_tile_rows(),
           "image_bytes": api.view_image_bytes(),
           "stream_ceiling_GBps": STREAM_CEILING_GBPS, "layouts": []}
    for name, inline_frac, n_bufs in (("one_buffer", 0.0, 1), ("four_buffers", 0.3, 4)):
        views, bufs, lens = make_views(off, data, inline_frac, n_bufs, 7)
        value_bytes = int(lens.astype(np.int64).sum())
        long_bytes = int(lens[lens > 12].astype(np.int64).sum())
        ingest_bytes = 16 * n + 2 * value_bytes
        emit_bytes = 4 * n + value_bytes + 16 * n + long_bytes
        lay = {"layout": name, "n_bufs": n_bufs, "value_bytes": value_bytes,
               "long_bytes": long_bytes, "inline_rows": int((lens <= 12).sum()),
               "ingest_algorithmic_bytes": ingest_bytes,
               "emit_algorithmic_bytes": emit_bytes, "tiers": []}
        lay["host_cast_upload"] = host_baseline(views, bufs, n, a.host_reps)

        # stand-alone ingest, tiers alternated run by run on the same uploaded views
        vp = api._dev_alloc(views.nbytes)
        api._h2d(vp, views)
        bps = []
        for b in bufs:
            p = api._dev_alloc(b.nbytes)
            api._h2d(p, b)
            bps.append(p)
        runs = {"1": [], "0": []}
        tier_seen = {}
        for it in range(a.warmup + a.reps):
            for knob in ("1", "0"):
                os.environ["DD_VIEW_LDS"] = knob
                ing = api.ViewIngest(vp.value, None, n, [p.value for p in bps],
                                     [int(b.nbytes) for b in bufs])
                tier_seen[knob] = ing.tier()
                if it >= a.warmup:
                    runs[knob].append(ing.kernel_ms())
                ing.destroy()
        for p in [vp] + bps:
            api.lib().dd_dev_free(p)

        # through the partitioner: the batch ingests the column, then emit on its output
        os.environ.pop("DD_VIEW_LDS", None)
        bcols = list(cols)
        bcols[1] = {"dtype": "utf8view", "views": views, "bufs": bufs, "valid": None}
        batch = api.DeviceBatch(bcols)
        part = api.Partitioner(batch, keys, a.parts)
        pms = []
        for _ in range(a.warmup + 3):
            part.run()
            part.sync()
            pms.append(sum(part.kernel_ms()))
        lay["partitioner_ms"] = round(statistics.median(pms[a.warmup:]), 4)
        lay["partitioner_info"] = part.info()
        eruns = {"1": [], "0": []}
        for it in range(a.warmup + a.reps):
            for knob in ("1", "0"):
                os.environ["DD_VIEW_LDS"] = knob
                em = api.ViewEmit(part, 1, a.windows)
                if it >= a.warmup:
                    eruns[knob].append(em.kernel_ms())
                em.destroy()
        os.environ.pop("DD_VIEW_LDS", None)
        part.destroy()
        batch.free()

        for knob in ("1", "0"):
            ing_tot = [sum(r) for r in runs[knob]]
            em_tot = [sum(r) for r in eruns[knob]]
            ig = ingest_bytes / statistics.median(ing_tot) / 1e6
            eg = emit_bytes / statistics.median(em_tot) / 1e6
            lay["tiers"].append({
                "tier": "lds" if knob == "1" else "direct",
                "ingest_tier_reported": tier_seen[knob],
                "ingest_ms": {k: stats([r[i] for r in runs[knob]])
                              for i, k in enumerate(("len", "scan", "copy"))},
                "ingest_total_ms": stats(ing_tot),
                "emit_ms": {k: stats([r[i] for r in eruns[knob]])
                            for i, k in enumerate(("scan", "build", "copy"))},
                "emit_total_ms": stats(em_tot),
                "ingest_GBps": round(ig, 1), "emit_GBps": round(eg, 1),
                "ingest_frac_of_stream": round(ig / STREAM_CEILING_GBPS, 3),
                "emit_frac_of_stream": round(eg / STREAM_CEILING_GBPS, 3),
                "ingest_over_partitioner": round(
                    statistics.median(ing_tot) / lay["partitioner_ms"], 3),
                "emit_over_partitioner": round(
                    statistics.median(em_tot) / lay["partitioner_ms"], 3),
                "host_cast_upload_over_ingest": round(
                    lay["host_cast_upload"]["total_ms_median"] /
                    statistics.median(ing_tot), 1),
            })
        res["layouts"].append(lay)
        print(f"# {name} done", file=sys.stderr, flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
