"""bench.py --dump-outputs: the dump helper on a stand-in partitioner (CPU), and the real
flag end to end on the GPU checked against the oracle."""

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench
import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OraclePart:
    """Quacks like api.Partitioner after run(), with the oracle's result behind it."""

    def __init__(self, cols, key, nparts):
        self.ref = oracle.repartition(cols, key, nparts)
        self.batch = types.SimpleNamespace(cols=cols, n_rows=len(self.ref["pid"]))

    def row_offsets(self):
        return self.ref["part_offsets"]

    def col_out(self, i):
        return self.ref["cols"][i]  # same dict shape as Partitioner.col_out


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_is_complete(tmp_path):
    cols, key = bench.make_clickbench_userid(3001, seed=5)
    cols[2]["valid"] = (np.arange(3001) % 7 != 0).astype(np.uint8)
    part = OraclePart(cols, key, 13)
    bench.dump_outputs(part, str(tmp_path))
    got = load_dir(str(tmp_path))
    ref = part.ref
    assert "sample_rows" not in got
    assert got["row_offsets"].dtype == np.float64
    assert (got["row_offsets"] == ref["part_offsets"]).all()
    assert (got["col0_i64"] == ref["cols"][0]["data"]).all()
    assert (got["col1_utf8_bytes"] == ref["cols"][1]["data"]).all()
    assert (got["col1_utf8_lengths"] == ref["cols"][1]["lengths"]).all()
    assert (got["col2_i64_valid"] == ref["cols"][2]["valid"]).all()
    assert (got["col3_i32"] == ref["cols"][3]["data"]).all()
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())


def test_dump_large_is_a_fixed_sample_within_budget(tmp_path):
    cols, key = bench.make_lineitem_utf8key(20_000, seed=3)
    part = OraclePart(cols, key, 8)
    budget = 64 << 10
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(part, str(a), budget=budget)
    bench.dump_outputs(part, str(b), "rank1_", budget=budget)
    ga, gb = load_dir(str(a)), load_dir(str(b))
    assert sum(v.nbytes for v in ga.values()) <= budget + ga["row_offsets"].nbytes
    assert sorted("rank1_" + k for k in ga) == sorted(gb)
    for k, v in ga.items():  # same rows every time
        assert np.array_equal(v, gb["rank1_" + k])
    rows = ga["sample_rows"].astype(np.int64)
    assert 0 < len(rows) < 20_000 and (np.diff(rows) >= 0).all()
    assert (ga["col0_i64"] == part.ref["cols"][0]["data"][rows]).all()
    assert (ga["col2_f64"] == part.ref["cols"][2]["data"][rows]).all()
    assert len(ga["col1_utf8_bytes"]) == len(rows)


@pytest.mark.gpu
def test_bench_dump_outputs_matches_oracle(tmp_path):
    rows, steps = 70_001, 3
    out = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
         str(steps), "--warmup", "1", "--rows", str(rows), "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["metric"] == "tpch_sf10_shuffle_GBps" and line["cpu_baseline"] is None
    cols, key = bench.make_lineitem_q3(rows, seed=42)
    ref = oracle.repartition(cols, key, bench.PARTS_PER_RANK)
    got = load_dir(str(out))
    assert (got["row_offsets"] == ref["part_offsets"]).all()
    for i, name in enumerate(["col0_i64", "col1_f64", "col2_f64", "col3_i32"]):
        assert got[name].dtype == np.float64
        assert (got[name] == ref["cols"][i]["data"]).all(), name
