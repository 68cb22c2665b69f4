"""GPU parity tests (marked gpu): the HIP path through the C ABI must match the CPU oracle
bit-exactly — pids, partition offsets, and the stable scatter of every column type —
on the committed golden fixtures, edge cases, and larger randomized batches.
No CPU fallback exists: these tests exercise libdd_shuffle.so's kernels or fail."""

import glob
import os

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

import importlib.util

_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(GOLDEN, "gen_golden.py"))
gen_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen_golden)


def compare_to_oracle(part, cols, key_idx, nparts, ref=None):
    """Compare everything a run partitioner exposes with the CPU oracle's repartition of
    `cols`: pids (when the path keeps a pid array), row offsets, every column's data,
    validity, utf8 lengths, bytes and byte offsets. `ref` passes in an oracle result
    computed earlier for the same arguments."""
    if ref is None:
        ref = oracle.repartition(cols, key_idx, nparts)
    n = part.batch.n_rows
    pd = part.pids()  # None when the spec path recomputes hashes in-kernel
    if n and pd is not None:
        assert (pd == ref["pid"]).all(), "partition ids differ"
    assert (part.row_offsets() == ref["part_offsets"]).all(), "row offsets differ"
    for i, col in enumerate(cols):
        got = part.col_out(i)
        exp = ref["cols"][i]
        if col["dtype"] == "utf8":
            assert (got["lengths"] == exp["lengths"]).all(), f"col {i} lengths differ"
            # the output buffer is as long as the input's (data_len); its first
            # offsets[n] - offsets[0] bytes are defined, whatever follows them is not
            assert len(got["data"]) == np.asarray(col["data"], dtype=np.uint8).nbytes
            total = len(exp["data"])
            assert got["data"][:total].tobytes() == exp["data"].tobytes(), \
                f"col {i} bytes differ"
            # byte offsets = prefix of lengths at partition boundaries
            boff = part.byte_offsets(i)
            lens64 = exp["lengths"].astype(np.int64)
            pref = np.zeros(n + 1, dtype=np.int64)
            if n:
                pref[1:] = np.cumsum(lens64)
            expected_boff = pref[ref["part_offsets"]]
            assert (boff == expected_boff).all(), \
                f"col {i} byte offsets differ: {boff} vs {expected_boff}"
            # staged engines also rebuild the Arrow offsets of the partition-major output
            off64 = part.var_offsets64(i)
            if off64 is not None:
                assert off64.shape == (n + 1,)
                assert (off64.astype(np.int64) == pref).all(), \
                    f"col {i} var_offsets64 differ (last: {off64[-1]} vs {pref[-1]})"
        elif col["dtype"] in ("f32", "f64"):
            assert np.array_equal(got["data"], exp["data"], equal_nan=True), \
                f"col {i} data differ"
        else:
            assert (got["data"] == exp["data"]).all(), f"col {i} data differ"
        if col.get("valid") is not None:
            assert (got["valid"] == exp["valid"]).all(), f"col {i} validity differs"


def assert_info(part, expect):
    """Assert the plan the partitioner chose (Partitioner.info()). `expect` maps a field
    to its required value, or to a predicate over the value."""
    info = part.info()
    for name, want in (expect or {}).items():
        got = info[name]
        good = want(got) if callable(want) else got == want
        assert good, f"info()[{name!r}] = {got}, not the tier this test names: {info}"
    return info


def check_against_oracle(cols, key_idx, nparts, expect=None):
    """One create / run / compare / destroy. `expect` (see assert_info) pins the scatter
    tier the case is meant to exercise, checked before the run."""
    ref = oracle.repartition(cols, key_idx, nparts)
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        assert_info(part, expect)
        part.run()
        part.sync()
        compare_to_oracle(part, cols, key_idx, nparts, ref=ref)
    finally:
        part.destroy()
        batch.free()


@pytest.mark.parametrize("fname", sorted(glob.glob(os.path.join(GOLDEN, "*_p*.npz"))))
def test_gpu_matches_golden(fname):
    cols, key_idx, nparts, _ = gen_golden.load_case(fname)
    check_against_oracle(cols, key_idx, nparts)


def test_gpu_empty_batch():
    cols = [{"dtype": "i64", "data": np.zeros(0, dtype=np.int64), "valid": None}]
    check_against_oracle(cols, [0], 8)


def test_gpu_single_partition():
    rng = np.random.default_rng(1)
    cols = [{"dtype": "i64", "data": rng.integers(0, 1000, 10000, dtype=np.int64),
             "valid": None}]
    check_against_oracle(cols, [0], 1)


def test_gpu_all_null_key():
    n = 4096
    cols = [
        {"dtype": "i64", "data": np.arange(n, dtype=np.int64),
         "valid": np.zeros(n, dtype=np.uint8)},
        {"dtype": "f64", "data": np.random.default_rng(2).normal(size=n), "valid": None},
    ]
    check_against_oracle(cols, [0], 16)


def test_gpu_skew_single_key():
    # every row has the same key -> one partition takes everything (atomic/ranking stress)
    n = 100000
    cols = [{"dtype": "i64", "data": np.full(n, 42, dtype=np.int64), "valid": None},
            {"dtype": "i32", "data": np.arange(n, dtype=np.int32), "valid": None}]
    check_against_oracle(cols, [0], 64)


def test_gpu_skew_zipf_utf8_payload():
    # ClickBench-UserID stand-in: Zipf(1.1) keys + var-width payload
    rng = np.random.default_rng(9)
    n = 200000
    keys = rng.zipf(1.1, n).astype(np.int64) % 100000
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum(rng.integers(0, 32, n))
    # random bytes: a byte moved to the wrong place must differ from the one it replaces
    data = np.random.default_rng(90).integers(33, 127, int(off[-1]), dtype=np.int64)
    cols = [
        {"dtype": "i64", "data": keys, "valid": None},
        {"dtype": "utf8", "data": data.astype(np.uint8),
         "offsets": off, "valid": (rng.random(n) > 0.1).astype(np.uint8)},
    ]
    check_against_oracle(cols, [0], 128)


def test_gpu_2m_rows_q3_shape():
    # the bench workload shape at reduced size: q3 projection, i64 key, P=128
    rng = np.random.default_rng(42)
    n = 2_000_000
    cols = [
        {"dtype": "i64", "data": rng.integers(1, 60_000_000, n, dtype=np.int64),
         "valid": None},
        {"dtype": "f64", "data": rng.uniform(900, 105000, n), "valid": None},
        {"dtype": "f64", "data": rng.uniform(0, 0.1, n), "valid": None},
        {"dtype": "i32", "data": rng.integers(8000, 11000, n, dtype=np.int64)
         .astype(np.int32), "valid": None},
    ]
    check_against_oracle(cols, [0], 128)


def test_gpu_p2048_max_partitions():
    rng = np.random.default_rng(3)
    n = 500000
    cols = [{"dtype": "i64", "data": rng.integers(0, 2**63 - 1, n, dtype=np.int64),
             "valid": None}]
    check_against_oracle(cols, [0], 2048)


def test_gpu_multikey_mixed():
    cols = gen_golden.make_bench_batch(100000, seed=77)
    check_against_oracle(cols, [0, 3, 4], 32)


def test_gpu_task_cache_lifecycle():
    """set_plan / execute_task / drop_task mirror (task_data.rs): unknown key fails with
    NOT_FOUND; execute is idempotent across partition-range requests."""
    import ctypes
    import uuid

    from datafusion_distributed_amd import TaskKey
    from datafusion_distributed_amd.shuffle import ExecuteTaskRequest, InProcessGpuChannel

    rng = np.random.default_rng(4)
    n, P = 10000, 12
    cols = [{"dtype": "i64", "data": rng.integers(0, 10**9, n, dtype=np.int64),
             "valid": None}]
    batch = api.DeviceBatch(cols)
    key = TaskKey(uuid.uuid4(), 3, 0)
    keyc = key.to_c()
    keys = (ctypes.c_int32 * 1)(0)

    # unknown key -> NOT_FOUND (mirrors impl_execute_task plan-wait timeout)
    h = ctypes.c_void_p()
    st = api.lib().dd_execute_task(ctypes.byref(keyc), 0, 1, None, ctypes.byref(h))
    assert st == 5

    api._check(api.lib().dd_set_plan(ctypes.byref(keyc), ctypes.byref(batch.desc),
                                     keys, 1, ctypes.c_uint32(P)))
    ch = InProcessGpuChannel()
    p1 = ch.execute_task(ExecuteTaskRequest(key, 0, 6, P))
    p2 = ch.execute_task(ExecuteTaskRequest(key, 6, 12, P))
    assert p1.h.value == p2.h.value  # same cached task state, ran once
    p1.batch = batch
    p1.sync()
    ref = oracle.repartition(cols, [0], P)
    pd = p1.pids()
    if pd is not None:
        assert (pd == ref["pid"]).all()
    assert (p1.row_offsets() == ref["part_offsets"]).all()
    api._check(api.lib().dd_drop_task(ctypes.byref(keyc)))
    st = api.lib().dd_execute_task(ctypes.byref(keyc), 0, 1, None, ctypes.byref(h))
    assert st == 5  # dropped
    batch.free()


@pytest.mark.parametrize("staged_var", ["0", "1"])
def test_gpu_staged_var_two_utf8_with_nulls(staged_var, monkeypatch):
    # two var cols + nulls + f64 through BOTH var paths: v1 direct (default) and the
    # staged-var path (DD_V2_VAR=1: synthetic VARLEN/ROWID columns + K4 byte
    # materialization with device-rebuilt Arrow offsets)
    monkeypatch.setenv("DD_V2_VAR", staged_var)
    rng = np.random.default_rng(17)
    n = 300000

    def utf8(maxlen, null_p):
        lens = rng.integers(0, maxlen, n)
        off = np.zeros(n + 1, dtype=np.int32)
        off[1:] = np.cumsum(lens)
        data = rng.integers(32, 127, int(off[-1]), dtype=np.int64).astype(np.uint8)
        valid = (rng.random(n) > null_p).astype(np.uint8) if null_p else None
        return {"dtype": "utf8", "data": data, "offsets": off, "valid": valid}

    cols = [
        {"dtype": "i64", "data": rng.integers(0, 10**12, n, dtype=np.int64), "valid": None},
        utf8(48, 0.15),
        utf8(8, 0.0),
        {"dtype": "f64", "data": rng.normal(size=n), "valid": None},
    ]
    check_against_oracle(cols, [0], 64, expect={"path": 0} if staged_var == "0"
                         else {"path": 1, "k5": 0})
