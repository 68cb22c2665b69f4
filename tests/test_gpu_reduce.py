"""GPU partial aggregation (marked gpu): final-merge of the GPU partials must equal direct
aggregation by pyarrow — exact on counts/keys, <=1e-6 relative on float sums (the
reference's correctness bar: tests/tpch_correctness_test.rs:139-158 analog). The final
merge is oracle/reduce_ref.final_merge (op-aware, exact; proven on CPU in
test_reduce_ref_cpu.py); the exact-model comparison lives in test_gpu_reduce_parity.py."""

import numpy as np
import pytest

from datafusion_distributed_amd import api
from oracle import reduce_ref as rr

pytestmark = pytest.mark.gpu


def run_and_merge(cols, key_idx, aggs):
    """partial_reduce + final merge -> (raw partial, {group id: [merged values]}). Row
    conservation: the merged counts of a count aggregate, and the non-null input counts
    of every aggregate over a column without NULLs, must add up to the input rows."""
    batch = api.DeviceBatch(cols)
    try:
        res = api.partial_reduce(batch, key_idx, aggs)
    finally:
        batch.free()
    ops = [o for _, o in aggs]
    final = rr.final_merge(res, ops)
    merged = {gid: [e["value"] for e in ent] for gid, ent in final.items()}
    n = len(cols[0]["data"])
    for g, (ci, op) in enumerate(aggs):
        if op == "count":
            assert sum(v[g] for v in merged.values()) == n
        if op == "count" or cols[ci]["valid"] is None:  # every row is a non-null input
            assert sum(ent[g]["nn"] for ent in final.values()) == n
    return res, merged


def f64_of(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def masked(data, valid):
    import pyarrow as pa

    return pa.array(data, mask=~valid.astype(bool))


def test_partial_reduce_q1_low_cardinality():
    import pyarrow as pa

    rng = np.random.default_rng(23)
    n = 300_000
    rf = rng.integers(0, 3, n, dtype=np.int64).astype(np.uint8)
    ls = rng.integers(0, 2, n, dtype=np.int64).astype(np.uint8)
    qty = rng.uniform(1, 50, n)
    price = rng.uniform(900, 105000, n)
    cols = [
        {"dtype": "u8", "data": rf, "valid": None},
        {"dtype": "u8", "data": ls, "valid": None},
        {"dtype": "f64", "data": qty, "valid": None},
        {"dtype": "f64", "data": price, "valid": None},
    ]
    res, merged = run_and_merge(cols, [0, 1], [(2, "sum_f64"), (3, "sum_f64"),
                                               (None, "count")])
    # partial output is small: 6 true groups per block plus bounded claim-race
    # duplicates (dd_reduce.hip probe notes); far below the input row count
    assert len(res["keynull"]) <= 64 * 64

    tbl = pa.table({"rf": rf, "ls": ls, "qty": qty, "price": price})
    direct = tbl.group_by(["rf", "ls"]).aggregate([("qty", "sum"), ("price", "sum"),
                                                   ([], "count_all")])
    assert len(merged) == direct.num_rows
    for i in range(direct.num_rows):
        key = ((direct["rf"][i].as_py(), direct["ls"][i].as_py()), 0)
        got = merged[key]
        assert got[2] == direct["count_all"][i].as_py()  # counts exact
        assert abs(got[0] - direct["qty_sum"][i].as_py()) <= 1e-6 * abs(
            direct["qty_sum"][i].as_py())
        assert abs(got[1] - direct["price_sum"][i].as_py()) <= 1e-6 * abs(
            direct["price_sum"][i].as_py())


def test_partial_reduce_high_cardinality_spills():
    # 40k distinct i64 keys over 150k rows: every block sees several times more groups
    # than table slots -> spill path exercised
    rng = np.random.default_rng(29)
    n = 150_000
    keys = rng.integers(0, 40_000, n, dtype=np.int64)
    vals = rng.normal(size=n)
    res, merged = run_and_merge([
        {"dtype": "i64", "data": keys, "valid": None},
        {"dtype": "f64", "data": vals, "valid": None},
    ], [0], [(1, "sum_f64"), (None, "count")])
    geo = api.partial_reduce_geometry(n)
    # table rows are at most nblocks * table_slots: anything beyond is a spilled singleton
    assert len(res["keynull"]) > geo["nblocks"] * geo["table_slots"]
    # numpy groupby cross-check of EVERY group
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], vals[order]
    bounds = np.flatnonzero(np.diff(sk)) + 1
    starts = np.concatenate([[0], bounds])
    ends = np.concatenate([bounds, [n]])
    uk = sk[starts]
    sums = np.add.reduceat(sv, starts)
    counts = ends - starts
    gids = sorted(merged)
    assert all(mask == 0 for _, mask in gids)
    assert np.array_equal(np.array([g[0][0] for g in gids], dtype=np.int64), uk)
    assert np.array_equal(np.array([merged[g][1] for g in gids]), counts)
    got_sums = np.array([merged[g][0] for g in gids])
    assert (np.abs(got_sums - sums) <= 1e-6 * np.maximum(np.abs(sums), 1.0)).all()


def test_partial_reduce_null_keys_and_null_aggs():
    import pyarrow as pa

    rng = np.random.default_rng(31)
    n = 100_000
    k = rng.integers(0, 5, n, dtype=np.int64).astype(np.int32)
    kvalid = (rng.random(n) > 0.1).astype(np.uint8)
    v = rng.normal(size=n)
    vvalid = (rng.random(n) > 0.2).astype(np.uint8)
    _, merged = run_and_merge([
        {"dtype": "i32", "data": k, "valid": kvalid},
        {"dtype": "f64", "data": v, "valid": vvalid},
    ], [0], [(1, "sum_f64"), (None, "count")])

    tbl = pa.table({"k": masked(k, kvalid), "v": masked(v, vvalid)})
    direct = tbl.group_by("k").aggregate([("v", "sum"), ([], "count_all")])
    assert len(merged) == direct.num_rows
    for i in range(direct.num_rows):
        kv = direct["k"][i].as_py()
        key = ((0,), 1) if kv is None else ((kv,), 0)
        got = merged[key]
        assert got[1] == direct["count_all"][i].as_py()
        want = direct["v_sum"][i].as_py()
        if want is None:
            assert got[0] is None
        else:
            assert abs(got[0] - want) <= 1e-6 * max(abs(want), 1.0)


def test_partial_reduce_all_null_group_is_null():
    """A group whose aggregate inputs are ALL NULL must merge to NULL, not the op
    identity (DataFusion: SUM(v)=NULL, MIN(v)=NULL over an all-null group; COUNT(*)
    still counts rows). Pinned vs pyarrow direct aggregation."""
    import pyarrow as pa

    rng = np.random.default_rng(41)
    n = 50_000
    k = rng.integers(0, 8, n, dtype=np.int64)
    v = rng.normal(size=n)
    vvalid = (k != 3).astype(np.uint8)  # group 3: every aggregate input is NULL
    _, merged = run_and_merge([
        {"dtype": "i64", "data": k, "valid": None},
        {"dtype": "f64", "data": v, "valid": vvalid},
    ], [0], [(1, "sum_f64"), (1, "min_f64"), (None, "count")])

    tbl = pa.table({"k": pa.array(k), "v": masked(v, vvalid)})
    direct = tbl.group_by("k").aggregate([("v", "sum"), ("v", "min"), ([], "count_all")])
    assert len(merged) == direct.num_rows
    saw_null = False
    for i in range(direct.num_rows):
        kv = direct["k"][i].as_py()
        got = merged[((kv,), 0)]
        want = direct["v_sum"][i].as_py()
        if want is None:
            assert got[0] is None, f"group {kv} v_sum: want NULL, got {got[0]}"
            saw_null = True
        else:
            assert abs(got[0] - want) <= 1e-6 * max(abs(want), 1.0)
        want = direct["v_min"][i].as_py()
        if want is None:
            assert got[1] is None, f"group {kv} v_min: want NULL, got {got[1]}"
        else:
            assert f64_of(got[1]) == want  # a minimum is one of the inputs: exact
        assert got[2] == direct["count_all"][i].as_py()
    assert saw_null


def test_partial_reduce_min_max():
    import pyarrow as pa

    rng = np.random.default_rng(37)
    n = 200_000
    k = rng.integers(0, 64, n, dtype=np.int64)
    f = rng.normal(size=n) * 1000
    i = rng.integers(-(2**60), 2**60, n, dtype=np.int64)
    _, merged = run_and_merge([
        {"dtype": "i64", "data": k, "valid": None},
        {"dtype": "f64", "data": f, "valid": None},
        {"dtype": "i64", "data": i, "valid": None},
    ], [0], [(1, "min_f64"), (1, "max_f64"), (2, "min_i64"), (2, "max_i64")])

    tbl = pa.table({"k": k, "f": f, "i": i})
    direct = tbl.group_by("k").aggregate([("f", "min"), ("f", "max"), ("i", "min"),
                                          ("i", "max")])
    assert len(merged) == direct.num_rows
    for r in range(direct.num_rows):
        got = merged[((direct["k"][r].as_py(),), 0)]
        assert f64_of(got[0]) == direct["f_min"][r].as_py()
        assert f64_of(got[1]) == direct["f_max"][r].as_py()
        assert got[2] == direct["i_min"][r].as_py()
        assert got[3] == direct["i_max"][r].as_py()


def test_partial_reduce_dict_key():
    import pyarrow as pa

    rng = np.random.default_rng(41)
    n = 200_000
    nvals = 10
    vals = [f"cat{v}".encode() for v in range(nvals)]
    dby = np.frombuffer(b"".join(vals), dtype=np.uint8).copy()
    doff = np.zeros(nvals + 1, dtype=np.int32)
    doff[1:] = np.cumsum([len(v) for v in vals])
    idx = rng.integers(0, nvals, n).astype(np.int32)
    x = rng.normal(size=n)
    _, merged = run_and_merge([
        {"dtype": "dict32", "data": idx, "dict_bytes": dby, "dict_offsets": doff,
         "valid": None},
        {"dtype": "f64", "data": x, "valid": None},
    ], [0], [(1, "sum_f64"), (None, "count")])
    tbl = pa.table({"k": idx, "v": x})
    direct = tbl.group_by("k").aggregate([("v", "sum"), ([], "count_all")])
    assert len(merged) == direct.num_rows
    for r in range(direct.num_rows):
        got = merged[((direct["k"][r].as_py(),), 0)]
        assert got[1] == direct["count_all"][r].as_py()
        want = direct["v_sum"][r].as_py()
        assert abs(got[0] - want) <= 1e-6 * max(abs(want), 1.0)
