"""TPC-H q3-shaped join pipeline with the join on the device (marked gpu): the pipeline of
tests/test_gpu_join_pipeline.py at about a tenth of its size, with its stage 3 (per-partition
pyarrow joins over host copies) replaced by api.hash_join over the two exchanged windows and
api.partial_reduce over Joined.batch(). No exchanged column is copied to the host; only the
partial aggregate rows are. The whole-query answer is held to the direct pyarrow plan over
the full tables: groups and counts exact, revenue <= 1e-6 relative (DESIGN.md §3, and the
tolerance of the host-join pipeline test)."""

import numpy as np
import pytest
import pyarrow.compute as pc

from datafusion_distributed_amd import api

pytestmark = pytest.mark.gpu

CUTOFF = 9204  # days: 1995-03-15 in the synthetic date space


def make_tables(rng, n_cust=15_000, n_orders=150_000, n_li=600_000):
    cust = {
        "c_custkey": np.arange(1, n_cust + 1, dtype=np.int64),
        "c_mktsegment": rng.integers(0, 5, n_cust).astype(np.int32),  # 0 = BUILDING
    }
    orders = {
        "o_orderkey": np.arange(1, n_orders + 1, dtype=np.int64) * 4,
        "o_custkey": rng.integers(1, n_cust + 1, n_orders, dtype=np.int64),
        "o_orderdate": rng.integers(8000, 10500, n_orders, dtype=np.int64).astype(np.int32),
        "o_shippriority": rng.integers(0, 2, n_orders, dtype=np.int64).astype(np.int32),
    }
    li = {
        "l_orderkey": rng.integers(1, n_orders + 1, n_li, dtype=np.int64) * 4,
        "l_extendedprice": rng.uniform(900, 105000, n_li),
        "l_discount": np.round(rng.uniform(0, 0.1, n_li), 2),
        "l_shipdate": rng.integers(8000, 10500, n_li, dtype=np.int64).astype(np.int32),
    }
    return cust, orders, li


def direct_answer(pa, cust, orders, li):
    """The single-node plan: pure pyarrow over the full tables."""
    tc, to, tl = pa.table(cust), pa.table(orders), pa.table(li)
    tc = tc.filter(pc.equal(tc["c_mktsegment"], 0))
    to = to.filter(pc.less(to["o_orderdate"], CUTOFF))
    tl = tl.filter(pc.greater(tl["l_shipdate"], CUTOFF))
    oj = to.join(tc.select(["c_custkey"]), keys="o_custkey", right_keys="c_custkey",
                 join_type="inner")
    lj = tl.join(oj.select(["o_orderkey", "o_orderdate", "o_shippriority"]),
                 keys="l_orderkey", right_keys="o_orderkey", join_type="inner")
    rev = pc.multiply(lj["l_extendedprice"], pc.subtract(pa.scalar(1.0), lj["l_discount"]))
    lj = lj.append_column("revenue", rev)
    return lj.group_by(["l_orderkey", "o_orderdate", "o_shippriority"]).aggregate(
        [("revenue", "sum"), ("revenue", "count")])


def test_q3_pipeline_with_the_join_on_the_device():
    import pyarrow as pa

    rng = np.random.default_rng(54)
    cust, orders, li = make_tables(rng)
    P = 16
    comm = api.Comm(api.Comm.unique_id(), 0, 1)

    # ---- stage 1: orders filtered and semi-joined with the BUILDING customers (the join
    # above the broadcast, host-side as in the host-join pipeline), shuffled on o_orderkey
    building = cust["c_custkey"][cust["c_mktsegment"] == 0]
    omask = (orders["o_orderdate"] < CUTOFF) & np.isin(orders["o_custkey"], building)
    oj = {k: v[omask] for k, v in orders.items()}
    obatch = api.DeviceBatch([
        {"dtype": "i64", "data": oj["o_orderkey"], "valid": None},
        {"dtype": "i32", "data": oj["o_orderdate"], "valid": None},
        {"dtype": "i32", "data": oj["o_shippriority"], "valid": None},
    ])
    opart = api.Partitioner(obatch, [0], P)
    opart.run()
    opart.sync()
    oex = comm.exchange(opart)

    # ---- stage 2: lineitem filtered, revenue precomputed, shuffled on l_orderkey (same P)
    lmask = li["l_shipdate"] > CUTOFF
    lf = {k: v[lmask] for k, v in li.items()}
    lbatch = api.DeviceBatch([
        {"dtype": "i64", "data": lf["l_orderkey"], "valid": None},
        {"dtype": "f64", "data": lf["l_extendedprice"] * (1.0 - lf["l_discount"]),
         "valid": None},
    ])
    lpart = api.Partitioner(lbatch, [0], P)
    lpart.run()
    lpart.sync()
    lex = comm.exchange(lpart)

    # ---- stage 3 on the device: partitioned hash join of the two windows, orders as the
    # build side, then the partial aggregate over the join's output
    oview, olay = api.exchanged_batch(oex)
    lview, llay = api.exchanged_batch(lex)
    assert olay["n_parts"] == llay["n_parts"] == P
    j = api.hash_join(oview, [0], lview, [0], "inner", olay, llay,
                      build_proj=[1, 2], probe_proj=[0, 1])
    jview, jlay = j.batch()  # o_orderdate, o_shippriority, l_orderkey, revenue
    joff = j.seg_offsets()
    assert joff[0] == 0 and (np.diff(joff) >= 0).all() and joff[-1] == j.n_rows == jview.n_rows
    assert np.array_equal(jlay["seg_part"], llay["seg_part"])
    res = api.partial_reduce(jview, [2, 0, 1], [(3, "sum_f64"), (None, "count")])
    n_joined = j.n_rows
    for h in (j, oex, lex, opart, lpart, comm):
        h.destroy()
    obatch.free()
    lbatch.free()

    # ---- stage 4: merge the partial rows on the host
    merged = {}
    sums = res["aggs"][:, 0]
    counts = np.ascontiguousarray(res["aggs"][:, 1]).view(np.int64)
    assert not res["keynull"].any()
    for (k, d, sp), s, c in zip(res["keys"].tolist(), sums.tolist(), counts.tolist()):
        key = (k, np.int64(d).astype(np.int32).item(), np.int64(sp).astype(np.int32).item())
        rev, cnt = merged.get(key, (0.0, 0))
        merged[key] = (rev + s, cnt + c)

    want = direct_answer(pa, cust, orders, li)
    assert n_joined == sum(want["revenue_count"].to_pylist())
    assert len(merged) == want.num_rows, "group count differs"
    for row in want.to_pylist():
        key = (row["l_orderkey"], row["o_orderdate"], row["o_shippriority"])
        assert key in merged, f"missing group {key}"
        g, c = merged[key]
        w = row["revenue_sum"]
        assert c == row["revenue_count"], f"count differs for {key}"
        assert abs(g - w) <= 1e-6 * max(abs(w), 1.0), f"revenue differs for {key}"
