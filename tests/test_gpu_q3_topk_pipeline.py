"""TPC-H q3 carried to its ten result rows on the device (marked gpu): the q3 shape of
tests/test_gpu_join_device_pipeline.py, then what that test leaves to the host. Join ->
partial aggregate -> shuffle on the group keys -> api.final_merge_device -> api.sort_topk on
[revenue DESC, o_orderdate ASC NULLS LAST, l_orderkey ASC] with fetch=10 per partition (the
SortExec) -> api.sort_topk again over the collapsed layout with fetch=10 (the
SortPreservingMergeExec). No column passes through the host between the second shuffle and
the ten rows. Revenue is an exact i64 sum and the trailing group key makes the order total, so
the result equals the direct pyarrow plan row for row, without a tolerance."""

import numpy as np
import pytest
import pyarrow.compute as pc

from datafusion_distributed_amd import api, finalagg, sortref
from tests.test_gpu_join_device_pipeline import CUTOFF, make_tables

pytestmark = pytest.mark.gpu

LIMIT = 10


def direct_answer(pa, cust, orders, li):
    """The single-node plan: join, group_by, sort_by, slice."""
    tc, to, tl = pa.table(cust), pa.table(orders), pa.table(li)
    tc = tc.filter(pc.equal(tc["c_mktsegment"], 0))
    to = to.filter(pc.less(to["o_orderdate"], CUTOFF))
    tl = tl.filter(pc.greater(tl["l_shipdate"], CUTOFF))
    oj = to.join(tc.select(["c_custkey"]), keys="o_custkey", right_keys="c_custkey",
                 join_type="inner")
    lj = tl.join(oj.select(["o_orderkey", "o_orderdate", "o_shippriority"]),
                 keys="l_orderkey", right_keys="o_orderkey", join_type="inner")
    g = lj.group_by(["l_orderkey", "o_orderdate", "o_shippriority"]).aggregate(
        [("revenue", "sum")])
    return g.sort_by([("revenue_sum", "descending"), ("o_orderdate", "ascending"),
                      ("l_orderkey", "ascending")]).slice(0, LIMIT)


def shuffled(comm, cols, key_idx, P):
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, P)
    part.run()
    part.sync()
    return batch, part, comm.exchange(part)


def test_q3_from_two_shuffles_to_ten_rows_on_the_device():
    import pyarrow as pa

    rng = np.random.default_rng(55)
    cust, orders, li = make_tables(rng, n_cust=4_000, n_orders=40_000, n_li=160_000)
    # revenue in integer units: price in cents x (100 - discount in percent)
    li["revenue"] = (np.round(li.pop("l_extendedprice") * 100).astype(np.int64)
                     * (100 - np.round(li.pop("l_discount") * 100).astype(np.int64)))
    P = 16
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    held = []

    building = cust["c_custkey"][cust["c_mktsegment"] == 0]
    omask = (orders["o_orderdate"] < CUTOFF) & np.isin(orders["o_custkey"], building)
    oj = {k: v[omask] for k, v in orders.items()}
    obatch, opart, oex = shuffled(comm, [
        {"dtype": "i64", "data": oj["o_orderkey"], "valid": None},
        {"dtype": "i32", "data": oj["o_orderdate"], "valid": None},
        {"dtype": "i32", "data": oj["o_shippriority"], "valid": None}], [0], P)
    lmask = li["l_shipdate"] > CUTOFF
    lbatch, lpart, lex = shuffled(comm, [
        {"dtype": "i64", "data": li["l_orderkey"][lmask], "valid": None},
        {"dtype": "i64", "data": li["revenue"][lmask], "valid": None}], [0], P)
    held += [opart, lpart, oex, lex]  # destroyed in reverse: a window before its partitioner

    # 1, 2: the join over the two windows and the partial aggregate over its output
    oview, olay = api.exchanged_batch(oex)
    lview, llay = api.exchanged_batch(lex)
    j = api.hash_join(oview, [0], lview, [0], "inner", olay, llay,
                      build_proj=[1, 2], probe_proj=[0, 1])
    held.append(j)
    jview, _ = j.batch()  # o_orderdate, o_shippriority, l_orderkey, revenue
    ops = ["sum_i64", "count"]
    res = api.partial_reduce(jview, [2, 0, 1], [(3, "sum_i64"), (None, "count")])
    assert not res["keynull"].any()

    # 3: the partial states shuffled on the group keys
    pcols, key_idx, aggs = finalagg.partial_state_cols(res, ["i64", "i32", "i32"], ops)
    pbatch, ppart, pex = shuffled(comm, pcols, key_idx, P)
    held += [ppart, pex]

    # 4: the final merge, its result kept on the device as columns:
    #    l_orderkey, o_orderdate, o_shippriority, revenue, count
    pview, play = api.exchanged_batch(pex)
    merged = api.final_merge_device(pview, key_idx, aggs, **play)
    held.append(merged)
    mview, mlay = merged.batch()
    assert mlay["n_parts"] == P and mview.desc.n_cols == 5

    # 5: SortExec TopK(fetch=10), preserve_partitioning: per partition
    keys = [(3, True, True), (1, False, False), (0, False, False)]
    top = api.sort_topk(mview, keys, mlay, fetch=LIMIT)
    held.append(top)
    tview, tlay = top.batch()
    groups_p = np.diff(mlay["seg_offsets"])
    assert np.array_equal(np.diff(tlay["seg_offsets"]), np.minimum(groups_p, LIMIT))
    assert (groups_p > LIMIT).any()  # the fetch did cut

    # 6: SortPreservingMergeExec(fetch=10): the same sort over the collapsed layout
    final = api.sort_topk(tview, keys, sortref.collapsed_layout(tview.n_rows), fetch=LIMIT)
    held.append(final)
    got = {name: final.col(i) for i, name in enumerate(
        ["l_orderkey", "o_orderdate", "o_shippriority", "revenue", "count"])}
    n_groups = merged.n_groups
    for h in reversed(held):
        h.destroy()
    comm.destroy()
    for b in (obatch, lbatch, pbatch):
        b.free()

    want = direct_answer(pa, cust, orders, li)
    assert want.num_rows == LIMIT < n_groups
    assert final.n_rows == LIMIT
    assert got["l_orderkey"]["data"].tolist() == want["l_orderkey"].to_pylist()
    assert got["o_orderdate"]["data"].tolist() == want["o_orderdate"].to_pylist()
    assert got["o_shippriority"]["data"].tolist() == want["o_shippriority"].to_pylist()
    assert got["revenue"]["data"].tolist() == want["revenue_sum"].to_pylist()
    for name in ("l_orderkey", "o_orderdate", "o_shippriority", "revenue"):
        assert got[name]["valid"].all()
    assert "valid" not in got["count"] and (got["count"]["data"] >= 1).all()
