"""TPC-H q13's stage 3 at test size with the LEFT join on the device (marked gpu; DESIGN.md
§20): HashJoinExec mode=Partitioned, join_type=Left, on=[(c_custkey, o_custkey)],
projection=[c_custkey, o_orderkey] directly above two shuffles and directly below a partial
aggregate. customer and orders are shuffled on the join key and exchanged; api.outer_join
runs over the two exchanged windows with customer as the build side; api.partial_reduce
groups Joined.batch() by c_custkey, and the aggregate's non-null count over the
NULL-extended o_orderkey is count(o_orderkey). No exchanged column is copied to the host;
only the partial aggregate rows are. The c_count -> custdist histogram is held to the direct
pyarrow plan over the full tables. Everything is an integer and everything is exact."""

from collections import Counter

import numpy as np
import pytest

from datafusion_distributed_amd import api

pytestmark = pytest.mark.gpu


def test_q13_pipeline_with_the_left_join_on_the_device():
    import pyarrow as pa

    rng = np.random.default_rng(13)
    n_cust, n_orders, P = 15_000, 150_000, 16
    c_custkey = np.arange(1, n_cust + 1, dtype=np.int64)
    # as in TPC-H, a third of the customers place no order
    buyers = c_custkey[c_custkey % 3 != 0]
    o_custkey = rng.choice(buyers, n_orders)
    o_orderkey = np.arange(1, n_orders + 1, dtype=np.int64) * 4
    comm = api.Comm(api.Comm.unique_id(), 0, 1)

    # ---- stages 1 and 2: both tables shuffled on the join key, same P, and exchanged
    cbatch = api.DeviceBatch([{"dtype": "i64", "data": c_custkey, "valid": None}])
    cpart = api.Partitioner(cbatch, [0], P)
    cpart.run()
    cpart.sync()
    cex = comm.exchange(cpart)
    obatch = api.DeviceBatch([{"dtype": "i64", "data": o_orderkey, "valid": None},
                              {"dtype": "i64", "data": o_custkey, "valid": None}])
    opart = api.Partitioner(obatch, [1], P)
    opart.run()
    opart.sync()
    oex = comm.exchange(opart)

    # ---- stage 3 on the device: the LEFT join, then the partial aggregate over its output
    cview, clay = api.exchanged_batch(cex)
    oview, olay = api.exchanged_batch(oex)
    assert clay["n_parts"] == olay["n_parts"] == P
    j = api.outer_join(cview, [0], oview, [1], "left", clay, olay, build_proj=[0],
                       probe_proj=[0])
    jview, jlay = j.batch()  # c_custkey, o_orderkey (nullable)
    joff = j.seg_offsets()
    n_joined = j.n_rows
    assert joff[0] == 0 and (np.diff(joff) >= 0).all() and joff[-1] == n_joined == jview.n_rows
    assert np.array_equal(jlay["seg_part"],
                          np.concatenate([olay["seg_part"], clay["seg_part"]]))
    res = api.partial_reduce(jview, [0], [(1, "max_i64"), (None, "count")])
    for h in (j, cex, oex, cpart, opart, comm):
        h.destroy()
    cbatch.free()
    obatch.free()

    # ---- stage 4: merge the partial rows on the host: c_count, then custdist
    assert not res["keynull"].any()
    c_count = Counter()
    rows = Counter()
    for k, nn, c in zip(res["keys"][:, 0].tolist(), res["nn"][:, 0].tolist(),
                        np.ascontiguousarray(res["aggs"][:, 1]).view(np.int64).tolist()):
        c_count[k] += nn
        rows[k] += c
    custdist = Counter(c_count.values())

    tc = pa.table({"c_custkey": c_custkey})
    to = pa.table({"o_orderkey": o_orderkey, "o_custkey": o_custkey})
    lj = tc.join(to, keys="c_custkey", right_keys="o_custkey", join_type="left outer")
    per_cust = lj.group_by("c_custkey").aggregate([("o_orderkey", "count")])
    want = dict(zip(per_cust["c_custkey"].to_pylist(), per_cust["o_orderkey_count"].to_pylist()))
    want_dist = per_cust.group_by("o_orderkey_count").aggregate([("c_custkey", "count")])

    assert n_joined == lj.num_rows == n_orders + n_cust - len(np.unique(o_custkey))
    assert dict(c_count) == want
    # a customer without orders stands in the join's output once, with count(o_orderkey) = 0
    assert all(rows[k] == max(c, 1) for k, c in want.items())
    assert custdist[0] >= n_cust // 3
    assert dict(custdist) == dict(zip(want_dist["o_orderkey_count"].to_pylist(),
                                      want_dist["c_custkey_count"].to_pylist()))
