"""TPC-H q1 Stage 1 -> Stage 2 on native decimals, end to end on the GPU (marked gpu).

The reference's q1 plan puts AggregateExec mode=Partial (eight aggregates over Decimal128)
directly below RepartitionExec Hash([l_returnflag, l_linestatus], 6). Here: the six-state
partial plan (five decimal sums + count; the avgs share the sums' states)
-> hash repartition of the partials -> self exchange -> per-partition final merge with
Python ints, held EXACTLY to pyarrow's direct decimal group-by."""

import decimal

import numpy as np
import pytest

from datafusion_distributed_amd import api, decagg

pytestmark = pytest.mark.gpu


def _dec_array(pa, unscaled, typ):
    """Decimal128Array of the given unscaled i64 values (sign-extended to 16 bytes)."""
    v = np.ascontiguousarray(unscaled, dtype=np.int64)
    words = np.ascontiguousarray(np.stack([v, v >> 63], axis=1))
    return pa.Array.from_buffers(typ, len(v), [None, pa.py_buffer(words)])


def _unscaled(d, scale):
    return None if d is None else int(d.scaleb(scale))


def test_q1_decimal_partial_reduce_shuffle_final():
    import pyarrow as pa
    import pyarrow.compute as pc

    rng = np.random.default_rng(4747)
    n = 200_000
    d152 = pa.decimal128(15, 2)
    rf = rng.integers(0, 3, n).astype(np.uint8)
    ls = rng.integers(0, 2, n).astype(np.uint8)
    qty = _dec_array(pa, rng.integers(100, 5001, n), d152)  # 1.00 .. 50.00
    price = _dec_array(pa, rng.integers(90_000, 10_500_000, n), d152)
    disc = _dec_array(pa, rng.integers(0, 11, n), d152)  # 0.00 .. 0.10
    tax = _dec_array(pa, rng.integers(0, 9, n), d152)
    # the ProjectionExec below the aggregate (not ours): 1 - disc and 1 + tax lie in [0, 2),
    # so narrowing them keeps the products inside 38 digits
    one = pa.scalar(decimal.Decimal(1), pa.decimal128(1, 0))
    d32 = pa.decimal128(3, 2)
    disc_price = pc.multiply(price, pc.cast(pc.subtract(one, disc), d32))
    charge = pc.multiply(disc_price, pc.cast(pc.add(one, tax), d32))
    sums = [("qty", qty), ("price", price), ("disc_price", disc_price), ("charge", charge),
            ("disc", disc)]
    assert all(pa.types.is_decimal128(a.type) for _, a in sums)

    # stage 1: partial aggregation below the shuffle, the six-state plan
    dcols = [api.dec128_col(a) for _, a in sums]
    batch = api.DeviceBatch([{"dtype": "u8", "data": rf, "valid": None},
                             {"dtype": "u8", "data": ls, "valid": None}] + dcols)
    aggs = [(2 + i, "sum_dec128") for i in range(5)] + [(None, "count")]
    try:
        res = api.partial_reduce(batch, [0, 1], aggs)
    finally:
        batch.free()
    assert res["kernel"] == 1
    m = len(res["keynull"])
    assert 0 < m < n / 100  # the exchange moves partials, not rows

    # stage 2: hash-repartition the PARTIALS on the same keys + exchange (1 rank window)
    pcols = [{"dtype": "u8", "data": res["keys"][:, 0].astype(np.uint8), "valid": None},
             {"dtype": "u8", "data": res["keys"][:, 1].astype(np.uint8), "valid": None}]
    for g in range(5):
        c = api.reduce_dec128_col(res, g, dcols[g]["precision"], dcols[g]["scale"])
        assert c["valid"] is None  # no NULL input: every partial saw a value
        assert c["precision"] == min(38, dcols[g]["precision"] + 10)
        pcols.append(c)
    pcols.append({"dtype": "i64", "valid": None,
                  "data": np.ascontiguousarray(res["aggs"][:, 5]).view(np.int64)})
    for g in range(5):  # each sum's nn: the count half of avg's (sum, count) state
        pcols.append({"dtype": "i64", "data": res["nn"][:, g].astype(np.int64),
                      "valid": None})
    pbatch = api.DeviceBatch(pcols)
    P = 6
    part = api.Partitioner(pbatch, [0, 1], P)
    part.run()
    part.sync()
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    ex = comm.exchange(part)
    try:
        assert ex.total_rows == m
        off = part.row_offsets()
        krf = ex.col_data(0)["data"]
        kls = ex.col_data(1)["data"]
        words = [ex.col_data(2 + g)["data"].tolist() for g in range(5)]
        cnt = ex.col_data(7)["data"]
        nns = [ex.col_data(8 + g)["data"] for g in range(5)]

        # final aggregation per partition; groups must not split across partitions
        final, home = {}, {}
        for p in range(P):
            for i in range(off[p], off[p + 1]):
                k = (int(krf[i]), int(kls[i]))
                assert home.setdefault(k, p) == p, (
                    f"group {k} appears in partitions {home[k]} and {p}")
                acc = final.setdefault(k, {"sum": [0] * 5, "nn": [0] * 5, "count": 0})
                for g in range(5):
                    lo, hi = words[g][i]
                    acc["sum"][g] += lo | (hi << 64)
                    acc["nn"][g] += int(nns[g][i])
                acc["count"] += int(cnt[i])
        assert off[P] == m and sum(v["count"] for v in final.values()) == n  # rows conserved
    finally:
        ex.destroy()
        comm.destroy()
        part.destroy()
        pbatch.free()

    table = pa.table(dict([("rf", rf), ("ls", ls)] + sums))
    direct = table.group_by(["rf", "ls"]).aggregate(
        [(name, "sum") for name, _ in sums] + [(name, "count") for name, _ in sums]
        + [([], "count_all")])
    assert len(final) == direct.num_rows == 6
    for i in range(direct.num_rows):
        got = final[(direct["rf"][i].as_py(), direct["ls"][i].as_py())]
        assert got["count"] == direct["count_all"][i].as_py()
        for g, (name, arr) in enumerate(sums):
            want = _unscaled(direct[f"{name}_sum"][i].as_py(), arr.type.scale)
            assert decagg.to_signed128(got["sum"][g]) == want, f"sum({name}) of group {i}"
            # avg(x)'s partial state is (sum, count): both halves exact; the division and
            # its rounding belong to the final aggregate
            assert got["nn"][g] == direct[f"{name}_count"][i].as_py()
