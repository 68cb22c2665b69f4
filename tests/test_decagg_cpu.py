"""The exact decimal-aggregation model and the plan geometry (no GPU).

decagg.reduce_dec_ref / final_merge_dec are what the GPU tests hold the wide partial-reduce
kernel to, so they are pinned here first: against pyarrow's exact decimal sums, on crafted
wraps past +-2^127, and against each other over arbitrary splits of the rows into
"partials". partial_reduce_plan_geometry needs no device and is swept over every plan
shape."""

import decimal
import itertools

import numpy as np
import pytest

from datafusion_distributed_amd import api, decagg
from oracle import reduce_ref as rr


def col(dtype, data, valid=None, **kw):
    return dict({"dtype": dtype, "data": data, "valid": valid}, **kw)


def dec_col(values, valid=None):
    return col("dec128", decagg.dec_words(values), valid, precision=38, scale=2)


def test_model_matches_pyarrow_decimal_sums():
    import pyarrow as pa

    rng = np.random.default_rng(1701)
    n = 5000
    k = rng.integers(0, 7, n).astype(np.int32)
    unscaled = rng.integers(-10**14, 10**14, n).tolist()
    valid = (rng.random(n) >= 0.2).astype(np.uint8)
    valid[k == 3] = 0  # one group with every input NULL
    arr = pa.array([decimal.Decimal(v).scaleb(-2) if ok else None
                    for v, ok in zip(unscaled, valid)], type=pa.decimal128(15, 2))
    cols = [col("i32", k), api.dec128_col(arr)]
    assert cols[1]["precision"] == 15 and cols[1]["scale"] == 2
    got = decagg.reduce_dec_ref(cols, [0], [(1, "sum_dec128"), (None, "count")])
    direct = pa.table({"k": k, "v": arr}).group_by(["k"]).aggregate(
        [("v", "sum"), ("v", "count")])
    assert direct.schema.field("v_sum").type == pa.decimal128(38, 2)  # sums stay exact
    assert direct.num_rows == len(got) == 7
    for i in range(direct.num_rows):
        e = got[((int(direct["k"][i].as_py()),), 0)]
        want = direct["v_sum"][i].as_py()
        assert e[0]["nn"] == direct["v_count"][i].as_py()
        if want is None:
            assert e[0]["value"] is None and e[0]["nn"] == 0
        else:
            assert e[0]["value"] == int(want.scaleb(2))
        assert e[1]["value"] == int((k == direct["k"][i].as_py()).sum())
    assert got[((3,), 0)][0]["value"] is None


def test_crafted_wraps_past_the_signed_range():
    big = (1 << 127) - 1
    values = [big, big, 5,            # group 0: 2^128 + 3 -> wraps to 3
              -(1 << 127), -1,        # group 1: -2^127 - 1 -> wraps to 2^127 - 1
              big, 1,                 # group 2: 2^127 -> wraps to -2^127
              -7, 7]                  # group 3: 0, not None
    k = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int64)
    exact = {g: sum(v for v, kk in zip(values, k.tolist()) if kk == g) for g in range(4)}
    assert exact[0] > big and exact[1] < -(1 << 127) and exact[2] == 1 << 127  # the premise
    got = decagg.reduce_dec_ref([col("i64", k), dec_col(values)], [0], [(1, "sum_dec128")])
    assert got[((0,), 0)][0]["value"] == 3
    assert got[((1,), 0)][0]["value"] == big
    assert got[((2,), 0)][0]["value"] == -(1 << 127)
    assert got[((3,), 0)][0] == {"op": "sum_dec128", "value": 0, "nn": 2}
    assert decagg.dec_ints(dec_col(values)) == values  # words <-> ints round trip


def _as_partials(cols, key_idx, aggs, pieces):
    """Aggregate each piece of the rows on its own and lay the groups out as partial rows
    in api.partial_reduce's shape."""
    keys, keynull, lo, hi, nn = [], [], [], [], []
    for idx in pieces:
        sub = []
        for c in cols:
            s = dict(c, data=np.ascontiguousarray(np.asarray(c["data"])[idx]))
            if c.get("valid") is not None:
                s["valid"] = np.asarray(c["valid"])[idx]
            sub.append(s)
        for (bits, mask), entries in decagg.reduce_dec_ref(sub, key_idx, aggs).items():
            keys.append(bits)
            keynull.append(mask)
            rlo, rhi, rnn = [], [], []
            for e in entries:
                v = e["value"]
                if e["op"] == "sum_dec128":
                    w = decagg.dec_words([0 if v is None else v])[0]
                    rlo.append(int(w[0]))
                    rhi.append(int(w[1]))
                else:  # count / sum_i64: the i64 bits
                    rlo.append((0 if v is None else v) & ((1 << 64) - 1))
                    rhi.append(0)
                rnn.append(e["nn"])
            lo.append(rlo)
            hi.append(rhi)
            nn.append(rnn)
    na = len(aggs)
    return {"keys": np.array(keys, dtype=np.uint64).reshape(-1, len(key_idx)),
            "keynull": np.array(keynull, dtype=np.uint32),
            "aggs": np.array(lo, dtype=np.uint64).reshape(-1, na).view(np.float64),
            "aggs_hi": np.array(hi, dtype=np.uint64).reshape(-1, na),
            "nn": np.array(nn, dtype=np.uint64).reshape(-1, na)}


@pytest.mark.parametrize("seed", range(4))
def test_final_merge_over_any_split_equals_the_whole(seed):
    rng = np.random.default_rng(1800 + seed)
    n = 1200
    k0 = rng.integers(0, 5, n).astype(np.uint8)
    k1 = rng.integers(-2, 2, n).astype(np.int64)
    k1v = (rng.random(n) >= 0.2).astype(np.uint8)
    # full-range words: sums wrap, which must commute with the split
    words = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    cols = [col("u8", k0), col("i64", k1, k1v),
            col("dec128", words, (rng.random(n) >= 0.3).astype(np.uint8)),
            col("i64", rng.integers(-99, 99, n, dtype=np.int64))]
    aggs = [(2, "sum_dec128"), (None, "count"), (3, "sum_i64"), (2, "sum_dec128")]
    ops = [o for _, o in aggs]
    cuts = np.sort(rng.integers(0, n, int(rng.integers(1, 9))))
    pieces = [p for p in np.split(rng.permutation(n), cuts) if len(p)]
    merged = decagg.final_merge_dec(_as_partials(cols, [0, 1], aggs, pieces), ops)
    whole = decagg.reduce_dec_ref(cols, [0, 1], aggs)
    assert merged.keys() == whole.keys()
    for gid, want in whole.items():
        for ge, we in zip(merged[gid], want):
            assert (ge["op"], ge["value"], ge["nn"]) == (we["op"], we["value"], we["nn"])


def test_final_merge_all_null_group_is_none():
    cols = [col("i64", np.array([1, 1, 2], dtype=np.int64)),
            dec_col([10, 20, 30], np.array([0, 0, 1], dtype=np.uint8))]
    aggs = [(1, "sum_dec128")]
    res = _as_partials(cols, [0], aggs, [np.array([0]), np.array([1, 2])])
    got = decagg.final_merge_dec(res, ["sum_dec128"])
    assert got[((1,), 0)][0] == {"op": "sum_dec128", "value": None, "nn": 0}
    assert got[((2,), 0)][0] == {"op": "sum_dec128", "value": 30, "nn": 1}


# ---------------- plan geometry ----------------

NARROW = [o for o in rr.OPS]
LDS_LIMIT = 163840  # the issue's bound: LDS of one workgroup on gfx950


def _plans():
    """Plans of 1..8 ops: all-decimal, all of one narrow op, and mixed ones."""
    plans = []
    for na in range(1, 9):
        plans.append(["sum_dec128"] * na)
        plans.append(["sum_f64"] * na)
        plans.append([(NARROW + ["sum_dec128"])[(na + i) % 8] for i in range(na)])
        plans.append((["count", "min_i64"] + ["sum_dec128"] * 6)[:na])
    return plans


def test_plan_geometry_every_plan_shape():
    for n_keys, ops, n in itertools.product(range(1, 5), _plans(), (0, 1, 150_001)):
        geo = api.partial_reduce_plan_geometry(n, n_keys, ops)
        ctx = f"n_keys={n_keys} ops={ops} n={n}: {geo}"
        wide = len(ops) > 4 or "sum_dec128" in ops
        assert geo["kernel"] == (1 if wide else 0), ctx
        assert geo["nblocks"] * geo["chunk_rows"] >= n, ctx
        assert geo["probe_limit"] <= geo["table_slots"], ctx
        if geo["kernel"] == 0:
            old = api.partial_reduce_geometry(n)
            assert {k: geo[k] for k in old} == old, ctx
            continue
        slots = geo["table_slots"]
        assert 512 <= slots <= 1024 and slots & (slots - 1) == 0, ctx
        assert geo["lds_bytes"] <= LDS_LIMIT, ctx
        assert geo["block_threads"] % 64 == 0 and geo["block_threads"] <= 1024, ctx
        n_dec = ops.count("sum_dec128")
        per_slot = 8 + 4 + 4 + 8 * n_keys + 12 * len(ops) + 8 * n_dec
        assert geo["lds_bytes"] == slots * per_slot, ctx


def test_plan_geometry_named_plans():
    q1 = ["sum_dec128"] * 5 + ["count"]
    geo = api.partial_reduce_plan_geometry(6_000_000, 2, q1)
    assert geo["lds_bytes"] == 144 * geo["table_slots"]
    worst = api.partial_reduce_plan_geometry(6_000_000, 4, ["sum_dec128"] * 8)
    assert worst["table_slots"] == 512 and worst["lds_bytes"] == 208 * 512


def test_plan_geometry_refusals():
    with pytest.raises(api.DDError) as ei:
        api.partial_reduce_plan_geometry(10, 1, ["count"] * 9)
    assert ei.value.status == 6 and "8 aggregates" in str(ei.value)
    with pytest.raises(api.DDError) as ei:
        api.partial_reduce_plan_geometry(10, 5, ["count"])
    assert ei.value.status == 6


def test_reduce_dec128_col_builds_the_shuffle_column():
    lo = np.array([[5, 7], [0, 1]], dtype=np.uint64)
    res = {"aggs": lo.view(np.float64), "aggs_hi": np.array([[9, 0], [0, 0]], dtype=np.uint64),
           "nn": np.array([[2, 1], [0, 1]], dtype=np.uint64)}
    c = api.reduce_dec128_col(res, 0, 15, 2)
    assert c["dtype"] == "dec128" and c["precision"] == 25 and c["scale"] == 2
    assert c["data"].tolist() == [[5, 9], [0, 0]] and c["valid"].tolist() == [1, 0]
    c = api.reduce_dec128_col(res, 1, 30, 4)
    assert c["precision"] == 38 and c["valid"] is None
    assert c["data"].tolist() == [[7, 0], [1, 0]]
    assert api.AGG_OPS["sum_dec128"] == 7
