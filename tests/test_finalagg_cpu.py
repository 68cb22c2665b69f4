"""The exact model of the final aggregation above the shuffle (no GPU).

finalagg.final_merge_ref is what the GPU tests hold dd_final_merge_run to, so it is pinned
here first: merging partials made from blocks of rows must give what aggregating all rows
at once gives, and what pyarrow's group_by gives. table_slots / home_slot restate the claim
table's arithmetic and are spot-checked against hand-computed values."""

import decimal

import numpy as np
import pytest

from datafusion_distributed_amd import api, decagg, finalagg
from oracle import pyref

ALL_OPS = ["sum_f64", "count", "sum_i64", "min_f64", "max_f64", "min_i64", "max_i64",
           "sum_dec128"]
# a min / max partial without a non-null input holds a value that would win if it were read
POISON = {"min_i64": 1 << 63, "max_i64": (1 << 63) - 1, "min_f64": 0xFFFFFFFFFFFFFFFF,
          "max_f64": 0x7FFFFFFFFFFFFFFF, "sum_i64": 12345, "sum_f64": 0x7FF8000000000000,
          "sum_dec128": (1 << 128) - 1}


def col(dtype, data, valid=None, **kw):
    return dict({"dtype": dtype, "data": data, "valid": valid}, **kw)


def take(cols, idx):
    out = []
    for c in cols:
        s = dict(c, data=np.ascontiguousarray(np.asarray(c["data"])[idx]))
        if c.get("valid") is not None:
            s["valid"] = np.asarray(c["valid"])[idx]
        out.append(s)
    return out


def raw_rows(rng, n):
    """Two nullable keys and one nullable input column per dtype the ops read."""
    k0 = rng.integers(0, 6, n).astype(np.int32)
    k1 = rng.choice(np.array([0.0, -0.0, 1.5, np.nan]), n)
    f = rng.normal(size=n) * 1e3
    i = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    words = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    fv = (rng.random(n) >= 0.3).astype(np.uint8)
    fv[k0 == 2] = 0  # every f64 input of these groups is NULL
    cols = [col("i32", k0, (rng.random(n) >= 0.1).astype(np.uint8)), col("f64", k1),
            col("f64", f, fv), col("i64", i, (rng.random(n) >= 0.3).astype(np.uint8)),
            col("dec128", words, (rng.random(n) >= 0.3).astype(np.uint8))]
    aggs = [(2, "sum_f64"), (None, "count"), (3, "sum_i64"), (2, "min_f64"), (2, "max_f64"),
            (3, "min_i64"), (3, "max_i64"), (4, "sum_dec128")]
    return cols, [0, 1], aggs


@pytest.mark.parametrize("seed", range(3))
def test_merge_of_block_partials_equals_the_whole(seed):
    rng = np.random.default_rng(2100 + seed)
    n = 3000
    cols, key_idx, aggs = raw_rows(rng, n)
    cuts = np.sort(rng.integers(0, n, 6))
    blocks = np.split(np.arange(n), cuts)
    partials = [decagg.reduce_dec_ref(take(cols, b), key_idx, aggs) for b in blocks]
    res = finalagg.groups_as_partials(partials, 2, ALL_OPS, poison=POISON)
    assert (res["nn"] == 0).any()  # the nn == 0 rule is exercised
    pcols, pkeys, paggs = finalagg.partial_state_cols(res, ["i32", "f64"], ALL_OPS)
    got = finalagg.final_merge_ref(pcols, pkeys, paggs)
    want = decagg.reduce_dec_ref(cols, key_idx, aggs)
    assert len(got) == 1 and got[0].keys() == want.keys()
    for gid, went in want.items():
        for ge, we in zip(got[0][gid], went):
            assert ge["op"] == we["op"] and ge["nn"] == we["nn"], (gid, ge, we)
            if we["op"] != "sum_f64" or we["value"] is None:
                assert ge["value"] == we["value"], (gid, ge, we)
            else:
                # the partial sums are rounded once each, the two fsums once each
                bound = (len(blocks) + 2) * 2.0 ** -53 * we["abs_sum"]
                assert abs(ge["value"] - we["value"]) <= bound, (gid, ge, we)
    assert any(e[0]["value"] is None for e in want.values())  # an all-NULL group survived


def test_layout_groups_stay_inside_their_partition():
    """The same key in two partitions gives two groups; segments of one partition merge."""
    k = np.array([7, 7, 8, 7, 8, 8], dtype=np.int64)
    c = np.array([1, 2, 4, 8, 16, 32], dtype=np.int64)
    cols = [col("i64", k), col("i64", c)]
    got = finalagg.final_merge_ref(cols, [0], [(1, "count", None)], seg_offsets=[0, 2, 3, 3, 6],
                                   seg_part=[0, 1, 1, 0], n_parts=3)
    assert [{g[0][0]: e[0]["value"] for g, e in p.items()} for p in got] == [
        {7: 1 + 2 + 8, 8: 16 + 32}, {8: 4}, {}]
    with pytest.raises(ValueError, match="segment layout"):
        finalagg.final_merge_ref(cols, [0], [(1, "count", None)], [0, 2, 5], [0, 1], 2)
    with pytest.raises(ValueError, match="segment layout"):
        finalagg.final_merge_ref(cols, [0], [(1, "count", None)], [0, 2, 6], [0, 2], 2)


def test_model_matches_pyarrow_group_by():
    import pyarrow as pa

    rng = np.random.default_rng(2200)
    n = 4000
    k = rng.integers(0, 9, n).astype(np.int32)
    f = rng.integers(-4000, 4000, n) / 8.0  # sums of these are exact in any order
    i = rng.integers(-10**12, 10**12, n, dtype=np.int64)
    unscaled = rng.integers(-10**14, 10**14, n).tolist()
    ok = rng.random(n) >= 0.25
    ok[k == 4] = False  # one group with every input NULL
    okv = ok.astype(np.uint8)
    dec = pa.array([decimal.Decimal(v).scaleb(-2) if o else None
                    for v, o in zip(unscaled, ok)], type=pa.decimal128(15, 2))
    cols = [col("i32", k), col("f64", f, okv), col("i64", i, okv), api.dec128_col(dec)]
    aggs = [(1, "sum_f64"), (None, "count"), (2, "sum_i64"), (1, "min_f64"), (1, "max_f64"),
            (2, "min_i64"), (2, "max_i64"), (3, "sum_dec128")]
    blocks = np.array_split(np.arange(n), 7)
    partials = [decagg.reduce_dec_ref(take(cols, b), [0], aggs) for b in blocks]
    res = finalagg.groups_as_partials(partials, 1, ALL_OPS, poison=POISON)
    pcols, pkeys, paggs = finalagg.partial_state_cols(res, ["i32"], ALL_OPS)
    # the partials arrive as two "producers" of one partition each holding every group
    m = len(res["keynull"])
    got = finalagg.final_merge_ref(pcols, pkeys, paggs, [0, m // 3, m], [0, 0], 1)[0]

    table = pa.table({"k": k, "f": pa.array(f, mask=~ok), "i": pa.array(i, mask=~ok), "d": dec})
    direct = table.group_by(["k"]).aggregate(
        [("f", "sum"), ("f", "min"), ("f", "max"), ("i", "sum"), ("i", "min"), ("i", "max"),
         ("d", "sum"), ("f", "count"), ([], "count_all")])
    assert direct.num_rows == len(got) == 9

    def f64_bits(x):
        return None if x is None else int(np.float64(x).view(np.uint64))

    for r in range(direct.num_rows):
        e = got[((int(direct["k"][r].as_py()),), 0)]
        row = {name: direct[name][r].as_py() for name in direct.column_names}
        assert e[0]["value"] == row["f_sum"]
        assert e[1]["value"] == e[1]["nn"] == row["count_all"]
        assert e[2]["value"] == row["i_sum"]
        assert e[3]["value"] == f64_bits(row["f_min"])
        assert e[4]["value"] == f64_bits(row["f_max"])
        assert e[5]["value"] == row["i_min"] and e[6]["value"] == row["i_max"]
        assert e[7]["value"] == (None if row["d_sum"] is None else int(row["d_sum"].scaleb(2)))
        assert all(e[g]["nn"] == row["f_count"] for g in (0, 2, 3, 4, 5, 6, 7))
    assert got[((4,), 0)][0]["value"] is None


def test_table_slots_and_home_slot():
    assert [finalagg.table_slots(r) for r in (0, 1, 32, 33, 64, 256, 257, 20_000)] == [
        64, 64, 64, 128, 128, 512, 1024, 65536]
    for rows in (1, 31, 100, 5000, 123_457):
        slots = finalagg.table_slots(rows)
        assert slots & (slots - 1) == 0 and 2 * rows <= slots and (slots == 64 or slots < 4 * rows)
    # hand-computed: mix64(0) == 0; mix64(1) is splitmix64's finaliser of 1
    assert finalagg.home_slot(0, 64) == 0
    assert pyref.mix64_scalar(1) == 0x5692161D100B05E5
    assert finalagg.home_slot(1, 64) == 0x5692161D100B05E5 >> 58 == 21
    assert finalagg.home_slot(1, 512) == 0x5692161D100B05E5 >> 55
    h = pyref.hash_cols([col("i64", np.arange(1000, dtype=np.int64))], 1000)
    for slots in (64, 512, 1 << 20):
        vec = finalagg.home_slot(h, slots)
        assert vec.min() >= 0 and vec.max() < slots
        assert vec.tolist() == [finalagg.home_slot(int(x), slots) for x in h.tolist()]
    # rows of one shuffled partition share h % P; their home slots still spread
    mine = h[h % np.uint64(8) == 3]
    assert len(np.unique(finalagg.home_slot(mine, 64))) > 48
    with pytest.raises(AssertionError):
        finalagg.home_slot(1, 100)
