"""GPU final aggregation above the shuffle vs its exact model (marked gpu).

One checker, check_final, runs dd_final_merge_run through api.final_merge and holds it to
finalagg.final_merge_ref: group_offsets monotone from 0 to n_groups, exactly one output row
per (partition, group) and no other, keys / keynull / nn / integer and decimal values /
min-max bit patterns exact, float sums within n * 2^-52 * sum|x| over the n merged addends
(the bound tests/test_gpu_reduce_parity.py uses). Inputs are partial STATES: most cases
draw them directly (random_states), since to the merge they are just columns."""

import ctypes
import decimal
import math

import numpy as np
import pytest

from datafusion_distributed_amd import api, decagg, finalagg
from oracle import pyref

pytestmark = pytest.mark.gpu

ALL_OPS = ["sum_f64", "count", "sum_i64", "min_f64", "max_f64", "min_i64", "max_i64",
           "sum_dec128"]
I64 = np.iinfo(np.int64)
NEG_QNAN = 0xFFF8000000000000
POS_QNAN = 0x7FF8000000000000
PAYLOAD_NAN = 0x7FF8000000000ABC
NEG_PAYLOAD_NAN = 0xFFF8000000000DEF
NEG_ZERO = 0x8000000000000000
SPECIAL_F64 = np.array(
    [POS_QNAN, NEG_QNAN, PAYLOAD_NAN, NEG_PAYLOAD_NAN, 0x7FF0000000000000, 0xFFF0000000000000,
     0, NEG_ZERO, 1, 0x8000000000000001], dtype=np.uint64).view(np.float64)
INVALID, UNSUPPORTED = 1, 6


def col(dtype, data, valid=None, **kw):
    return dict({"dtype": dtype, "data": data, "valid": valid}, **kw)


def random_states(rng, n, ops, first_col):
    """State and nn columns of n partial rows for `ops`, as (cols, aggs) whose column
    indices start at first_col. Values span the full range of their type (integer and
    decimal sums wrap, min / max see the special floats); nn is 0 for about a quarter of
    the partials, and those hold values like any other, which the merge must not read."""
    cols, aggs = [], []
    for op in ops:
        sc = first_col + len(cols)
        if op == "sum_f64":
            cols.append(col("f64", rng.normal(size=n) * 1e3))
        elif op == "count":
            cols.append(col("i64", rng.integers(1, 6, n, dtype=np.int64)))
            aggs.append((sc, op, None))
            continue
        elif op in ("min_f64", "max_f64"):
            v = rng.normal(size=n)
            pick = rng.random(n) < 0.3
            v[pick] = rng.choice(SPECIAL_F64, int(pick.sum()))
            cols.append(col("f64", v))
        elif op == "sum_dec128":
            cols.append(col("dec128", rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)))
        else:
            cols.append(col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64,
                                                endpoint=True)))
        cols.append(col("i64", rng.integers(0, 4, n, dtype=np.int64)))
        aggs.append((sc, op, sc + 1))
    return cols, aggs


def compare(res, want, ops, nk):
    """Hold api.final_merge's result to the model's [{gid: entries} per partition]."""
    off = res["group_offsets"]
    n_groups = len(res["keynull"])
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == n_groups
    assert len(off) == len(want) + 1
    assert res["keys"].shape == (n_groups, nk) and res["aggs"].shape == (n_groups, len(ops))
    lo = np.ascontiguousarray(res["aggs"]).view(np.uint64)
    keys = res["keys"].tolist()
    keynull = res["keynull"].tolist()
    for p, wp in enumerate(want):
        rows = {}
        for r in range(off[p], off[p + 1]):  # sorted by identity: a dict keyed by it
            gid = (tuple(keys[r]), keynull[r])
            assert gid not in rows, f"partition {p}: group {gid} came out twice"
            rows[gid] = r
        missing, invented = wp.keys() - rows.keys(), rows.keys() - wp.keys()
        assert not missing and not invented, (
            f"partition {p}: missing {sorted(missing)[:5]} invented {sorted(invented)[:5]}")
        for gid, went in wp.items():
            r = rows[gid]
            for g, we in enumerate(went):
                ctx = f"partition {p} group {gid} agg {g} {we['op']}: want {we}"
                assert int(res["nn"][r, g]) == we["nn"], ctx
                bits, hi = int(lo[r, g]), int(res["aggs_hi"][r, g])
                if we["op"] != "sum_dec128":
                    assert hi == 0, ctx
                wv = we["value"]
                if wv is None:
                    assert we["nn"] == 0, ctx  # SQL NULL: the value slot is unspecified
                elif we["op"] == "sum_dec128":
                    assert decagg.to_signed128(bits | (hi << 64)) == wv, f"{ctx} got {bits} {hi}"
                elif we["op"] in ("min_f64", "max_f64"):
                    assert bits == wv, f"{ctx} got {bits:#x}"
                elif we["op"] == "sum_f64":
                    gv = float(np.uint64(bits).view(np.float64))
                    if not math.isfinite(wv):
                        assert gv == wv or (gv != gv and wv != wv), f"{ctx} got {gv}"
                    else:
                        if "terms" in we:  # the model merged these partial sums
                            cnt = len(we["terms"])
                            mag = math.fsum(abs(x) for x in we["terms"])
                        else:  # the model summed the raw inputs
                            cnt, mag = we["n_nonnull"], we["abs_sum"]
                        bound = cnt * 2.0 ** -52 * mag
                        assert abs(gv - wv) <= bound, f"{ctx} err {abs(gv - wv)} bound {bound}"
                else:
                    assert pyref.M64 & wv == bits, f"{ctx} got {bits}"


def check_final(cols, key_idx, aggs, **layout):
    batch = api.DeviceBatch(cols)
    try:
        res = api.final_merge(batch, key_idx, aggs, **layout)
    finally:
        batch.free()
    want = finalagg.final_merge_ref(cols, key_idx, aggs, **layout)
    compare(res, want, [op for _, op, _ in aggs], len(key_idx))
    return res, want


def layout(seg_offsets, seg_part, n_parts):
    return {"seg_offsets": np.asarray(seg_offsets, dtype=np.int64),
            "seg_part": np.asarray(seg_part, dtype=np.int32), "n_parts": n_parts}


# ---------------- sizes and table shapes ----------------

@pytest.mark.parametrize("n", [0, 1])
def test_zero_rows_and_one_row(n):
    rng = np.random.default_rng(3000 + n)
    st, aggs = random_states(rng, n, ALL_OPS, 1)
    res, _ = check_final([col("i64", np.arange(n, dtype=np.int64))] + st, [0], aggs)
    assert len(res["keynull"]) == n and res["group_offsets"].tolist() == [0, n]


def test_empty_partitions_own_empty_regions():
    """n_parts = 5, three of them without a row (one named by an empty segment, two by no
    segment at all)."""
    rng = np.random.default_rng(3002)
    n = 700
    st, aggs = random_states(rng, n, ["count", "sum_i64", "min_f64"], 1)
    lay = layout([0, 300, 300, 700], [1, 2, 4], 5)
    k = rng.integers(0, 40, n)
    res, want = check_final([col("i64", k)] + st, [0], aggs, **lay)
    off = res["group_offsets"]
    assert [len(w) for w in want] == [0, len(np.unique(k[:300])), 0, 0, len(np.unique(k[300:]))]
    assert off[0] == off[1] and off[2] == off[3] == off[4]


def test_one_hot_group():
    """5 000 rows of one group: every atomic of every op lands on one address."""
    rng = np.random.default_rng(3003)
    n = 5000
    st, aggs = random_states(rng, n, ALL_OPS, 1)
    res, _ = check_final([col("i32", np.full(n, -5, dtype=np.int32))] + st, [0], aggs)
    assert len(res["keynull"]) == 1


def test_all_distinct_keys():
    """20 000 distinct i64 keys in one partition: as many claims as rows, 64 scan tiles.
    The region has table_slots(20 000) = 65 536 slots (load 0.31; the rule
    max(64, next_pow2(2 * rows)) keeps every load at or below 0.5)."""
    rng = np.random.default_rng(3004)
    n = 20_000
    assert finalagg.table_slots(n) == 65536
    keys = rng.permutation(np.arange(-n // 2, n // 2, dtype=np.int64) * 7919)
    st, aggs = random_states(rng, n, ["count", "sum_dec128"], 1)
    res, _ = check_final([col("i64", keys)] + st, [0], aggs)
    assert len(res["keynull"]) == n


def test_scan_past_one_round_of_tile_sums():
    """600 000 rows in one partition: a 2^21-slot table is 2048 scan tiles, two rounds of
    the block that scans the tile sums."""
    rng = np.random.default_rng(3005)
    n = 600_000
    assert finalagg.table_slots(n) // 1024 > 1024
    st, aggs = random_states(rng, n, ["count", "sum_i64"], 1)
    res, _ = check_final([col("i64", rng.integers(0, 1000, n))] + st, [0], aggs)
    assert len(res["keynull"]) == 1000


def test_more_segments_than_the_staged_search_holds():
    """1 500 segments: past the 1 024 whose offsets the claim kernel stages in LDS, so
    the segment search reads them from memory. Many segments are empty."""
    rng = np.random.default_rng(3006)
    n, S, P = 4000, 1500, 7
    off = np.concatenate([[0], np.sort(rng.integers(0, n + 1, S - 1)), [n]])
    st, aggs = random_states(rng, n, ["count", "max_i64"], 1)
    check_final([col("i64", rng.integers(0, 25, n))] + st, [0], aggs,
                **layout(off, np.arange(S) % P, P))


def test_long_probe_chain():
    """256 rows in one partition (512 slots) with >= 200 distinct keys that share one home
    slot: the probe walks a run of up to 200 slots and wraps inside the region."""
    n, slots = 256, finalagg.table_slots(256)
    assert slots == 512
    cand = np.arange(100_000, dtype=np.int64)
    home = finalagg.home_slot(pyref.hash_cols([col("i64", cand)], len(cand)), slots)
    counts = np.bincount(home, minlength=slots)
    # the fullest home slot among those whose run must wrap past the end of the region
    late = np.arange(slots) >= slots - 150
    target = int(np.argmax(np.where(late, counts, 0)))
    hit = cand[home == target]
    assert len(hit) >= 200, f"only {len(hit)} of 10^5 keys home at slot {target}"
    rng = np.random.default_rng(3007)
    keys = np.concatenate([hit[:200], rng.choice(hit[:200], n - 200)])  # 56 repeats
    keys = rng.permutation(keys)
    st, aggs = random_states(rng, n, ["count", "sum_i64", "min_i64"], 1)
    res, _ = check_final([col("i64", keys)] + st, [0], aggs)
    assert len(res["keynull"]) == 200


# ---------------- group identity ----------------

def test_null_key_and_zero_key_stay_apart():
    rng = np.random.default_rng(3010)
    n = 600
    k = rng.integers(0, 3, n).astype(np.int32)
    valid = (rng.random(n) >= 0.4).astype(np.uint8)
    assert ((k == 0) & (valid == 1)).any() and (valid == 0).any()
    st, aggs = random_states(rng, n, ["count", "sum_i64"], 1)
    res, want = check_final([col("i32", k, valid)] + st, [0], aggs)
    assert ((0,), 1) in want[0] and ((0,), 0) in want[0] and len(want[0]) == 4


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_float_keys_canonicalise(dtype):
    """-0.0 and +0.0 are one group, every NaN payload is one group."""
    rng = np.random.default_rng(3011)
    n = 500
    if dtype == "f64":
        pool = np.array([0, NEG_ZERO, POS_QNAN, PAYLOAD_NAN, NEG_QNAN, 0x3FF8000000000000],
                        dtype=np.uint64).view(np.float64)
    else:
        pool = np.array([0, 0x80000000, 0x7FC00000, 0x7FC00ABC, 0xFFC00000, 0x3FC00000],
                        dtype=np.uint32).view(np.float32)
    st, aggs = random_states(rng, n, ["count", "max_f64"], 1)
    res, _ = check_final([col(dtype, rng.choice(pool, n))] + st, [0], aggs)
    assert len(res["keynull"]) == 3  # zero, NaN, 1.5


def test_four_keys_with_mixed_null_masks():
    """The widest key plan; every key nullable and drawn from two values, so groups differ
    by mask alone (a NULL component has bits 0, like a valid 0)."""
    rng = np.random.default_rng(3012)
    n = 3000
    kcols = [col("u8", rng.integers(0, 2, n).astype(np.uint8), (rng.random(n) >= 0.3).astype(np.uint8)),
             col("i16", rng.integers(0, 2, n).astype(np.int16), (rng.random(n) >= 0.3).astype(np.uint8)),
             col("i64", rng.integers(0, 2, n), (rng.random(n) >= 0.3).astype(np.uint8)),
             col("bool", rng.integers(0, 2, n).astype(np.uint8), (rng.random(n) >= 0.3).astype(np.uint8))]
    st, aggs = random_states(rng, n, ["count", "sum_f64", "sum_dec128"], 4)
    res, want = check_final(kcols + st, [0, 1, 2, 3], aggs)
    assert len(want[0]) == 3 ** 4
    assert len(set(res["keynull"].tolist())) == 16


def test_same_key_in_two_partitions_gives_two_groups():
    k = np.array([7, 7, 9, 7, 7, 9, 9], dtype=np.int64)
    c = np.array([1, 2, 4, 8, 16, 32, 64], dtype=np.int64)
    res, _ = check_final([col("i64", k), col("i64", c)], [0], [(1, "count", None)],
                         **layout([0, 3, 7], [0, 1], 2))
    got = {(int(p), int(res["keys"][r, 0])): int(res["aggs"][r, 0].view(np.int64))
           for p in range(2) for r in range(res["group_offsets"][p], res["group_offsets"][p + 1])}
    assert got == {(0, 7): 3, (0, 9): 4, (1, 7): 24, (1, 9): 96}


# ---------------- merge rules ----------------

def test_poisoned_partials_with_nn_zero_never_win():
    """min / max partials without a non-null input hold the value that would win."""
    k = np.array([0, 0, 0, 1, 1, 1], dtype=np.int64)
    nn = np.array([2, 0, 1, 0, 3, 0], dtype=np.int64)
    i_min = np.array([5, I64.min, 9, I64.min, -3, I64.min], dtype=np.int64)
    i_max = np.array([5, I64.max, 9, I64.max, -3, I64.max], dtype=np.int64)
    f_min = np.array([0x3FF0000000000000, 0xFFFFFFFFFFFFFFFF, 0x4000000000000000,
                      0xFFFFFFFFFFFFFFFF, NEG_ZERO, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    f_max = np.array([0x3FF0000000000000, 0x7FFFFFFFFFFFFFFF, 0x4000000000000000,
                      0x7FFFFFFFFFFFFFFF, NEG_ZERO, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    cols = [col("i64", k), col("i64", nn), col("i64", i_min), col("i64", i_max),
            col("f64", f_min.view(np.float64)), col("f64", f_max.view(np.float64))]
    aggs = [(2, "min_i64", 1), (3, "max_i64", 1), (4, "min_f64", 1), (5, "max_f64", 1)]
    _, want = check_final(cols, [0], aggs)
    assert [e["value"] for e in want[0][((0,), 0)]] == [5, 9, 0x3FF0000000000000,
                                                        0x4000000000000000]
    assert [e["value"] for e in want[0][((1,), 0)]] == [-3, -3, NEG_ZERO, NEG_ZERO]


def test_all_null_group_reports_nn_zero():
    rng = np.random.default_rng(3020)
    n = 400
    k = rng.integers(0, 5, n)
    ops = ["sum_f64", "sum_i64", "min_f64", "max_i64", "sum_dec128", "count"]
    st, aggs = random_states(rng, n, ops, 1)
    for _, op, nc in aggs:
        if nc is not None:
            st[nc - 1]["data"][k == 3] = 0  # group 3: no partial saw a non-null input
    res, want = check_final([col("i64", k)] + st, [0], aggs)
    r = int(np.flatnonzero(res["keys"][:, 0] == 3)[0])
    assert res["nn"][r].tolist()[:5] == [0] * 5 and res["nn"][r, 5] > 0
    assert all(e["value"] is None for e in want[0][((3,), 0)][:5])


def test_count_merges_counts_and_reports_them_as_nn():
    rng = np.random.default_rng(3021)
    n = 2000
    k = rng.integers(0, 30, n)
    c = rng.integers(0, 1 << 40, n, dtype=np.int64)  # a partial count of 0 adds nothing
    res, _ = check_final([col("i64", k), col("i64", c)], [0], [(1, "count", None)])
    got = np.ascontiguousarray(res["aggs"][:, 0]).view(np.int64)
    assert (res["nn"][:, 0].astype(np.int64) == got).all()
    assert got.sum() == c.sum()


def test_decimal_carries_and_wraps():
    big = (1 << 127) - 1
    m64 = (1 << 64) - 1
    groups = {
        0: [m64, 1, m64, m64],           # low halves cross 2^64 three times
        1: [big, big, 5],                # 2^128 + 3 wraps to 3
        2: [-(1 << 127), -1],            # wraps to 2^127 - 1
        3: [-1, -1, -(1 << 64), 7],      # negative values: high halves of all ones
        4: [big, 1],                     # 2^127 wraps to -2^127
        5: [-7, 7],                      # 0, not NULL
    }
    k = np.array([g for g, vs in groups.items() for _ in vs], dtype=np.int64)
    values = [v for vs in groups.values() for v in vs]
    cols = [col("i64", k), col("dec128", decagg.dec_words(values)),
            col("i64", np.ones(len(k), dtype=np.int64))]
    _, want = check_final(cols, [0], [(1, "sum_dec128", 2)])
    exact = {g: decagg.to_signed128(sum(vs)) for g, vs in groups.items()}
    assert exact[1] == 3 and exact[2] == big and exact[4] == -(1 << 127) and exact[5] == 0
    assert {g[0][0]: e[0]["value"] for g, e in want[0].items()} == exact
    # and at scale: 3 000 full-range words over 4 groups, every add may carry
    rng = np.random.default_rng(3022)
    st, aggs = random_states(rng, 3000, ["sum_dec128"], 1)
    check_final([col("i64", rng.integers(0, 4, 3000))] + st, [0], aggs)


def test_sum_i64_wraps():
    k = np.array([0, 0, 0, 1, 1], dtype=np.int64)
    v = np.array([I64.max, I64.max, 2, I64.min, -1], dtype=np.int64)
    cols = [col("i64", k), col("i64", v), col("i64", np.ones(5, dtype=np.int64))]
    _, want = check_final(cols, [0], [(1, "sum_i64", 2)])
    assert want[0][((0,), 0)][0]["value"] == 0  # 2^64 wraps to 0
    assert want[0][((1,), 0)][0]["value"] == I64.max


def test_float_min_max_follow_total_order():
    """Sign-set NaN < -inf < -0.0 < +0.0 < +inf < sign-clear NaN, payloads preserved."""
    sets = [
        ([POS_QNAN, PAYLOAD_NAN, 0x7FF0000000000000], 0x7FF0000000000000, PAYLOAD_NAN),
        ([NEG_QNAN, NEG_PAYLOAD_NAN, 0xFFF0000000000000], NEG_PAYLOAD_NAN, 0xFFF0000000000000),
        ([0, NEG_ZERO], NEG_ZERO, 0),
        ([NEG_ZERO, 0x8000000000000001, NEG_QNAN, 1, PAYLOAD_NAN], NEG_QNAN, PAYLOAD_NAN),
    ]
    k = np.array([g for g, (b, _, _) in enumerate(sets) for _ in b], dtype=np.int64)
    bits = np.array([x for b, _, _ in sets for x in b], dtype=np.uint64)
    cols = [col("i64", k), col("f64", bits.view(np.float64)),
            col("i64", np.ones(len(k), dtype=np.int64))]
    _, want = check_final(cols, [0], [(1, "min_f64", 2), (1, "max_f64", 2)])
    for g, (_, lo, hi) in enumerate(sets):
        assert [e["value"] for e in want[0][((g,), 0)]] == [lo, hi]


def test_eight_aggregates_over_many_groups():
    rng = np.random.default_rng(3023)
    n = 6000
    kcols = [col("i32", rng.integers(0, 40, n).astype(np.int32)),
             col("f64", rng.choice(np.array([0.0, -0.0, 2.5, np.nan]), n))]
    st, aggs = random_states(rng, n, ALL_OPS, 2)
    res, _ = check_final(kcols + st, [0, 1], aggs, **layout([0, 2500, 6000], [1, 0], 2))
    assert len(res["keynull"]) == 2 * 40 * 3


# ---------------- layouts from the shuffle ----------------

def test_two_producers_of_four_partitions():
    """Two Partitioner outputs (P = 4) concatenated producer-major: S = 8, seg_part = s % 4.
    A group present in both producers comes out once, in its partition."""
    rng = np.random.default_rng(3030)
    P = 4
    ops = ["count", "sum_i64", "min_f64", "sum_dec128"]
    outs, offs = [], []
    for n in (3000, 2500):
        st, aggs = random_states(rng, n, ops, 1)
        cols = [col("i64", rng.integers(0, 40, n), (rng.random(n) >= 0.1).astype(np.uint8))] + st
        batch = api.DeviceBatch(cols)
        part = api.Partitioner(batch, [0], P)
        try:
            part.run()
            part.sync()
            off = part.row_offsets()
            out = [part.col_out(i) for i in range(len(cols))]
            # the partitioner's own output, merged where it lies: one segment per partition
            view, lay = api.partitioned_batch(part)
            assert lay["seg_part"].tolist() == list(range(P)) and lay["n_parts"] == P
            res = api.final_merge(view, [0], aggs, **lay)
        finally:
            part.destroy()
            batch.free()
        host = [col(c["dtype"], o["data"], o.get("valid")) for c, o in zip(cols, out)]
        compare(res, finalagg.final_merge_ref(host, [0], aggs, **lay), ops, 1)
        outs.append(host)
        offs.append(off)
    both = []
    for a, b in zip(*outs):
        valid = None if a["valid"] is None else np.concatenate([a["valid"], b["valid"]])
        both.append(col(a["dtype"], np.concatenate([a["data"], b["data"]]), valid))
    seg_offsets = np.concatenate([offs[0], offs[0][-1] + offs[1][1:]])
    lay = layout(seg_offsets, np.arange(2 * P) % P, P)
    res, want = check_final(both, [0], aggs, **lay)
    assert sum(len(w) for w in want) == 41  # 40 keys and NULL, each in exactly one partition
    assert len(res["keynull"]) == 41


def _dec_array(pa, unscaled, typ):
    v = np.ascontiguousarray(unscaled, dtype=np.int64)
    words = np.ascontiguousarray(np.stack([v, v >> 63], axis=1))
    return pa.Array.from_buffers(typ, len(v), [None, pa.py_buffer(words)])


def test_q1_decimal_pipeline_ends_on_the_device(monkeypatch):
    """tests/test_gpu_q1_decimal_pipeline.py with the final aggregate on the GPU: partial
    reduce -> repartition of the partials -> exchange -> api.final_merge over the exchanged
    window where it lies, held exactly to pyarrow's direct decimal group-by."""
    import pyarrow as pa
    import pyarrow.compute as pc

    rng = np.random.default_rng(4747)
    n = 200_000
    d152 = pa.decimal128(15, 2)
    rf = rng.integers(0, 3, n).astype(np.uint8)
    ls = rng.integers(0, 2, n).astype(np.uint8)
    qty = _dec_array(pa, rng.integers(100, 5001, n), d152)
    price = _dec_array(pa, rng.integers(90_000, 10_500_000, n), d152)
    disc = _dec_array(pa, rng.integers(0, 11, n), d152)
    tax = _dec_array(pa, rng.integers(0, 9, n), d152)
    one = pa.scalar(decimal.Decimal(1), pa.decimal128(1, 0))
    d32 = pa.decimal128(3, 2)
    disc_price = pc.multiply(price, pc.cast(pc.subtract(one, disc), d32))
    charge = pc.multiply(disc_price, pc.cast(pc.add(one, tax), d32))
    sums = [("qty", qty), ("price", price), ("disc_price", disc_price), ("charge", charge),
            ("disc", disc)]

    dcols = [api.dec128_col(a) for _, a in sums]
    batch = api.DeviceBatch([col("u8", rf), col("u8", ls)] + dcols)
    ops = ["sum_dec128"] * 5 + ["count"]
    try:
        res = api.partial_reduce(batch, [0, 1], [(2 + i, "sum_dec128") for i in range(5)]
                                 + [(None, "count")])
    finally:
        batch.free()
    m = len(res["keynull"])
    pcols, pkeys, paggs = finalagg.partial_state_cols(res, ["u8", "u8"], ops)
    pbatch = api.DeviceBatch(pcols)
    P = 6
    part = api.Partitioner(pbatch, pkeys, P)
    part.run()
    part.sync()
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    ex = comm.exchange(part)
    try:
        assert ex.total_rows == m

        def no_fetch(*a, **k):
            raise AssertionError("a column of the exchanged window was fetched to the host")

        monkeypatch.setattr(api.Exchanged, "col_data", no_fetch)
        monkeypatch.setattr(api.Exchanged, "col_validity", no_fetch)
        view, lay = api.exchanged_batch(ex)
        assert lay["n_parts"] == P and len(lay["seg_part"]) == P
        assert lay["seg_offsets"].tolist() == part.row_offsets().tolist()
        final = api.final_merge(view, pkeys, paggs, **lay)
    finally:
        ex.destroy()
        comm.destroy()
        part.destroy()
        pbatch.free()

    table = pa.table(dict([("rf", rf), ("ls", ls)] + sums))
    direct = table.group_by(["rf", "ls"]).aggregate(
        [(name, "sum") for name, _ in sums] + [(name, "count") for name, _ in sums]
        + [([], "count_all")])
    off = final["group_offsets"]
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(final["keynull"])
    assert len(final["keynull"]) == direct.num_rows == 6  # no group split across partitions
    assert (final["keynull"] == 0).all()
    lo = np.ascontiguousarray(final["aggs"]).view(np.uint64)
    row = {(int(a), int(b)): r for r, (a, b) in enumerate(final["keys"].tolist())}
    assert len(row) == 6
    for i in range(direct.num_rows):
        r = row[(direct["rf"][i].as_py(), direct["ls"][i].as_py())]
        assert int(lo[r, 5]) == int(final["nn"][r, 5]) == direct["count_all"][i].as_py()
        for g, (name, arr) in enumerate(sums):
            want = int(direct[f"{name}_sum"][i].as_py().scaleb(arr.type.scale))
            got = decagg.to_signed128(int(lo[r, g]) | (int(final["aggs_hi"][r, g]) << 64))
            assert got == want, f"sum({name}) of group {i}"
            assert int(final["nn"][r, g]) == direct[f"{name}_count"][i].as_py()


def test_partial_reduce_then_final_merge_equals_the_whole():
    """50 000 random rows in 300 groups: api.partial_reduce, its partials laid out as
    columns, api.final_merge with n_parts = 1 -> decagg.reduce_dec_ref of the raw rows."""
    rng = np.random.default_rng(3040)
    n = 50_000
    k0 = rng.integers(0, 100, n).astype(np.int32)
    k1 = rng.integers(0, 3, n).astype(np.uint8)
    cols = [col("i32", k0, (rng.random(n) >= 0.05).astype(np.uint8)), col("u8", k1),
            col("f64", rng.normal(size=n) * 1e3, (rng.random(n) >= 0.2).astype(np.uint8)),
            col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64),
                (rng.random(n) >= 0.2).astype(np.uint8)),
            col("dec128", rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64),
                (rng.random(n) >= 0.2).astype(np.uint8))]
    aggs = [(2, "sum_f64"), (None, "count"), (3, "sum_i64"), (2, "min_f64"), (2, "max_f64"),
            (3, "min_i64"), (3, "max_i64"), (4, "sum_dec128")]
    batch = api.DeviceBatch(cols)
    try:
        partial = api.partial_reduce(batch, [0, 1], aggs)
    finally:
        batch.free()
    pcols, pkeys, paggs = finalagg.partial_state_cols(partial, ["i32", "u8"], ALL_OPS)
    pbatch = api.DeviceBatch(pcols)
    try:
        res = api.final_merge(pbatch, pkeys, paggs)
    finally:
        pbatch.free()
    want = decagg.reduce_dec_ref(cols, [0, 1], aggs)
    assert len(want) == 303 == len(res["keynull"])  # 101 x 3: NULL is a key value too
    compare(res, [want], ALL_OPS, 2)  # sum_f64: the any-order bound over the raw addends


# ---------------- refusals ----------------

def _small():
    n = 8
    return [col("i64", np.arange(n, dtype=np.int64)),                       # 0
            col("i64", np.ones(n, dtype=np.int64)),                         # 1
            col("f64", np.ones(n)),                                         # 2
            col("dec128", np.zeros((n, 2), dtype=np.uint64)),               # 3
            col("dict32", np.zeros(n, dtype=np.int32),
                dict_bytes=np.frombuffer(b"ab", dtype=np.uint8),
                dict_offsets=np.array([0, 1, 2], dtype=np.int32)),          # 4
            col("utf8", np.frombuffer(b"x" * n, dtype=np.uint8),
                offsets=np.arange(n + 1, dtype=np.int32)),                  # 5
            col("i32", np.zeros(n, dtype=np.int32))]                        # 6


REFUSALS = {
    # name: (key_idx, aggs, layout or None, status, message part)
    "dict32_key": ([4], [(1, "count", None)], None, UNSUPPORTED, "merged by value"),
    "utf8_key": ([5], [(1, "count", None)], None, UNSUPPORTED, "utf8"),
    "dec128_key": ([3], [(1, "count", None)], None, UNSUPPORTED, "dec128 keys"),
    "five_keys": ([0, 6, 0, 6, 0], [(1, "count", None)], None, UNSUPPORTED, "1..4 key"),
    "nine_aggregates": ([0], [(1, "count", None)] * 9, None, UNSUPPORTED, "at most 8"),
    "count_state_f64": ([0], [(2, "count", None)], None, UNSUPPORTED, "i64 column"),
    "sum_f64_state_i64": ([0], [(1, "sum_f64", 1)], None, UNSUPPORTED, "f64 column"),
    "min_i64_state_f64": ([0], [(2, "min_i64", 1)], None, UNSUPPORTED, "i64 column"),
    "max_f64_state_dec": ([0], [(3, "max_f64", 1)], None, UNSUPPORTED, "f64 column"),
    "sum_dec_state_i64": ([0], [(1, "sum_dec128", 1)], None, UNSUPPORTED, "dec128 column"),
    "sum_i64_state_i32": ([0], [(6, "sum_i64", 1)], None, UNSUPPORTED, "i64 column"),
    "nn_f64": ([0], [(1, "sum_i64", 2)], None, UNSUPPORTED, "nn column must be i64"),
    "key_out_of_range": ([7], [(1, "count", None)], None, INVALID, "key column out of range"),
    "key_negative": ([-1], [(1, "count", None)], None, INVALID, "key column out of range"),
    "state_out_of_range": ([0], [(7, "count", None)], None, INVALID,
                           "state column out of range"),
    "nn_out_of_range": ([0], [(1, "sum_i64", 9)], None, INVALID, "nn column out of range"),
    "nn_missing": ([0], [(1, "sum_i64", None)], None, INVALID, "nn column out of range"),
    "offsets_start_past_zero": ([0], [(1, "count", None)], ([1, 8], [0], 1), INVALID,
                                "segment layout"),
    "offsets_end_short": ([0], [(1, "count", None)], ([0, 4, 7], [0, 0], 1), INVALID,
                          "segment layout"),
    "offsets_decrease": ([0], [(1, "count", None)], ([0, 6, 4, 8], [0, 0, 0], 1), INVALID,
                         "segment layout"),
    "seg_part_past_n_parts": ([0], [(1, "count", None)], ([0, 4, 8], [0, 2], 2), INVALID,
                              "segment layout"),
    "seg_part_negative": ([0], [(1, "count", None)], ([0, 4, 8], [0, -1], 2), INVALID,
                          "segment layout"),
    "no_partition": ([0], [(1, "count", None)], ([0, 8], [0], 0), INVALID, "segment layout"),
}


@pytest.fixture(scope="module")
def small_batch():
    batch = api.DeviceBatch(_small())
    yield batch
    batch.free()


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_their_cause(what, small_batch):
    key_idx, aggs, lay, status, part = REFUSALS[what]
    kw = {} if lay is None else layout(*lay)
    with pytest.raises(api.DDError) as ei:
        api.final_merge(small_batch, key_idx, aggs, **kw)
    assert ei.value.status == status, str(ei.value)
    assert "final merge" in str(ei.value) and part in str(ei.value)


def test_refuses_a_utf8view_key_and_two_to_the_31_rows(small_batch):
    views = np.zeros((4, 16), dtype=np.uint8)
    views[:, 0] = 1  # four 1-byte inline strings
    batch = api.DeviceBatch([{"dtype": "utf8view", "views": views, "bufs": [], "valid": None},
                             col("i64", np.ones(4, dtype=np.int64))])
    try:
        with pytest.raises(api.DDError) as ei:
            api.final_merge(batch, [0], [(1, "count", None)])
        assert ei.value.status == UNSUPPORTED and "utf8view" in str(ei.value)
    finally:
        batch.free()
    # a descriptor that only CLAIMS 2^31 rows: refused before anything is read
    desc = api.BatchDesc()
    ctypes.memmove(ctypes.byref(desc), ctypes.byref(small_batch.desc), ctypes.sizeof(desc))
    big = api.DeviceBatch.from_device([], 1 << 31)
    big.desc = desc
    big.desc.n_rows = 1 << 31
    with pytest.raises(api.DDError) as ei:
        api.final_merge(big, [0], [(1, "count", None)])
    assert ei.value.status == INVALID and "2^31" in str(ei.value)
