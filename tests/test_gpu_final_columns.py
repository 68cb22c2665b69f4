"""The final merge's columnar device output (api.final_merge_device, k_final_columns; marked
gpu): Merged.fetch() is held to finalagg.final_merge_ref by test_gpu_final_merge's checker,
and every typed column of Merged.batch() to Merged.fetch() bit for bit: keys in their input
dtype with validity from keynull, one column per aggregate with validity nn != 0, the nn
columns when asked for."""

import numpy as np
import pytest

from datafusion_distributed_amd import api, finalagg
from tests.test_gpu_final_merge import ALL_OPS, col, compare, layout, random_states

pytestmark = pytest.mark.gpu

KEY_NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.uint16, "i32": np.uint32,
          "f32": np.uint32, "i64": np.uint64, "f64": np.uint64}
AGG_DTYPE = {"count": "i64", "sum_i64": "i64", "min_i64": "i64", "max_i64": "i64",
             "sum_f64": "f64", "min_f64": "f64", "max_f64": "f64", "sum_dec128": "dec128"}


def raw(c):
    return np.ascontiguousarray(c["data"]).view(np.uint8).reshape(-1)


def check_columns(cols, key_idx, aggs, with_nn=False, **lay):
    ops = [op for _, op, _ in aggs]
    nk, na = len(key_idx), len(ops)
    batch = api.DeviceBatch(cols)
    m = api.final_merge_device(batch, key_idx, aggs, with_nn=with_nn, **lay)
    try:
        res = m.fetch()
        compare(res, finalagg.final_merge_ref(cols, key_idx, aggs, **lay), ops, nk)
        n = m.n_groups
        assert n == len(res["keynull"])
        key_dtypes = [cols[k]["dtype"] for k in key_idx]
        assert m.dtypes == key_dtypes + [AGG_DTYPE[o] for o in ops] + ["i64"] * (na * with_nn)
        view, vlay = m.batch()
        assert view.n_rows == n and view.desc.n_cols == m.n_cols == nk + na * (1 + with_nn)
        assert np.array_equal(vlay["seg_offsets"], res["group_offsets"])
        assert np.array_equal(vlay["seg_part"], np.arange(vlay["n_parts"]))
        assert vlay["n_parts"] == lay.get("n_parts", 1)
        lo = np.ascontiguousarray(res["aggs"]).view(np.uint64)
        for k, dt in enumerate(key_dtypes):
            got = m.col(k)
            want = np.ascontiguousarray(res["keys"][:, k].astype(KEY_NP[dt]))
            assert got["dtype"] == dt and np.array_equal(raw(got), want.view(np.uint8))
            assert np.array_equal(got["valid"], 1 - ((res["keynull"] >> k) & 1))
        for g, op in enumerate(ops):
            got = m.col(nk + g)
            if op == "sum_dec128":
                want = np.ascontiguousarray(np.stack([lo[:, g], res["aggs_hi"][:, g]], axis=1))
            else:
                want = np.ascontiguousarray(lo[:, g])
            assert np.array_equal(raw(got), want.view(np.uint8).reshape(-1)), f"agg {g} {op}"
            if op == "count":
                assert "valid" not in got  # never NULL
            else:
                assert np.array_equal(got["valid"], (res["nn"][:, g] != 0).astype(np.uint8))
            if with_nn:
                nn = m.col(nk + na + g)
                assert "valid" not in nn and nn["dtype"] == "i64"
                assert np.array_equal(nn["data"].view(np.uint64), res["nn"][:, g])
        return res
    finally:
        m.destroy()
        batch.free()


@pytest.mark.parametrize("with_nn", (False, True))
def test_every_op_and_key_dtype(with_nn):
    """All eight ops over four keys at a time, NULL key components included; a quarter of the
    partials have nn == 0, and the groups of key 0 == 0 have nothing else: total nn == 0."""
    rng = np.random.default_rng(60 + with_nn)
    n = 3000
    for dts in (("u8", "i16", "f32", "i64"), ("bool", "i32", "f64")):
        keys = []
        for j, dt in enumerate(dts):
            data = rng.integers(0, 2 if dt == "bool" else 3, n)
            if dt in ("f32", "f64"):  # canonicalised on the way out: -0.0 and NaNs included
                data = np.array([-0.0, 0.0, np.nan, 2.5])[rng.integers(0, 4, n)]
            keys.append(col(dt, data.astype(api.FIXED_NP[dt]),
                            (rng.random(n) < 0.8).astype(np.uint8) if j % 2 else None))
        st, aggs = random_states(rng, n, ALL_OPS, len(keys))
        dead = np.asarray(keys[0]["data"]) == 0
        for _, op, nc in aggs:
            if nc is not None:
                st[nc - len(keys)]["data"][dead] = 0
        lay = layout([0, 1000, 1700, n], [2, 0, 2], 4)
        res = check_columns(keys + st, list(range(len(keys))), aggs, with_nn, **lay)
        sums = [g for g, (_, op, _) in enumerate(aggs) if op != "count"]
        assert (res["nn"][:, sums] == 0).all(axis=1).any(), "no group with a total nn of 0"
        assert res["keynull"].any()
        hi = res["aggs_hi"][:, ALL_OPS.index("sum_dec128")]
        assert (hi != 0).any() and (hi != np.uint64(2**64 - 1)).any()  # the high word matters


def test_float_keys_come_out_canonical():
    n = 64
    bits = np.array([0x8000000000000000, 0x0, 0x7ff8000000000001, 0xfff8000000000000],
                    dtype=np.uint64)
    cols = [col("f64", np.tile(bits, n // 4).view(np.float64)),
            col("i64", np.ones(n, dtype=np.int64))]
    batch = api.DeviceBatch(cols)
    m = api.final_merge_device(batch, [0], [(1, "count", None)])
    try:
        got = sorted(m.col(0)["data"].view(np.uint64).tolist())
        assert got == [0x0, 0x7ff8000000000000]  # +0.0 for both zeros, one quiet NaN
        assert sorted(m.col(1)["data"].tolist()) == [n // 2, n // 2]
    finally:
        m.destroy()
        batch.free()


def test_zero_groups():
    st, aggs = random_states(np.random.default_rng(62), 0, ["count", "sum_dec128", "min_f64"], 1)
    cols = [col("i32", np.zeros(0, dtype=np.int32))] + st
    res = check_columns(cols, [0], aggs, True, **layout([0, 0, 0], [1, 0], 3))
    assert res["group_offsets"].tolist() == [0, 0, 0, 0]


def test_fetch_equals_final_merge():
    """Merged.fetch() is api.final_merge's answer on the same input once the groups inside
    each partition are put in one order (theirs is unspecified). Exact ops only: a float sum
    depends on the order of its atomics."""
    rng = np.random.default_rng(63)
    n = 4000
    ops = [o for o in ALL_OPS if o != "sum_f64"]
    st, aggs = random_states(rng, n, ops, 2)
    cols = [col("i32", rng.integers(-20, 20, n).astype(np.int32)),
            col("u8", rng.integers(0, 3, n).astype(np.uint8),
                (rng.random(n) < 0.9).astype(np.uint8))] + st
    lay = layout([0, 1500, 1500, n], [1, 0, 3], 5)
    batch = api.DeviceBatch(cols)
    m = api.final_merge_device(batch, [0, 1], aggs, **lay)
    try:
        a = m.fetch()
        b = api.final_merge(batch, [0, 1], aggs, **lay)
    finally:
        m.destroy()
        batch.free()
    assert np.array_equal(a["group_offsets"], b["group_offsets"])

    def ordered(r):
        part = np.repeat(np.arange(5), np.diff(r["group_offsets"]))
        order = np.lexsort((r["keynull"], r["keys"][:, 1], r["keys"][:, 0], part))
        # a NULL aggregate's value slot is unspecified: compare it as zero
        live = r["nn"][order] != 0
        lo = np.where(live, np.ascontiguousarray(r["aggs"]).view(np.uint64)[order], 0)
        hi = np.where(live, r["aggs_hi"][order], 0)
        return r["keys"][order], r["keynull"][order], r["nn"][order], lo, hi

    for x, y in zip(ordered(a), ordered(b)):
        assert np.array_equal(x, y)


def test_refusals_are_the_final_merges():
    cols = [col("dec128", np.zeros((4, 2), dtype=np.uint64)), col("i64", np.ones(4, np.int64))]
    batch = api.DeviceBatch(cols)
    try:
        with pytest.raises(api.DDError) as ei:
            api.final_merge_device(batch, [0], [(1, "count", None)])
        assert ei.value.status == 6 and "dec128 keys" in str(ei.value)
        with pytest.raises(api.DDError) as ei:
            api.final_merge_device(batch, [1], [(1, "count", None)], [0, 3], [0], 1)
        assert ei.value.status == 1 and "segment layout" in str(ei.value)
    finally:
        batch.free()
