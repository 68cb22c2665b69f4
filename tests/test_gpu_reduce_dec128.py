"""The wide partial-reduce kernel vs the exact models (marked gpu).

One checker, check_wide, runs a plan through api.partial_reduce under both settings of
DD_REDUCE_WAVEAGG and holds each result to the models: raw-partial invariants on every
output row, then — after the final merge — the exact group set, nn, bit-exact decimal sums
(decagg.final_merge_dec against decagg.reduce_dec_ref, Python ints modulo 2^128) and the
narrow aggregates as tests/test_gpu_reduce_parity.py holds them (oracle/reduce_ref.py's
final_merge against reduce_ref, which the decagg functions delegate to). Launch geometry
always comes from api.partial_reduce_plan_geometry."""

import math

import numpy as np
import pytest

from datafusion_distributed_amd import api, decagg
from oracle import reduce_ref as rr
from tests.test_gpu_fuzz import random_col
from tests.test_gpu_reduce_parity import FUZZ_SHAPES, col, keys_with_home_slot, nulls

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
M64 = (1 << 64) - 1
BIG = (1 << 127) - 1
Q1_OPS = ["sum_dec128"] * 5 + ["count"]


def dec_col(values, valid=None):
    """dec128 column from signed Python ints."""
    return col("dec128", decagg.dec_words(values), valid)


def dec_words_col(words, valid=None):
    return col("dec128", np.ascontiguousarray(words, dtype=np.uint64), valid)


def small_dec(rng, n, null_p=0.0):
    """|v| < 10^15 like a decimal128(15, 2) money column."""
    v = rng.integers(-10**15 + 1, 10**15, n).tolist()
    return dec_col(v, nulls(rng, n, null_p) if null_p else None)


def check_wide(monkeypatch, cols, key_idx, aggs, exact_f64_sum=False, kernel=1):
    """Run the plan with DD_REDUCE_WAVEAGG=0 and 1 and hold both results to the models.
    Returns ({waveagg: raw partial}, geometry, {waveagg: merged groups})."""
    n = len(cols[key_idx[0]]["data"])
    nk = len(key_idx)
    ops = [o for _, o in aggs]
    geo = api.partial_reduce_plan_geometry(n, nk, ops)
    assert geo["kernel"] == kernel
    want = decagg.reduce_dec_ref(cols, key_idx, aggs)
    raw, merged = {}, {}
    for wa in (0, 1):
        monkeypatch.setenv("DD_REDUCE_WAVEAGG", str(wa))
        batch = api.DeviceBatch(cols)
        try:
            res = api.partial_reduce(batch, key_idx, aggs)
        finally:
            batch.free()
        # the configuration reached the kernel it names
        assert res["kernel"] == kernel
        assert res["waveagg"] == (wa if kernel == 1 else 0)
        keys, keynull, nn = res["keys"], res["keynull"], res["nn"].astype(np.int64)
        rows = len(keynull)

        # a. raw-partial invariants, every output row
        assert keys.shape == (rows, nk)
        assert res["aggs"].shape == res["aggs_hi"].shape == (rows, len(aggs))
        assert rows <= n + geo["nblocks"] * geo["table_slots"]
        assert (keynull >> np.uint32(nk) == 0).all(), "keynull bit at or above n_keys"
        for k in range(nk):
            isnull = ((keynull >> np.uint32(k)) & 1).astype(bool)
            assert (keys[isnull, k] == 0).all(), f"NULL key component {k} with non-zero bits"
        for g, op in enumerate(ops):
            lo = np.ascontiguousarray(res["aggs"][:, g]).view(np.uint64)
            hi = res["aggs_hi"][:, g]
            if op == "sum_dec128":
                empty = nn[:, g] == 0
                assert (lo[empty] == 0).all() and (hi[empty] == 0).all(), (
                    "decimal partial with nn == 0 must hold (0, 0)")
            else:
                assert (hi == 0).all(), f"high half set for {op}"
            if op == "count":
                cnt = lo.view(np.int64)
                assert (cnt >= 1).all(), "partial row with count < 1"
                assert (nn[:, g] == cnt).all(), "nn[count] != count"
                assert (nn <= cnt[:, None]).all(), "non-null count above row count"

        # b. after the final merge: group set, nn, values
        got = decagg.final_merge_dec(res, ops)
        missing = want.keys() - got.keys()
        invented = got.keys() - want.keys()
        assert not missing and not invented, (
            f"waveagg {wa}: groups missing {sorted(missing)[:5]} invented "
            f"{sorted(invented)[:5]}")
        for gid, went in want.items():
            for g, (ge, we) in enumerate(zip(got[gid], went)):
                ctx = f"waveagg {wa} group {gid} agg {g} {we['op']}: got {ge} want {we}"
                assert ge["op"] == we["op"] and ge["nn"] == we["nn"], ctx
                gv, wv = ge["value"], we["value"]
                if we["op"] != "sum_f64" or wv is None:
                    assert gv == wv and type(gv) is type(wv), ctx  # decimal sums: bit-exact
                elif not math.isfinite(wv):
                    assert gv == wv or (gv != gv and wv != wv), ctx
                elif exact_f64_sum:
                    assert gv == wv, ctx
                else:
                    # any-order summation bound, as tests/test_gpu_reduce_parity.py derives it
                    bound = we["n_nonnull"] * 2.0 ** -52 * we["abs_sum"]
                    assert abs(gv - wv) <= bound, f"{ctx} err {abs(gv - wv)} bound {bound}"
        raw[wa], merged[wa] = res, got
    return raw, geo, merged


# ---------------- 1. sizes ----------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097, 150_001])
def test_sizes(monkeypatch, n):
    rng = np.random.default_rng(1100 + n)
    ops = ["count", "sum_dec128"]
    if n == 150_001:  # more than the minimum block count, ragged last chunk
        geo = api.partial_reduce_plan_geometry(n, 1, ops)
        assert geo["nblocks"] > api.partial_reduce_plan_geometry(0, 1, ops)["nblocks"]
        assert n % geo["chunk_rows"] != 0
    cols = [col("i64", rng.integers(-5, 5, n, dtype=np.int64)), small_dec(rng, n, 0.1)]
    raw, _, got = check_wide(monkeypatch, cols, [0], [(None, "count"), (1, "sum_dec128")])
    for wa in (0, 1):
        if n == 0:
            assert len(raw[wa]["keynull"]) == 0 and got[wa] == {}
        assert sum(e[0]["value"] for e in got[wa].values()) == n


# ---------------- 2. carries, signs, wraps, all-NULL ----------------

def _carry_data(rng):
    per = 3000
    groups = []
    # 0: every low-word add carries (lo = 2^64 - 1, hi = 0)
    groups.append([M64] * per)
    # 1: small negatives (hi all ones) and positives mixed: carries and sign words cross
    groups.append(rng.integers(-1000, 1000, per).tolist())
    # 2: the exact sum leaves the signed 128-bit range
    groups.append([BIG - int(x) for x in rng.integers(0, 1000, per)])
    # 3: every input NULL
    groups.append(rng.integers(-10**9, 10**9, per).tolist())
    k = np.repeat(np.arange(4, dtype=np.int64), per)
    v = [x for g in groups for x in g]
    valid = nulls(rng, len(v), 0.1)
    valid[k == 3] = 0
    p = rng.permutation(len(v))
    return k[p], [v[i] for i in p], valid[p]


def test_carries_signs_wraps_and_null_groups(monkeypatch):
    rng = np.random.default_rng(1202)
    k, v, valid = _carry_data(rng)
    words = decagg.dec_words(v)
    ok = valid.astype(bool)
    # the data premises
    g0 = (k == 0) & ok
    assert (words[g0, 0] == np.uint64(M64)).all() and (words[g0, 1] == 0).all()
    g1 = words[(k == 1) & ok, 1]
    assert (g1 == np.uint64(M64)).any() and (g1 == 0).any()
    exact2 = sum(x for x, kk, o in zip(v, k.tolist(), ok.tolist()) if kk == 2 and o)
    assert exact2 > BIG
    _, _, got = check_wide(monkeypatch, [col("i64", k), dec_col(v, valid)], [0],
                           [(1, "sum_dec128"), (None, "count")])
    for wa in (0, 1):
        assert got[wa][((0,), 0)][0]["value"] == int(g0.sum()) * M64
        assert got[wa][((2,), 0)][0]["value"] == decagg.to_signed128(exact2) != exact2
        assert got[wa][((3,), 0)][0] == {"op": "sum_dec128", "value": None, "nn": 0}


# ---------------- 3. eight aggregates; narrow-only wide plan; dispatch ----------------

def test_eight_mixed_aggregates(monkeypatch):
    rng = np.random.default_rng(1303)
    n = 20_000
    full = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    near = np.stack([np.uint64(M64) - rng.integers(0, 4, n).astype(np.uint64),
                     rng.integers(0, 3, n).astype(np.uint64)], axis=1)
    cols = [col("u8", rng.integers(0, 3, n).astype(np.uint8)),
            col("bool", rng.integers(0, 2, n).astype(np.uint8), nulls(rng, n, 0.1)),
            small_dec(rng, n), small_dec(rng, n, 0.2), dec_words_col(full, nulls(rng, n, 0.3)),
            dec_words_col(near), small_dec(rng, n, 1.0),  # col 6: every value NULL
            col("f64", rng.integers(-1000, 1000, n).astype(np.float64), nulls(rng, n, 0.1)),
            col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64), nulls(rng, n, 0.1))]
    aggs = [(2, "sum_dec128"), (3, "sum_dec128"), (4, "sum_dec128"), (None, "count"),
            (5, "sum_dec128"), (7, "sum_f64"), (6, "sum_dec128"), (8, "min_i64")]
    _, _, got = check_wide(monkeypatch, cols, [0, 1], aggs, exact_f64_sum=True)
    assert len(got[0]) == 9  # 3 x (false, true, NULL)
    assert all(e[6]["value"] is None for e in got[1].values())


def test_six_narrow_sums_run_the_wide_kernel(monkeypatch):
    rng = np.random.default_rng(1304)
    n = 10_000
    cols = [col("i32", rng.integers(0, 40, n).astype(np.int32))]
    cols += [col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64), nulls(rng, n, 0.2))
             for _ in range(6)]
    check_wide(monkeypatch, cols, [0], [(c, "sum_i64") for c in range(1, 7)])


def test_dispatch_narrow_plans_keep_the_existing_kernel(monkeypatch):
    rng = np.random.default_rng(1305)
    n = 5000
    cols = [col("i32", rng.integers(0, 9, n).astype(np.int32)),
            col("i64", rng.integers(-99, 99, n, dtype=np.int64)),
            col("f64", rng.integers(-99, 99, n).astype(np.float64))]
    aggs = [(None, "count"), (1, "sum_i64"), (2, "sum_f64"), (1, "max_i64")]
    raw, geo, _ = check_wide(monkeypatch, cols, [0], aggs, exact_f64_sum=True, kernel=0)
    old = api.partial_reduce_geometry(n)
    assert {k: geo[k] for k in old} == old
    assert (raw[0]["aggs_hi"] == 0).all()


# ---------------- 4. forced spill, probe wrap ----------------

def _signext(lo):
    return np.where(lo >> np.uint64(63) == 1, np.uint64(M64), np.uint64(0))


def test_forced_spill_carries_full_128_bit_values(monkeypatch):
    """96 keys that all home at the LAST table slot, 40 rows each: a block seats at most
    probe_limit of them, the rest spill as singletons with their (lo, hi) intact."""
    rng = np.random.default_rng(1407)
    ops = ["count", "sum_dec128"]
    geo = api.partial_reduce_plan_geometry(3840, 1, ops)
    pool = keys_with_home_slot(geo["table_slots"] - 1, 96, geo["table_slots"])
    keys = rng.permutation(np.repeat(pool, 40))
    n = len(keys)
    assert n == 3840
    for b in range(geo["nblocks"]):  # input precondition: every block must overflow
        chunk = keys[b * geo["chunk_rows"]:(b + 1) * geo["chunk_rows"]]
        assert len(np.unique(chunk)) > geo["probe_limit"]
    words = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    assert (words[:, 1] != _signext(words[:, 0])).all()  # hi is no sign extension of lo
    raw, geo, _ = check_wide(monkeypatch, [col("i64", keys), dec_words_col(words)], [0],
                             [(None, "count"), (1, "sum_dec128")])
    inputs = set(zip(keys.tolist(), words[:, 0].tolist(), words[:, 1].tolist()))
    for wa in (0, 1):
        res = raw[wa]
        rows = len(res["keynull"])
        # table rows <= nblocks * probe_limit, so anything beyond is a singleton spill row
        assert rows > geo["nblocks"] * geo["probe_limit"]
        single = np.ascontiguousarray(res["aggs"][:, 0]).view(np.int64) == 1
        assert single.sum() >= rows - geo["nblocks"] * geo["probe_limit"]
        lo = np.ascontiguousarray(res["aggs"][:, 1]).view(np.uint64)[single]
        hi = res["aggs_hi"][:, 1][single]
        k = res["keys"][:, 0].view(np.int64)[single]
        assert set(zip(k.tolist(), lo.tolist(), hi.tolist())) <= inputs
        assert (hi != _signext(lo)).all()


def test_probe_walk_wraps_past_the_table_end(monkeypatch):
    """4 keys that all home at the LAST slot, the key chosen by (row offset in the block's
    chunk) mod 4 so every thread meets one key for good (the reasoning of the test of the
    same name in tests/test_gpu_reduce_parity.py): three of them are seated only if the
    walk wraps to slot 0. A walk stuck at the last slot would spill three quarters of the
    input."""
    n = 131_072
    rng = np.random.default_rng(1408)
    ops = ["count", "sum_dec128"]
    geo = api.partial_reduce_plan_geometry(n, 1, ops)
    assert geo["block_threads"] % 4 == 0
    pool = keys_with_home_slot(geo["table_slots"] - 1, 4, geo["table_slots"])
    offset = np.arange(n) % geo["chunk_rows"]
    cols = [col("i64", pool[offset % 4]), small_dec(rng, n)]
    raw, geo, got = check_wide(monkeypatch, cols, [0], [(None, "count"), (1, "sum_dec128")])
    for wa in (0, 1):
        assert len(got[wa]) == 4
        rows = len(raw[wa]["keynull"])
        print(f"wrap waveagg {wa}: {rows} partial rows for {n} input rows")
        assert rows <= geo["nblocks"] * (geo["probe_limit"] + geo["block_threads"])


# ---------------- 5. low and high cardinality ----------------

def test_low_cardinality_never_spills(monkeypatch):
    rng = np.random.default_rng(1509)
    n = 131_072
    cols = [col("u8", rng.integers(0, 3, n).astype(np.uint8)),
            col("bool", rng.integers(0, 2, n).astype(np.uint8))]
    cols += [small_dec(rng, n) for _ in range(5)]
    aggs = [(c, "sum_dec128") for c in range(2, 7)] + [(None, "count")]
    raw, geo, got = check_wide(monkeypatch, cols, [0, 1], aggs)
    for wa in (0, 1):
        assert len(got[wa]) == 6
        assert len(raw[wa]["keynull"]) <= geo["nblocks"] * geo["table_slots"]


def test_high_cardinality_takes_the_per_lane_path(monkeypatch):
    rng = np.random.default_rng(1510)
    n = 30_000
    full = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    cols = [col("i32", rng.integers(0, 30_000, n).astype(np.int32)),
            dec_words_col(full, nulls(rng, n, 0.1)), small_dec(rng, n)]
    _, _, got = check_wide(monkeypatch, cols, [0],
                           [(1, "sum_dec128"), (2, "sum_dec128"), (None, "count")])
    assert len(got[1]) > 15_000


# ---------------- 6. refusals ----------------

def test_refusals_name_the_cause():
    rng = np.random.default_rng(1611)
    n = 100
    batch = api.DeviceBatch([col("i64", rng.integers(0, 5, n, dtype=np.int64)),
                             small_dec(rng, n),
                             col("f64", rng.normal(size=n))])
    try:
        with pytest.raises(api.DDError) as ei:
            api.partial_reduce(batch, [0], [(0, "sum_dec128")])
        assert ei.value.status == 6 and "sum_dec128 needs a dec128 column" in str(ei.value)
        with pytest.raises(api.DDError) as ei:
            api.partial_reduce(batch, [0], [(1, "sum_f64")])
        assert ei.value.status == 6 and "dec128" in str(ei.value)
        with pytest.raises(api.DDError) as ei:
            api.partial_reduce(batch, [0], [(None, "count")] * 9)
        assert ei.value.status == 6 and "at most 8 aggregates" in str(ei.value)
    finally:
        batch.free()


# ---------------- fuzz ----------------

def fuzz_dec(rng, n, null_p):
    """Decimal data from three regimes, mixed per row: |v| < 10^15, full 128-bit random,
    and lo within a few units of 2^64 with a small hi."""
    small = decagg.dec_words(rng.integers(-10**15 + 1, 10**15, n).tolist())
    full = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)
    near = np.stack([np.uint64(M64) - rng.integers(0, 3, n).astype(np.uint64),
                     rng.choice(np.array([0, 1, M64], dtype=np.uint64), n)], axis=1)
    regime = rng.integers(0, 3, n)[:, None]
    words = np.where(regime == 0, small, np.where(regime == 1, full, near))
    return dec_words_col(words, nulls(rng, n, null_p) if null_p > 0 else None)


@pytest.mark.parametrize("case", range(12))
def test_fuzz_reduce_wide(monkeypatch, case):
    rng = np.random.default_rng(9100 + case)
    n, card = FUZZ_SHAPES[case]
    nk = int(rng.integers(1, 5))
    na = int(rng.integers(1, 9))
    cols = []
    for dt in rng.choice(["u8", "i16", "i32", "i64", "f32", "f64", "bool", "dict32"], nk):
        c = random_col(rng, n, str(dt), float(rng.choice([0, 0.1, 0.5, 1.0])))
        take = rng.integers(0, min(card, n), n)  # draw rows from a pool of `card` values
        c["data"] = np.ascontiguousarray(c["data"][take])
        cols.append(c)
    aggs = []
    for op in rng.choice(list(rr.OPS) + ["sum_dec128"] * 5, na):
        op = str(op)
        if op == "count":
            aggs.append((None, op))
            continue
        null_p = float(rng.choice([0, 0.1, 0.5, 1.0]))
        if op == "sum_dec128":
            cols.append(fuzz_dec(rng, n, null_p))
        else:
            cols.append(random_col(rng, n, "f64" if op.endswith("f64") else "i64", null_p))
        aggs.append((len(cols) - 1, op))
    ops = [o for _, o in aggs]
    kernel = 1 if na > 4 or "sum_dec128" in ops else 0
    raw, geo, got = check_wide(monkeypatch, cols, list(range(nk)), aggs, kernel=kernel)
    print(f"fuzz {case}: n={n} keys={[c['dtype'] for c in cols[:nk]]} aggs={ops} "
          f"kernel={kernel} groups={len(got[0])} rows={len(raw[0]['keynull'])}")
