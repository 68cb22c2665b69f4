"""GPU partial aggregation vs the exact reference model (marked gpu).

One checker, check_reduce, runs k_partial_reduce through api.partial_reduce and holds it
to oracle/reduce_ref.py: raw-partial invariants on every output row, then — after the
op-aware final merge — the exact group set, bit-exact counts / nn / integer aggregates /
totalOrder min-max bit patterns, and float sums within the derived any-order summation
bound (bit-exact where the inputs make every partial sum exact). Launch geometry (table
slots, probe limit, block count, chunk rows) always comes from
api.partial_reduce_geometry, never from literals mirrored here."""

import math

import numpy as np
import pytest

from datafusion_distributed_amd import api
from oracle import pyref
from oracle import reduce_ref as rr
from tests.test_gpu_fuzz import random_col

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
NEG_QNAN = 0xFFF8000000000000
POS_QNAN = 0x7FF8000000000000
PAYLOAD_NAN = 0x7FF8000000000ABC
NEG_ZERO = 0x8000000000000000
SPECIAL_F64 = np.array(
    [POS_QNAN, NEG_QNAN, PAYLOAD_NAN, 0x7FF0000000000000, 0xFFF0000000000000, 0, NEG_ZERO,
     1, 0x8000000000000001, 0x000FFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)


def col(dtype, data, valid=None, **kw):
    return dict({"dtype": dtype, "data": data, "valid": valid}, **kw)


def nulls(rng, n, p):
    return (rng.random(n) >= p).astype(np.uint8)


def check_reduce(cols, key_idx, aggs, exact_f64_sum=False, by_value=None):
    """Run the kernel and hold it to the model. by_value = (dict_values, ref_cols):
    compare after merge_dict_by_value against reduce_ref over ref_cols (whose dict32 key
    indices are canonical per value). Returns (raw partial, geometry, merged groups)."""
    n = len(cols[0]["data"])
    nk = len(key_idx)
    ops = [o for _, o in aggs]
    geo = api.partial_reduce_geometry(n)
    batch = api.DeviceBatch(cols)
    try:
        res = api.partial_reduce(batch, key_idx, aggs)
    finally:
        batch.free()
    keys, keynull, nn = res["keys"], res["keynull"], res["nn"].astype(np.int64)
    rows = len(keynull)

    # a. raw-partial invariants, every output row
    assert keys.shape == (rows, nk) and res["aggs"].shape == (rows, len(aggs))
    assert rows <= n + geo["nblocks"] * geo["table_slots"]
    assert (keynull >> np.uint32(nk) == 0).all(), "keynull bit at or above n_keys"
    for k in range(nk):
        isnull = ((keynull >> np.uint32(k)) & 1).astype(bool)
        assert (keys[isnull, k] == 0).all(), f"NULL key component {k} with non-zero bits"
    for g, op in enumerate(ops):
        if op != "count":
            continue
        cnt = np.ascontiguousarray(res["aggs"][:, g]).view(np.int64)
        assert (cnt >= 1).all(), "partial row with count < 1"
        assert (nn[:, g] == cnt).all(), "nn[count] != count"
        assert (nn <= cnt[:, None]).all(), "non-null count above row count"

    # b./c. after the final merge
    got = rr.final_merge(res, ops)
    if by_value is None:
        want = rr.reduce_ref(cols, key_idx, aggs)
    else:
        dict_values, ref_cols = by_value
        ref = rr.reduce_ref(ref_cols, key_idx, aggs)
        want = rr.merge_dict_by_value(ref, dict_values)
        assert len(want) == len(ref)  # the reference itself never needed a merge
        got = rr.merge_dict_by_value(got, dict_values)
    missing = want.keys() - got.keys()
    invented = got.keys() - want.keys()
    assert not missing and not invented, (
        f"groups missing {sorted(missing)[:5]} invented {sorted(invented)[:5]}")
    for gid, went in want.items():
        for g, (ge, we) in enumerate(zip(got[gid], went)):
            ctx = f"group {gid} agg {g} {we['op']}: got {ge} want {we}"
            assert ge["nn"] == we["nn"], ctx
            gv, wv = ge["value"], we["value"]
            if we["op"] != "sum_f64" or wv is None:
                assert gv == wv and type(gv) is type(wv), ctx
            elif not math.isfinite(wv):
                assert gv == wv or (gv != gv and wv != wv), ctx
            elif exact_f64_sum:
                assert gv == wv, ctx
            else:
                # any-order summation: (n-1) u sum|x| with u = 2^-53, doubled for the
                # reference's and the final merge's own roundings
                bound = we["n_nonnull"] * 2.0 ** -52 * we["abs_sum"]
                assert abs(gv - wv) <= bound, f"{ctx} err {abs(gv - wv)} bound {bound}"
    return res, geo, got


# ---------------- helpers that aim rows at chosen table slots ----------------

def keys_with_home_slot(slot, want, table_slots, scan=400_000):
    """i64 keys from 0..scan whose home slot max(h, 1) % table_slots equals `slot`."""
    cand = np.arange(scan, dtype=np.int64)
    h = pyref.hash_cols([col("i64", cand)], scan)
    home = np.maximum(h, np.uint64(1)) % np.uint64(table_slots)
    hit = cand[home == np.uint64(slot)]
    assert len(hit) >= want, f"only {len(hit)} keys home at slot {slot}"
    return hit[:want]


M64 = (1 << 64) - 1


def _unxorshift(x, s):
    t = x
    for _ in range(64 // s + 1):
        t = x ^ (t >> s)
    return t


def inv_mix64(z):
    z = _unxorshift(z, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    z = _unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    return _unxorshift(z, 30)


def _combine(h, vh):
    return h ^ ((vh + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & M64)


def colliding_third_key(a, b, target):
    """i64 c such that rowhash(a, b, c) == target (pyref.hash_cols' combine, inverted)."""
    h = _combine(_combine(0, pyref.mix64_scalar(a)), pyref.mix64_scalar(b))
    vh = ((target ^ h) - 0x9E3779B97F4A7C15 - (h << 6) - (h >> 2)) & M64
    return rr.to_signed64(inv_mix64(vh))


def special_f64_groups(rng, gclass):
    """f64 aggregate data by group class (gclass in 0..7): class 0 only +-0.0, class 1
    only NaNs (both signs, one payload), the rest normals seeded with every special."""
    n = len(gclass)
    v = rng.normal(size=n) * 1e3
    seed = rng.random(n) < 0.15
    v[seed] = SPECIAL_F64[rng.integers(0, len(SPECIAL_F64), int(seed.sum()))]
    z = gclass == 0
    v[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    nan = gclass == 1
    v[nan] = SPECIAL_F64[rng.integers(0, 3, int(nan.sum()))]
    return v


# ---------------- 1. sizes ----------------

@pytest.mark.parametrize("n", [0, 1, 7, 8, 255, 256, 257, 4097, 150_001])
def test_sizes(n):
    rng = np.random.default_rng(100 + n)
    geo = api.partial_reduce_geometry(n)
    if n == 150_001:  # more than the minimum block count, ragged last chunk
        assert geo["nblocks"] > api.partial_reduce_geometry(0)["nblocks"]
        assert n % geo["chunk_rows"] != 0
    cols = [col("i64", rng.integers(-5, 5, n, dtype=np.int64)),
            col("f64", rng.integers(-1000, 1000, n).astype(np.float64), nulls(rng, n, 0.1)),
            col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64))]
    res, _, got = check_reduce(cols, [0], [(None, "count"), (1, "sum_f64"), (2, "min_i64")],
                               exact_f64_sum=True)
    if n == 0:
        assert len(res["keynull"]) == 0 and got == {}
    assert sum(e[0]["value"] for e in got.values()) == n


# ---------------- 2. every op, with NULLs ----------------

def test_every_op_with_nulls():
    rng = np.random.default_rng(202)
    n = 20_000
    k = rng.integers(0, 12, n, dtype=np.int64).astype(np.int32)
    f = rng.normal(size=n) * 1e6
    i = rng.integers(I64.min, I64.max, n, dtype=np.int64)  # sums wrap past 2^63
    i[rng.integers(0, n, 40)] = I64.min
    i[rng.integers(0, n, 40)] = I64.max
    fv, iv = nulls(rng, n, 0.3), nulls(rng, n, 0.3)
    fv[k == 7] = 0  # group 7: every aggregate input NULL
    iv[k == 7] = 0
    cols = [col("i32", k), col("f64", f, fv), col("i64", i, iv)]
    # the data premise: some group's exact i64 sum leaves the signed range
    exact = [int(i[(k == g) & (iv == 1)].astype(object).sum()) for g in range(12)]
    assert any(not I64.min <= s <= I64.max for s in exact)
    _, _, got = check_reduce(cols, [0], [(1, "sum_f64"), (1, "min_f64"), (1, "max_f64"),
                                         (None, "count")])
    assert [e["value"] for e in got[((7,), 0)]][:3] == [None, None, None]
    _, _, got = check_reduce(cols, [0], [(2, "sum_i64"), (2, "min_i64"), (2, "max_i64"),
                                         (None, "count")])
    assert [e["value"] for e in got[((7,), 0)]][:3] == [None, None, None]
    assert any(e[1]["value"] == I64.min for e in got.values())
    assert any(e[2]["value"] == I64.max for e in got.values())


# ---------------- 3. totalOrder min/max ----------------

@pytest.mark.parametrize("spill", [False, True], ids=["table", "spill"])
def test_total_order_min_max(spill):
    rng = np.random.default_rng(303)
    geo = api.partial_reduce_geometry(3840)
    if spill:  # the forced-exhaustion keys of test_forced_probe_exhaustion_and_wrap
        pool = keys_with_home_slot(geo["table_slots"] - 1, 96, geo["table_slots"])
        pick = rng.permutation(np.repeat(np.arange(96), 40))
    else:
        pool = np.arange(8, dtype=np.int64)
        pick = rng.integers(0, 8, 3840)
    gclass = pick % 8
    v = special_f64_groups(rng, gclass)
    valid = nulls(rng, len(v), 0.2)
    planted = {0: [0, NEG_ZERO], 1: [NEG_QNAN, PAYLOAD_NAN, POS_QNAN],
               2: [NEG_QNAN, PAYLOAD_NAN, 0xFFF0000000000000, 0x7FF0000000000000]}
    for g, bits in planted.items():  # the groups asserted on below hold these for sure
        at = np.flatnonzero(pick == g)[:len(bits)]
        v[at] = np.array(bits, dtype=np.uint64).view(np.float64)
        valid[at] = 1
    cols = [col("i64", pool[pick]), col("f64", v, valid)]
    res, geo, got = check_reduce(cols, [0], [(1, "min_f64"), (1, "max_f64"),
                                             (None, "count")])
    if spill:
        assert len(res["keynull"]) > geo["nblocks"] * geo["probe_limit"]
    zeros = got[((int(np.uint64(pool[0])),), 0)]
    assert zeros[0]["value"] == NEG_ZERO and zeros[1]["value"] == 0
    nans = got[((int(np.uint64(pool[1])),), 0)]
    assert nans[0]["value"] == NEG_QNAN and nans[1]["value"] == PAYLOAD_NAN
    mixed = got[((int(np.uint64(pool[2])),), 0)]
    assert mixed[0]["value"] == NEG_QNAN  # sign-set NaN sorts below -inf
    assert mixed[1]["value"] == PAYLOAD_NAN  # payload NaN above the plain quiet NaN


# ---------------- 4. float keys ----------------

F32_KEYS = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                     0x3FC00000, 0xC0100000, 0x7F800000, 0xFF800000, 0x00000001],
                    dtype=np.uint32).view(np.float32)
F64_KEYS = np.array([0, NEG_ZERO, POS_QNAN, NEG_QNAN, 0x7FF0000000000001,
                     0x3FF8000000000000, 0xC002000000000000, 0x7FF0000000000000,
                     0xFFF0000000000000, 1], dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("keys", [[0], [1], [0, 1]], ids=["f32", "f64", "f32_f64"])
def test_float_keys_canonicalise(keys):
    rng = np.random.default_rng(404)
    n = 5000
    cols = [col("f32", F32_KEYS[rng.integers(0, 10, n)], nulls(rng, n, 0.1)),
            col("f64", F64_KEYS[rng.integers(0, 10, n)]),
            col("f64", rng.integers(-50, 50, n).astype(np.float64))]
    res, _, got = check_reduce(cols, keys, [(None, "count"), (2, "sum_f64")],
                               exact_f64_sum=True)
    canon = {0: {0, 0x7FC00000, 0x3FC00000, 0xC0100000, 0x7F800000, 0xFF800000, 1},
             1: {0, POS_QNAN, 0x3FF8000000000000, 0xC002000000000000, 0x7FF0000000000000,
                 0xFFF0000000000000, 1}}
    for pos, ci in enumerate(keys):  # raw rows carry only canonical bits
        assert set(res["keys"][:, pos].tolist()) == canon[ci]
    if len(keys) == 1:  # +-0.0 is ONE group, the three NaNs are ONE group (+ the NULL)
        assert len(got) == 7 + (1 if keys == [0] else 0)
    else:
        assert len(got) == 8 * 7


# ---------------- 5. multi-key NULL masks ----------------

@pytest.mark.parametrize("key_idx", [[0, 1, 2, 3], [1, 2, 3], [3, 1]],
                         ids=["4keys", "3keys", "2keys"])
def test_multi_key_null_masks(key_idx):
    rng = np.random.default_rng(505)
    n = 6000
    cols = [col("u8", rng.integers(0, 3, n).astype(np.uint8), nulls(rng, n, 0.25)),
            col("i16", rng.integers(-2, 1, n).astype(np.int16), nulls(rng, n, 0.25)),
            col("bool", rng.integers(0, 2, n).astype(np.uint8), nulls(rng, n, 0.25)),
            col("i32", rng.integers(-1, 2, n).astype(np.int32), nulls(rng, n, 0.25)),
            col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64),
                nulls(rng, n, 0.3))]
    mask = np.zeros(n, dtype=np.int64)
    for pos, ci in enumerate(key_idx):
        mask |= (1 - cols[ci]["valid"].astype(np.int64)) << pos
    assert set(mask.tolist()) == set(range(1 << len(key_idx)))  # every mask occurs
    res, _, got = check_reduce(cols, key_idx, [(None, "count"), (4, "sum_i64"),
                                               (4, "max_i64")])
    assert set(res["keynull"].tolist()) == set(range(1 << len(key_idx)))
    all_null = ((0,) * len(key_idx), (1 << len(key_idx)) - 1)  # row hash 0: the sentinel
    assert got[all_null][0]["value"] == int((mask == (1 << len(key_idx)) - 1).sum())


# ---------------- 6. dict32 keys ----------------

def dict_col(values, idx, valid=None):
    doff = np.zeros(len(values) + 1, dtype=np.int32)
    doff[1:] = np.cumsum([len(v) for v in values])
    by = np.frombuffer(b"".join(values), dtype=np.uint8).copy()
    return col("dict32", idx.astype(np.int32), valid, dict_bytes=by, dict_offsets=doff)


def test_dict_key_null_rows_carry_out_of_range_indices():
    rng = np.random.default_rng(606)
    n = 5000
    values = [b"alpha", b"", b"gamma", b"delta-long-value"]  # includes the empty string
    idx = rng.integers(0, len(values), n)
    valid = nulls(rng, n, 0.3)
    bad = np.array([-1, len(values)])
    idx[valid == 0] = bad[rng.integers(0, 2, int((valid == 0).sum()))]
    cols = [dict_col(values, idx, valid), col("i64", rng.integers(-9, 9, n, dtype=np.int64))]
    _, _, got = check_reduce(cols, [0], [(None, "count"), (1, "sum_i64")])
    assert len(got) == len(values) + 1
    assert got[((0,), 1)][0]["value"] == int((valid == 0).sum())


@pytest.mark.parametrize("two_keys", [False, True], ids=["dict", "i64_dict"])
def test_dict_key_duplicate_values_merge_by_value(two_keys):
    """Equal values under different indices hash alike but differ in key bits: the
    same-hash / different-key probe branch. Partials may split by index; merged by
    value they must equal the by-value reference."""
    rng = np.random.default_rng(607)
    n = 8000
    values = [b"x", b"yy", b"x", b"", b"yy", b"x", b""]
    first = np.array([values.index(v) for v in values])
    idx = rng.integers(0, len(values), n)
    valid = nulls(rng, n, 0.1)
    other = rng.integers(0, 3, n, dtype=np.int64)
    agg = [col("f64", rng.integers(-99, 99, n).astype(np.float64), nulls(rng, n, 0.2))]
    cols = [dict_col(values, idx, valid), col("i64", other)] + agg
    ref_cols = [dict_col(values, first[idx], valid), col("i64", other)] + agg
    key_idx = [1, 0] if two_keys else [0]
    pos = key_idx.index(0)
    res, _, got = check_reduce(cols, key_idx, [(None, "count"), (2, "sum_f64"),
                                               (2, "min_f64")], exact_f64_sum=True,
                               by_value=({pos: values}, ref_cols))
    assert len(got) == (3 + 1) * (3 if two_keys else 1)
    # the premise: the partial really was grouped by index, not by value
    assert len(set(res["keys"][res["keynull"] == 0, pos].tolist())) == len(values)


def test_dict_key_single_value_dictionary():
    rng = np.random.default_rng(608)
    n = 3000
    cols = [dict_col([b"only"], np.zeros(n, dtype=np.int32), nulls(rng, n, 0.5)),
            col("f64", rng.normal(size=n))]
    _, _, got = check_reduce(cols, [0], [(1, "sum_f64"), (1, "max_f64"), (None, "count")])
    assert set(got) == {((0,), 0), ((0,), 1)}


# ---------------- 7. forced probe exhaustion, wrap, equal hashes ----------------

def test_forced_probe_exhaustion_and_wrap():
    """96 keys that all home at the LAST table slot: each block can seat at most
    probe_limit of them (the walk wraps to slot 0), the rest must spill as singletons."""
    rng = np.random.default_rng(707)
    geo = api.partial_reduce_geometry(3840)
    pool = keys_with_home_slot(geo["table_slots"] - 1, 96, geo["table_slots"])
    keys = rng.permutation(np.repeat(pool, 40))
    n = len(keys)
    assert n == 3840
    for b in range(geo["nblocks"]):  # input precondition: every block must overflow
        chunk = keys[b * geo["chunk_rows"]:(b + 1) * geo["chunk_rows"]]
        assert len(np.unique(chunk)) > geo["probe_limit"]
    cols = [col("i64", keys),
            col("i64", rng.integers(I64.min, I64.max, n, dtype=np.int64), nulls(rng, n, 0.3)),
            col("f64", rng.normal(size=n), nulls(rng, n, 0.3))]
    res, geo, _ = check_reduce(cols, [0], [(None, "count"), (1, "sum_i64"), (2, "min_f64"),
                                           (1, "max_i64")])
    # table rows <= nblocks * probe_limit, so anything beyond is a singleton spill row
    assert len(res["keynull"]) > geo["nblocks"] * geo["probe_limit"]


def test_probe_walk_wraps_past_the_table_end():
    """4 keys that all home at the LAST slot: one is seated there, the other three only
    if the walk wraps to slot 0. The key is chosen by (row offset in the block's chunk)
    mod 4, so — block sizes being wave multiples — every thread meets ONE key for good.
    Its first row claims, matches or (while other claims are unpublished) spills; once it
    claimed or matched a slot it finds that slot again on every later row. So the output
    is at most the reachable table rows plus one transient row per thread (HIP blocks
    have at most 1024). Only if duplicate claims of some keys took all probe_limit
    reachable slots before another key got one would that key spill for good — runaway
    duplicates for 4 keys. A walk stuck at the last slot seats one key and spills the
    other three quarters of the input (~98 000 rows).

    (Measured while writing this: many keys sharing a home slot do crowd each other out
    — 40 keys homed 8 slots before the end, 131 072 rows, come back as ~15 000 partial
    rows, because concurrent rows that miss an unpublished claim each take a slot of
    their own. Correct, since the final merge folds duplicates, but it is why this case
    uses 4 keys and asserts nothing of that shape.)"""
    max_block_threads = 1024
    n = 131_072
    rng = np.random.default_rng(708)
    geo = api.partial_reduce_geometry(n)
    pool = keys_with_home_slot(geo["table_slots"] - 1, 4, geo["table_slots"])
    offset = np.arange(n) % geo["chunk_rows"]
    cols = [col("i64", pool[offset % 4]),
            col("f64", rng.integers(-9, 9, n).astype(np.float64))]
    res, geo, got = check_reduce(cols, [0], [(None, "count"), (1, "sum_f64")],
                                 exact_f64_sum=True)
    assert len(got) == 4
    print(f"wrap: {len(res['keynull'])} partial rows for {n} input rows")
    assert len(res["keynull"]) <= geo["nblocks"] * (geo["probe_limit"] + max_block_threads)


def test_equal_row_hash_different_keys_stay_apart():
    """Three i64 keys crafted so that DIFFERENT key tuples share one 64-bit row hash and
    the same first key: only the full key comparison keeps the groups apart."""
    rng = np.random.default_rng(709)
    groups = []
    for a in (11, -5, 2**40):
        target = int(rng.integers(1, 2**63))
        for b in (1, 2, 3, -7):
            groups.append((a, b, colliding_third_key(a, b, target)))
    g = np.array(groups, dtype=np.int64)
    pick = rng.integers(0, len(g), 6000)
    cols = [col("i64", g[pick, 0]), col("i64", g[pick, 1]), col("i64", g[pick, 2]),
            col("i64", rng.integers(-99, 99, len(pick), dtype=np.int64))]
    h = pyref.hash_cols(cols[:3], len(pick))
    assert len(np.unique(h)) == 3 and len(np.unique(g, axis=0)) == 12  # the premise
    _, _, got = check_reduce(cols, [0, 1, 2], [(None, "count"), (3, "sum_i64"),
                                               (3, "min_i64")])
    assert len(got) == 12


# ---------------- 8. cancellation sums ----------------

def test_cancellation_sums_meet_the_summation_bound():
    rng = np.random.default_rng(808)
    half = 10_000
    a = 10.0 ** rng.uniform(-3, 12, half) * rng.choice([-1.0, 1.0], half)
    v = np.concatenate([a, -a + rng.normal(size=half) * 1e-3])
    k = np.concatenate([np.arange(half) % 16, np.arange(half) % 16]).astype(np.int64)
    p = rng.permutation(2 * half)
    cols = [col("i64", k[p]), col("f64", v[p], nulls(rng, 2 * half, 0.05))]
    _, _, got = check_reduce(cols, [0], [(1, "sum_f64"), (None, "count")])
    assert len(got) == 16


# ---------------- 9. low-cardinality effectiveness ----------------

def test_low_cardinality_never_spills():
    """6 groups: a spill needs probe_limit contiguous occupied slots, impossible without
    runaway duplicate claims — so every output row is a table row."""
    rng = np.random.default_rng(909)
    n = 131_072
    cols = [col("u8", rng.integers(0, 3, n).astype(np.uint8)),
            col("bool", rng.integers(0, 2, n).astype(np.uint8)),
            col("f64", rng.integers(0, 1000, n).astype(np.float64))]
    res, geo, got = check_reduce(cols, [0, 1], [(2, "sum_f64"), (None, "count")],
                                 exact_f64_sum=True)
    assert len(got) == 6
    assert len(res["keynull"]) <= geo["nblocks"] * geo["table_slots"]


# ---------------- fuzz ----------------

# (n, distinct values per key column): sizes around the wave width, a table that fills
# without spilling (4096 rows over 8 blocks) and, at 30 000 distinct-ish rows, blocks
# that see several times more groups than table slots
FUZZ_SHAPES = [(1000, 1), (63, 63), (65, 5), (30_000, 30_000), (4096, 4096), (1000, 300),
               (64, 5), (30_000, 300), (1, 1), (4096, 1), (30_000, 30_000), (65, 65)]


@pytest.mark.parametrize("case", range(12))
def test_fuzz_reduce(case):
    rng = np.random.default_rng(9000 + case)
    n, card = FUZZ_SHAPES[case]
    nk = int(rng.integers(1, 5))
    na = int(rng.integers(1, 5))
    cols = []
    for dt in rng.choice(["u8", "i16", "i32", "i64", "f32", "f64", "bool", "dict32"], nk):
        c = random_col(rng, n, str(dt), float(rng.choice([0, 0.1, 0.5, 1.0])))
        take = rng.integers(0, min(card, n), n)  # draw rows from a pool of `card` values
        c["data"] = np.ascontiguousarray(c["data"][take])
        cols.append(c)
    aggs = []
    for op in rng.choice(rr.OPS, na):
        op = str(op)
        if op == "count":
            aggs.append((None, op))
            continue
        cols.append(random_col(rng, n, "f64" if op.endswith("f64") else "i64",
                               float(rng.choice([0, 0.1, 0.5, 1.0]))))
        aggs.append((len(cols) - 1, op))
    res, geo, got = check_reduce(cols, list(range(nk)), aggs)
    print(f"fuzz {case}: n={n} keys={[c['dtype'] for c in cols[:nk]]} "
          f"aggs={[o for _, o in aggs]} groups={len(got)} rows={len(res['keynull'])}")
