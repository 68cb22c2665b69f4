"""CPU tests of the partial-aggregation reference model (oracle/reduce_ref.py) and of the
geometry accessor. The model judges the GPU kernel in test_gpu_reduce_parity.py, so it
earns trust here first: against pyarrow where pyarrow's semantics coincide with the
contract, against hand-written totalOrder vectors where they do not, and final_merge
against reduce_ref on synthetic partials."""

import math
import struct

import numpy as np
import pytest

from datafusion_distributed_amd import api
from oracle import reduce_ref as rr


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


NEG_QNAN = 0xFFF8000000000000
POS_QNAN = 0x7FF8000000000000
PAYLOAD_NAN = 0x7FF8000000000123
SUBNORMAL = 0x0000000000000001
# -NaN < -inf < -1 < -0.0 < +0.0 < subnormal < 1 < +inf < +NaN
TOTAL_ORDER = [NEG_QNAN, f64_bits(-math.inf), f64_bits(-1.0), f64_bits(-0.0),
               f64_bits(0.0), SUBNORMAL, f64_bits(1.0), f64_bits(math.inf), POS_QNAN]


def test_total_order_hand_vectors():
    keys = [rr.total_order_key(b) for b in TOTAL_ORDER]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    ranks = rr.total_order_rank(np.array(TOTAL_ORDER, dtype=np.uint64)).tolist()
    assert ranks == sorted(ranks) and len(set(ranks)) == len(ranks)
    assert [rr.rank_to_bits(r) for r in ranks] == TOTAL_ORDER
    # payload NaN sorts above the plain quiet NaN of the same sign, mirrored when sign-set
    assert rr.total_order_key(PAYLOAD_NAN) > rr.total_order_key(POS_QNAN)
    assert rr.total_order_key(PAYLOAD_NAN | (1 << 63)) < rr.total_order_key(NEG_QNAN)


def test_total_order_rank_agrees_with_scalar_key_on_random_bits():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2**64, 2000, dtype=np.uint64)
    bits = np.concatenate([bits, np.array(TOTAL_ORDER, dtype=np.uint64)])
    by_rank = bits[np.argsort(rr.total_order_rank(bits), kind="stable")].tolist()
    by_key = sorted(bits.tolist(), key=rr.total_order_key)
    assert by_rank == by_key
    # and finite non-NaN values order numerically
    vals = rng.normal(size=500)
    r = rr.total_order_rank(vals.view(np.uint64))
    assert (np.argsort(r) == np.argsort(vals)).all()


def test_min_max_f64_total_order_one_group():
    data = np.array(TOTAL_ORDER, dtype=np.uint64).view(np.float64)
    rng = np.random.default_rng(5)
    data = data[rng.permutation(len(data))]
    cols = [{"dtype": "i32", "data": np.zeros(len(data), np.int32), "valid": None},
            {"dtype": "f64", "data": data, "valid": None}]
    (gid, ent), = rr.reduce_ref(cols, [0], [(1, "min_f64"), (1, "max_f64")]).items()
    assert gid == ((0,), 0)
    assert ent[0]["value"] == NEG_QNAN and ent[1]["value"] == POS_QNAN
    # only zeros: min is -0.0, max is +0.0, by bits
    z = np.array([0.0, -0.0, 0.0, -0.0])
    cols[0]["data"] = np.zeros(4, np.int32)
    cols[1]["data"] = z
    (_, ent), = rr.reduce_ref(cols, [0], [(1, "min_f64"), (1, "max_f64")]).items()
    assert ent[0]["value"] == f64_bits(-0.0) and ent[1]["value"] == f64_bits(0.0)


def test_sum_i64_wraps_and_int_extremes():
    i64 = np.iinfo(np.int64)
    v = np.array([i64.max, 1, i64.max, i64.min, 5], dtype=np.int64)
    k = np.array([0, 0, 1, 2, 2], dtype=np.int64)
    cols = [{"dtype": "i64", "data": k, "valid": None},
            {"dtype": "i64", "data": v, "valid": None}]
    got = rr.reduce_ref(cols, [0], [(1, "sum_i64"), (1, "min_i64"), (1, "max_i64")])
    assert got[((0,), 0)][0]["value"] == i64.min  # MAX + 1 wraps
    assert got[((1,), 0)][0]["value"] == i64.max
    assert got[((2,), 0)][0]["value"] == i64.min + 5
    assert got[((2,), 0)][1]["value"] == i64.min and got[((2,), 0)][2]["value"] == 5


def test_float_and_null_key_identity():
    nan2 = np.array([0x7FF0000000000001, 0xFFF8000000000000, POS_QNAN],
                    dtype=np.uint64).view(np.float64)
    k = np.concatenate([[0.0, -0.0, 1.5], nan2, [7.0]])
    valid = np.ones(len(k), np.uint8)
    valid[-1] = 0  # NULL key with a non-zero payload underneath
    cols = [{"dtype": "f64", "data": k, "valid": valid}]
    got = rr.reduce_ref(cols, [0], [(None, "count")])
    assert {g: e[0]["value"] for g, e in got.items()} == {
        ((0,), 0): 2, ((f64_bits(1.5),), 0): 1, ((POS_QNAN,), 0): 3, ((0,), 1): 1}


def _arrow_table(k, kvalid, cols):
    import pyarrow as pa

    arrays = {"k": pa.array(k, mask=None if kvalid is None else ~kvalid.astype(bool))}
    for name, (data, valid) in cols.items():
        arrays[name] = pa.array(data, mask=None if valid is None else ~valid.astype(bool))
    return pa.table(arrays)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reduce_ref_matches_pyarrow_where_semantics_coincide(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    k = rng.integers(-3, 9, n, dtype=np.int64).astype(np.int32)
    kvalid = (rng.random(n) > 0.1).astype(np.uint8)
    f = rng.normal(size=n) * 100  # NaN-free: pyarrow min/max skip NaN
    i = rng.integers(-(2**40), 2**40, n, dtype=np.int64)  # no overflow
    fvalid = (rng.random(n) > 0.3).astype(np.uint8)
    ivalid = (rng.random(n) > 0.3).astype(np.uint8)
    fvalid[k == 4] = 0  # an all-null group (per aggregate column)
    ivalid[k == 5] = 0
    cols = [{"dtype": "i32", "data": k, "valid": kvalid},
            {"dtype": "f64", "data": f, "valid": fvalid},
            {"dtype": "i64", "data": i, "valid": ivalid}]
    aggs = [(None, "count"), (2, "sum_i64"), (2, "min_i64"), (2, "max_i64"),
            (1, "min_f64"), (1, "max_f64"), (1, "sum_f64")]
    got = rr.reduce_ref(cols, [0], aggs)
    direct = _arrow_table(k, kvalid, {"f": (f, fvalid), "i": (i, ivalid)}) \
        .group_by("k").aggregate([([], "count_all"), ("i", "sum"), ("i", "min"),
                                  ("i", "max"), ("f", "min"), ("f", "max"), ("f", "sum"),
                                  ("f", "count"), ("i", "count")])
    assert len(got) == direct.num_rows
    saw_null = False
    for r in range(direct.num_rows):
        kv = direct["k"][r].as_py()
        gid = ((0,), 1) if kv is None else ((int(np.uint32(np.int32(kv))),), 0)
        e = got[gid]
        assert e[0]["value"] == direct["count_all"][r].as_py()
        assert e[1]["value"] == direct["i_sum"][r].as_py()
        assert e[2]["value"] == direct["i_min"][r].as_py()
        assert e[3]["value"] == direct["i_max"][r].as_py()
        for gi, name in ((4, "f_min"), (5, "f_max")):
            want = direct[name][r].as_py()
            assert e[gi]["value"] == (None if want is None else f64_bits(want))
        want = direct["f_sum"][r].as_py()
        if want is None:
            assert e[6]["value"] is None
            saw_null = True
        else:
            assert abs(e[6]["value"] - want) <= e[6]["n_nonnull"] * 2.0**-52 * e[6]["abs_sum"]
        assert e[6]["nn"] == e[4]["nn"] == direct["f_count"][r].as_py()
        assert e[1]["nn"] == direct["i_count"][r].as_py()
    assert saw_null


def synthetic_partial(cols, key_idx, aggs, cuts):
    """What a partial-aggregation pass may emit: reduce_ref per arbitrary row chunk, the
    chunks' groups concatenated (so groups repeat), in api.partial_reduce's layout."""
    n = len(cols[0]["data"])
    edges = [0] + list(cuts) + [n]
    keys, keynull, vals, nns = [], [], [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        chunk = [dict(c, data=c["data"][lo:hi],
                      valid=None if c.get("valid") is None else c["valid"][lo:hi])
                 for c in cols]
        for (bits, mask), ent in rr.reduce_ref(chunk, key_idx, aggs).items():
            keys.append(bits)
            keynull.append(mask)
            row = []
            for e in ent:
                v = e["value"]
                if e["op"] in rr.INT_OPS:
                    row.append(struct.unpack("<d", struct.pack("<q", 0 if v is None else v))[0])
                elif e["op"] == "sum_f64":
                    row.append(0.0 if v is None else v)
                else:  # *_f64 min/max: bit pattern; a NULL partial carries garbage
                    row.append(struct.unpack("<d", struct.pack("<Q", POS_QNAN if v is None
                                                                 else v))[0])
            vals.append(row)
            nns.append([e["nn"] for e in ent])
    nk, na = len(key_idx), len(aggs)
    return {"keys": np.array(keys, dtype=np.uint64).reshape(-1, nk),
            "keynull": np.array(keynull, dtype=np.uint32),
            "aggs": np.array(vals, dtype=np.float64).reshape(-1, na),
            "nn": np.array(nns, dtype=np.uint64).reshape(-1, na)}


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_final_merge_of_synthetic_partials_reproduces_reduce_ref(seed):
    rng = np.random.default_rng(seed)
    n = 3000
    k0 = rng.integers(0, 6, n, dtype=np.int64).astype(np.int16)
    k1 = rng.normal(size=n).round(0).astype(np.float32)  # few distinct, incl. +-0.0
    k1valid = (rng.random(n) > 0.2).astype(np.uint8)
    # integer-valued doubles: chunked fsum-of-fsums stays exact, so equality must be exact
    f = rng.integers(-1000, 1000, n).astype(np.float64)
    special = np.array(TOTAL_ORDER + [PAYLOAD_NAN], dtype=np.uint64).view(np.float64)
    m = rng.normal(size=n)
    m[rng.integers(0, n, 60)] = special[rng.integers(0, len(special), 60)]
    i = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64)
    fvalid = (rng.random(n) > 0.3).astype(np.uint8)
    fvalid[k0 == 2] = 0
    cols = [{"dtype": "i16", "data": k0, "valid": None},
            {"dtype": "f32", "data": k1, "valid": k1valid},
            {"dtype": "f64", "data": f, "valid": fvalid},
            {"dtype": "f64", "data": m, "valid": fvalid},
            {"dtype": "i64", "data": i, "valid": fvalid}]
    cuts = sorted(rng.choice(np.arange(1, n), 9, replace=False).tolist())
    for aggs in ([(None, "count"), (2, "sum_f64"), (3, "min_f64"), (3, "max_f64")],
                 [(4, "sum_i64"), (4, "min_i64"), (4, "max_i64"), (None, "count")]):
        ops = [o for _, o in aggs]
        want = rr.reduce_ref(cols, [0, 1], aggs)
        part = synthetic_partial(cols, [0, 1], aggs, cuts)
        assert len(part["keynull"]) > len(want)  # duplicates really were emitted
        got = rr.final_merge(part, ops)
        assert got.keys() == want.keys()
        for gid, went in want.items():
            for ge, we in zip(got[gid], went):
                assert ge["op"] == we["op"] and ge["nn"] == we["nn"], (gid, ge, we)
                assert ge["value"] == we["value"], (gid, ge, we)
        assert any(e[1]["value"] is None for e in want.values())


def test_merge_dict_by_value_collapses_duplicate_values():
    values = [b"a", b"", b"a", b"b"]  # index 0 and 2 hold the same value
    idx = np.array([0, 2, 1, 3, 2, 0, 1], dtype=np.int32)
    valid = np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)
    v = np.array([1, 2, 4, 8, 16, 32, 64], dtype=np.int64)
    doff = np.array([0, 1, 1, 2, 3], dtype=np.int32)
    cols = [{"dtype": "dict32", "data": idx, "valid": valid,
             "dict_bytes": np.frombuffer(b"aab", np.uint8), "dict_offsets": doff},
            {"dtype": "i64", "data": v, "valid": None}]
    by_index = rr.reduce_ref(cols, [0], [(1, "sum_i64"), (None, "count"), (1, "max_i64")])
    assert len(by_index) == 5
    by_value = rr.merge_dict_by_value(by_index, {0: values})
    assert {g: [e["value"] for e in ent] for g, ent in by_value.items()} == {
        ((b"a",), 0): [51, 4, 32], ((b"",), 0): [4, 1, 4], ((b"b",), 0): [8, 1, 8],
        ((0,), 1): [64, 1, 64]}


def test_fsum_ext_non_finite():
    assert math.isnan(rr.fsum_ext([1.0, math.nan]))
    assert math.isnan(rr.fsum_ext([math.inf, -math.inf]))
    assert rr.fsum_ext([math.inf, 1.0]) == math.inf
    assert rr.fsum_ext([1e308, 1e308]) == math.inf
    assert rr.fsum_ext([1e16, 1.0, -1e16]) == 1.0


def test_partial_reduce_geometry_recorded_values():
    """Recorded facts of today's kernel geometry: 1024 LDS slots per block, probe limit
    64, max(8, min(1024, ceil(n / 16384))) blocks of ceil(n / nblocks) rows. Tests that
    reason about spills take these from the accessor, not from literals of their own."""
    for n in [0, 1, 7, 8, 257, 131072, 131073, 150001, 16384 * 1024, 16384 * 1024 + 1,
              10**10]:
        g = api.partial_reduce_geometry(n)
        assert g["table_slots"] == 1024 and g["probe_limit"] == 64
        nb = max(8, min(1024, -(-n // 16384)))
        assert g["nblocks"] == nb
        assert g["chunk_rows"] == -(-n // nb)
        assert g["nblocks"] * g["chunk_rows"] >= n
    with pytest.raises(api.DDError):
        api.partial_reduce_geometry(-1)
