"""Decimal128 columns through the shuffle (marked gpu): a dec128 column is
an opaque 16-byte value [lo, hi] that hashes as the two i64 keys (lo, hi) and scatters as
one 16-byte element. The reference for every case is the UNMODIFIED CPU oracle run on the
split form of the batch (each dec128 column replaced by its i64 halves, sharing its
validity), with the two scattered halves interleaved again.

Every case pins the scatter tier with Partitioner.info() before it compares: a batch with a
16-byte column is refused by the pre / wide / HL / rhash / compile-time-column-count tiers
and lands on the generic staged kernel (path 1) or, past DD_STAGE_MAXC columns, on v1."""

import decimal

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api

pytestmark = pytest.mark.gpu

N = 70_001  # 8 tiles of 8 751 rows: more than two rounds each, ragged last round


def dec(rng, n, null_p=None, lo=None):
    """Random dec128 column: lo random, hi drawn per row from {0, 1, -1, random}, so that
    routing and data depend on both halves. null_p: None = no validity buffer, else the
    fraction of null rows (0.0 = buffer present, none null; 1.0 = all null)."""
    data = np.empty((n, 2), dtype=np.uint64)
    data[:, 0] = rng.integers(0, 2**64, n, dtype=np.uint64) if lo is None else lo
    rnd = rng.integers(0, 2**64, n, dtype=np.uint64)
    kind = rng.integers(0, 4, n)
    data[:, 1] = np.choose(kind, [np.uint64(0), np.uint64(1), np.uint64(2**64 - 1), rnd])
    valid = None if null_p is None else (rng.random(n) >= null_p).astype(np.uint8)
    return {"dtype": "dec128", "data": data, "valid": valid}


def i64(rng, n):
    return {"dtype": "i64", "data": rng.integers(-(2**62), 2**62, n, dtype=np.int64),
            "valid": None}


def i32(rng, n, null_p=None):
    valid = None if null_p is None else (rng.random(n) >= null_p).astype(np.uint8)
    return {"dtype": "i32", "data": rng.integers(-(2**31), 2**31, n, dtype=np.int64)
            .astype(np.int32), "valid": valid}


def f64(rng, n):
    return {"dtype": "f64", "data": rng.normal(size=n), "valid": None}


def utf8(rng, n, maxlen):
    lens = rng.integers(0, maxlen + 1, n)
    lens[0] = maxlen
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    return {"dtype": "utf8", "offsets": off, "valid": None,
            "data": rng.integers(97, 123, int(off[-1]), dtype=np.int64).astype(np.uint8)}


def split_ref(cols, key_idx, nparts):
    """Oracle result for `cols` through the split form: dec128 -> (lo i64, hi i64) sharing
    the validity, key index expanded to the pair in (lo, hi) order, outputs interleaved."""
    split, pos = [], []
    for c in cols:
        pos.append(len(split))
        if c["dtype"] == "dec128":
            halves = np.ascontiguousarray(c["data"]).view(np.int64).reshape(-1, 2)
            for h in range(2):
                split.append({"dtype": "i64", "data": np.ascontiguousarray(halves[:, h]),
                              "valid": c.get("valid")})
        else:
            split.append(c)
    keys = []
    for k in key_idx:
        keys.append(pos[k])
        if cols[k]["dtype"] == "dec128":
            keys.append(pos[k] + 1)
    ref = oracle.repartition(split, keys, nparts)
    out = []
    for c, p in zip(cols, pos):
        oc = ref["cols"][p]
        if c["dtype"] == "dec128":
            both = np.stack([oc["data"], ref["cols"][p + 1]["data"]], axis=1)
            oc = {"dtype": "dec128", "data": np.ascontiguousarray(both).view(np.uint64),
                  "valid": oc.get("valid")}
        out.append(oc)
    return {"pid": ref["pid"], "order": ref["order"], "part_offsets": ref["part_offsets"],
            "cols": out}


def compare(part, cols, ref):
    n = part.batch.n_rows
    pd = part.pids()
    assert pd is not None, "a dec128 batch never takes the rhash form"
    if n:
        assert (pd == ref["pid"]).all(), "partition ids differ"
    assert (part.row_offsets() == ref["part_offsets"]).all(), "row offsets differ"
    for i, col in enumerate(cols):
        got, exp = part.col_out(i), ref["cols"][i]
        if col["dtype"] == "utf8":
            assert (got["lengths"] == exp["lengths"]).all(), f"col {i} lengths differ"
            assert got["data"].tobytes() == exp["data"].tobytes(), f"col {i} bytes differ"
        elif col["dtype"] == "dec128":
            assert got["data"].dtype == np.uint64 and got["data"].shape == (n, 2)
            assert np.array_equal(got["data"], exp["data"]), f"col {i} dec128 data differ"
        else:
            assert got["data"].tobytes() == exp["data"].tobytes(), f"col {i} data differ"
        if col.get("valid") is not None:
            assert (got["valid"] == exp["valid"]).all(), f"col {i} validity differs"


def check(cols, key_idx, nparts, expect, k1_spec=None):
    """create / pin the tier / run / compare / destroy; returns info()."""
    ref = split_ref(cols, key_idx, nparts)
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        info = part.info()
        for name, want in expect.items():
            good = want(info[name]) if callable(want) else info[name] == want
            assert good, f"info()[{name!r}] = {info[name]}, not the tier named: {info}"
        if k1_spec is not None:
            assert part.k1_spec() == k1_spec
        assert part.pre_layout() == 0
        part.run()
        part.sync()
        compare(part, cols, ref)
        return info
    finally:
        part.destroy()
        batch.free()


STAGED = {"path": 1, "hl": 0, "rhash": 0}


# 1. staged, payload
@pytest.mark.parametrize("nparts", [1, 7, 128, 1000, 2048])
def test_staged_payload(nparts):
    rng = np.random.default_rng(1600 + nparts)
    check([i64(rng, N), dec(rng, N), i32(rng, N)], [0], nparts, STAGED)


# 2. the shapes whose gates tested only elem == 0
@pytest.mark.parametrize("env", [{}, {"DD_RHASH": "1"}, {"DD_K3_HL": "0"},
                                 {"DD_K3_PRE": "0"}],
                         ids=["default", "rhash", "nohl", "nopre"])
@pytest.mark.parametrize("shape", ["d884", "8d844"])
def test_shapes_old_gates_would_misroute(shape, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(1610)
    if shape == "d884":
        cols, key = [dec(rng, N), i64(rng, N), i64(rng, N), i32(rng, N)], [1]
    else:
        cols, key = [i64(rng, N), dec(rng, N), f64(rng, N), i32(rng, N), i32(rng, N)], [0]
    check(cols, key, 128, STAGED)


# 3. validity
@pytest.mark.parametrize("null_p", [0.1, 1.0, 0.0], ids=["10pct", "allnull", "nonenull"])
def test_validity(null_p):
    rng = np.random.default_rng(1620)
    check([i64(rng, N), dec(rng, N, null_p), i32(rng, N, null_p)], [0], 128, STAGED)


# 4. with strings
@pytest.mark.parametrize("env,expect", [
    ({}, {"path": 1, "k5": 1, "hl": 0, "rhash": 0}),
    ({"DD_K5": "0"}, {"path": 1, "k5": 0, "hl": 0, "rhash": 0}),
    ({"DD_V2_VAR": "0"}, {"path": 0}),
], ids=["k5", "k4", "v1"])
def test_with_strings(env, expect, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(1630)
    check([i64(rng, N), dec(rng, N, 0.1), utf8(rng, N, 12)], [0], 16, expect)


# 5. v1 by column count
@pytest.mark.parametrize("nparts", [7, 300])
def test_v1_nine_columns(nparts):
    rng = np.random.default_rng(1640)
    cols = [i64(rng, N), dec(rng, N), i32(rng, N), dec(rng, N, 0.1), f64(rng, N),
            i32(rng, N, 0.2), dec(rng, N), i64(rng, N), i32(rng, N)]
    check(cols, [0], nparts, {"path": 0})


# 6. many wide columns: whatever wpb / gmax the cascade picks, LDS fits and it is exact
@pytest.mark.parametrize("ndec,nparts", [(4, 128), (7, 16)])
def test_many_wide_columns(ndec, nparts):
    rng = np.random.default_rng(1650 + ndec)
    cols = [i64(rng, N)] + [dec(rng, N) for _ in range(ndec)]
    info = check(cols, [0], nparts, STAGED)
    # the staged image: partition arrays + scan scratch + R rows of (dstg + row bytes)
    wpb, R = info["wpb"], info["round_rows"]
    lds = nparts * (16 + 4 * wpb) + 4 * 64 * wpb + R * (4 + 8 + 16 * ndec)
    assert lds <= 160 * 1024, info


# 7. keys
@pytest.mark.parametrize("case", ["single", "dec_i32", "i32_dec", "nullable", "hi_only"])
def test_keys(case):
    rng = np.random.default_rng(1670)
    if case == "single":
        cols, key = [dec(rng, N), i32(rng, N)], [0]
    elif case == "dec_i32":
        cols, key = [dec(rng, N), i32(rng, N), i64(rng, N)], [0, 1]
    elif case == "i32_dec":
        cols, key = [dec(rng, N), i32(rng, N), i64(rng, N)], [1, 0]
    elif case == "nullable":  # null rows route by the other key only
        cols, key = [dec(rng, N, 0.3), i32(rng, N), i64(rng, N)], [0, 1]
    else:  # lo constant: only hi separates the rows
        cols, key = [dec(rng, N, lo=np.uint64(12345)), i32(rng, N)], [0]
        cols[0]["data"][:, 1] = rng.integers(0, 2**64, N, dtype=np.uint64)
    ref = split_ref(cols, key, 128)
    assert len(np.unique(ref["pid"])) == 128
    check(cols, key, 128, STAGED, k1_spec=0)


# 8. edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_edges(n):
    rng = np.random.default_rng(1680 + n)
    check([dec(rng, n, 0.2), i64(rng, n), i32(rng, n)], [0, 1], 7, STAGED, k1_spec=0)


# 9. reuse: refill with new decimals and new validity; phase-split run
def test_refill_and_phase_split():
    rng = np.random.default_rng(1690)
    a = [i64(rng, N), dec(rng, N, 0.1), i32(rng, N)]
    b = [i64(rng, N), dec(rng, N, 0.5), i32(rng, N)]
    ref_a, ref_b = split_ref(a, [0, 1], 128), split_ref(b, [0, 1], 128)
    batch = api.DeviceBatch(a)
    part = api.Partitioner(batch, [0, 1], 128)
    try:
        assert part.info()["path"] == 1
        part.run()
        part.sync()
        compare(part, a, ref_a)
        batch.refill(b)
        part.run()
        part.sync()
        compare(part, b, ref_b)
        batch.refill(a)
        part.run_phase1()
        part.run_phase2()
        part.sync()
        compare(part, a, ref_a)
    finally:
        part.destroy()
        batch.free()


# 10. orchestration
def test_chunked_cuts_mid_partition():
    from datafusion_distributed_amd.chunked import chunked_partition

    rng = np.random.default_rng(1700)
    n = 60_000
    cols = [i64(rng, n), dec(rng, n, 0.1), i32(rng, n)]
    ref = split_ref(cols, [0], 16)
    res = chunked_partition(cols, [0], 16, max_chunk_rows=20_000)
    assert res["n_chunks"] == 3
    assert (res["part_row_offsets"] == ref["part_offsets"]).all()
    assert res["cols"][1]["data"].shape == (n, 2)
    for i in range(3):
        assert res["cols"][i]["data"].tobytes() == ref["cols"][i]["data"].tobytes()
    assert (res["cols"][1]["valid"] == ref["cols"][1]["valid"]).all()


def test_two_level_ranged():
    from datafusion_distributed_amd.twolevel import two_level_partition

    rng = np.random.default_rng(1710)
    n = 50_000
    cols = [i64(rng, n), dec(rng, n, 0.1), utf8(rng, n, 20)]
    ref = split_ref(cols, [0, 1], 64)
    res = two_level_partition(cols, [0, 1], 64, buckets=4)
    assert (res["part_row_offsets"] == ref["part_offsets"]).all()
    assert res["cols"][0]["data"].tobytes() == ref["cols"][0]["data"].tobytes()
    assert np.array_equal(res["cols"][1]["data"], ref["cols"][1]["data"])
    assert (res["cols"][1]["valid"] == ref["cols"][1]["valid"]).all()
    assert (res["cols"][2]["lengths"] == ref["cols"][2]["lengths"]).all()
    assert res["cols"][2]["data"].tobytes() == ref["cols"][2]["data"].tobytes()


# 11. exchange (world 1: the collective sends to itself; one communicator per collective,
# as in test_gpu_exchange.py / test_gpu_broadcast.py)
@pytest.fixture(scope="module")
def exchange_case():
    rng = np.random.default_rng(1720)
    n, P = 30_000, 16
    cols = [i64(rng, n), dec(rng, n, 0.1), i32(rng, n)]
    return cols, P, split_ref(cols, [0], P)


@pytest.mark.parametrize("op", ["exchange", "coalesce"])
def test_self_exchange_and_coalesce(op, exchange_case):
    cols, P, ref = exchange_case
    n = len(cols[0]["data"])
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], P)
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    try:
        part.run()
        part.sync()
        compare(part, cols, ref)
        ex = comm.exchange(part) if op == "exchange" else comm.coalesce(part, 1)
        assert ex.total_rows == n
        got = ex.col_data(1)
        assert got["dtype"] == "dec128" and got["data"].shape == (n, 2)
        assert np.array_equal(got["data"], ref["cols"][1]["data"])
        assert (ex.col_validity(1) == ref["cols"][1]["valid"]).all()
        assert ex.col_data(0)["data"].tobytes() == ref["cols"][0]["data"].tobytes()
        assert ex.col_data(2)["data"].tobytes() == ref["cols"][2]["data"].tobytes()
        ex.destroy()
    finally:
        comm.destroy()
        part.destroy()
        batch.free()


def test_self_broadcast(exchange_case):
    cols, _, _ = exchange_case
    n = len(cols[0]["data"])
    batch = api.DeviceBatch(cols)
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    try:
        bc = comm.broadcast(batch, root=0)
        assert bc.n_rows == n and bc.n_cols == 3
        c1 = bc.col(1)
        assert c1["dtype"] == "dec128" and np.array_equal(c1["data"], cols[1]["data"])
        assert (c1["valid"] == cols[1]["valid"]).all()
        assert (bc.col(2)["data"] == cols[2]["data"]).all()
        bc.destroy()
    finally:
        comm.destroy()
        batch.free()


# 12. Arrow boundary
def test_arrow_boundary_decimal128():
    import pyarrow as pa

    from datafusion_distributed_amd import arrow_boundary

    rng = np.random.default_rng(1730)
    n, P = 5000, 7
    cents = rng.integers(-(10**13), 10**13, n)
    nulls = rng.random(n) < 0.1
    typ = pa.decimal128(15, 2)
    arr = pa.array([None if z else decimal.Decimal(int(c)).scaleb(-2)
                    for c, z in zip(cents, nulls)], type=typ)
    col = api.dec128_col(arr)
    assert col["precision"] == 15 and col["scale"] == 2
    cols = [i64(rng, n), col]
    ref = split_ref(cols, [0], P)
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], P)
    try:
        part.run()
        part.sync()
        pieces = {p: [] for p in range(P)}
        for p, rb in arrow_boundary.partition_batches(part, 0, P, batch_size=1000):
            assert rb.num_rows <= 1000 and rb.column(1).type == typ
            pieces[p].append(rb.column(1))
        poff = ref["part_offsets"]
        for p in range(P):
            got = pa.concat_arrays(pieces[p])
            rows = ref["order"][poff[p]:poff[p + 1]]
            want = arr.take(pa.array(rows, type=pa.int64()))
            assert got.equals(want), f"partition {p} differs from take()"
            assert got.null_count == want.null_count
    finally:
        part.destroy()
        batch.free()


# 13. rejections
def test_partial_reduce_rejects_dec128():
    rng = np.random.default_rng(1740)
    n = 1000
    batch = api.DeviceBatch([i64(rng, n), dec(rng, n)])
    try:
        with pytest.raises(api.DDError) as ei:
            api.partial_reduce(batch, [1], [(None, "count")])
        assert ei.value.status == 6 and "dec128" in str(ei.value)  # DD_ERR_UNSUPPORTED
        with pytest.raises(api.DDError) as ei:
            api.partial_reduce(batch, [0], [(1, "sum_i64")])
        assert ei.value.status == 6 and "dec128" in str(ei.value)
    finally:
        batch.free()


def test_misaligned_data_pointer_is_invalid():
    rng = np.random.default_rng(1750)
    batch = api.DeviceBatch([i64(rng, 100), dec(rng, 100)])
    try:
        batch.desc.cols[1].data += 8  # still inside the buffer, but not 16-byte aligned
        with pytest.raises(api.DDError) as ei:
            api.Partitioner(batch, [0], 4)
        assert ei.value.status == 1 and "aligned" in str(ei.value)  # DD_ERR_INVALID
    finally:
        batch.free()
