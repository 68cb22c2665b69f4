"""Dictionary columns across the exchange and at the Arrow boundary (marked gpu, nranks=1
as in test_gpu_exchange.py: the collective is a self-exchange through RCCL send/recv). The
N>1 placement of dictionaries rests on dictgc.merge_producers_ref and the rebase test in
test_gpu_dictgc.py — the arrangement the row data already uses."""

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from datafusion_distributed_amd.arrow_boundary import partition_batches
from datafusion_distributed_amd.dictgc import decode, gc_windows_ref, merge_producers_ref

pytestmark = pytest.mark.gpu


def _dict(values):
    off = np.zeros(len(values) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in values])
    return off, np.frombuffer(b"".join(values), dtype=np.uint8)


def test_self_exchange_ships_compacted_dictionary():
    rng = np.random.default_rng(71)
    n, P, dn = 100000, 16, 3000
    doff, dbytes = _dict([b"val-%d" % i + b"\xff" * (i % 3) for i in range(dn)])
    lens = rng.integers(0, 12, n)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    cols = [
        {"dtype": "i64", "data": rng.integers(0, 10**12, n, dtype=np.int64), "valid": None},
        {"dtype": "dict32", "data": rng.integers(500, 2500, n).astype(np.int32),
         "valid": (rng.random(n) > 0.1).astype(np.uint8),
         "dict_offsets": doff, "dict_bytes": dbytes},
        {"dtype": "utf8", "data": rng.integers(97, 123, int(off[-1])).astype(np.uint8),
         "offsets": off, "valid": None},
    ]
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], P)
    part.run()
    part.sync()
    out1 = part.col_out(1)
    comm = api.Comm(api.Comm.unique_id(), 0, 1)
    plain = comm.exchange(part)
    g = api.DictGC(part, 1, n_windows=1)
    ex = comm.exchange(part, gc=[g])

    ref = gc_windows_ref(out1["data"], out1["valid"], part.row_offsets(), doff, dbytes, 1)
    want = merge_producers_ref(
        [(ref["indices"], out1["valid"], ref["offsets"][0], ref["bytes"][0])])
    d = ex.col_dict(1)
    got_idx = ex.col_data(1)["data"]
    assert np.array_equal(d["offsets"], want["offsets"]) and d["offsets"].dtype == np.int32
    assert d["bytes"].tobytes() == want["bytes"].tobytes()
    assert (d["vals_per_producer"] == want["vals_per_producer"]).all()
    assert np.array_equal(got_idx, want["indices"])
    assert len(d["offsets"]) - 1 < dn  # the dictionary really shrank (<= 2000 used)
    # decodes to what the partitioner's output decodes to with the ORIGINAL dictionary
    v = ex.col_validity(1)
    assert (v == out1["valid"]).all()
    assert decode(got_idx, v, d["offsets"], d["bytes"]) == \
        decode(out1["data"], out1["valid"], doff, dbytes)

    # non-dict columns identical to a plain exchange of the same partitioner
    assert ex.total_rows == plain.total_rows == n
    assert (ex.row_counts() == plain.row_counts()).all()
    assert (ex.col_data(0)["data"] == plain.col_data(0)["data"]).all()
    a, b = ex.col_data(2), plain.col_data(2)
    assert (a["lengths"] == b["lengths"]).all() and a["data"].tobytes() == b["data"].tobytes()
    # the plain exchange still carries the partitioner's own indices and no dictionary
    assert np.array_equal(plain.col_data(1)["data"], out1["data"])
    with pytest.raises(api.DDError):
        plain.col_dict(1)
    assert ex.stats()[1] == 0  # single rank: no egress

    # a GC with n_windows != nranks, or of another partitioner's, is rejected
    g2 = api.DictGC(part, 1, n_windows=2)
    with pytest.raises(api.DDError) as ei:
        comm.exchange(part, gc=[g2])
    assert ei.value.status == 1
    for o in (g2, g, ex, plain, comm, part):
        o.destroy()
    batch.free()


def test_boundary_batches_use_partition_dictionaries():
    import pyarrow as pa

    rng = np.random.default_rng(72)
    n, P, dn = 30000, 8, 400
    values = [b"name-%d" % i for i in range(dn)]
    doff, dbytes = _dict(values)
    idx = rng.integers(0, dn, n).astype(np.int32)
    valid = (rng.random(n) > 0.15).astype(np.uint8)
    cols = [
        {"name": "k", "dtype": "i64", "data": rng.integers(0, 10**9, n, dtype=np.int64),
         "valid": None},
        {"name": "d", "dtype": "dict32", "data": idx, "valid": valid,
         "dict_offsets": doff, "dict_bytes": dbytes},
        {"name": "v", "dtype": "f64", "data": rng.normal(size=n), "valid": None},
    ]
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], P)
    part.run()
    part.sync()
    ref = oracle.repartition(cols, [0], P)
    roff = part.row_offsets()
    tbl = pa.table({
        "k": cols[0]["data"],
        "d": pa.array([values[i].decode() if vv else None for i, vv in zip(idx, valid)]),
        "v": cols[2]["data"],
    })
    g = api.DictGC(part, 1, n_windows=P)
    seen = 0
    for p, rb in partition_batches(part, 0, P, batch_size=1024, gc={1: g}):
        order = ref["order"][seen: seen + rb.num_rows]
        expected = tbl.take(pa.array(order))
        col = rb.column(1)
        assert pa.types.is_dictionary(col.type)
        got = pa.table({"k": rb.column(0), "d": col.cast(pa.string()), "v": rb.column(2)})
        assert got.equals(expected), f"partition {p} batch mismatch"
        prow = ref["order"][int(roff[p]): int(roff[p + 1])]
        used = np.unique(idx[prow][valid[prow].astype(bool)])
        assert len(col.dictionary) == len(used)
        assert col.dictionary.to_pylist() == [values[i].decode() for i in used]
        seen += rb.num_rows
    assert seen == n
    # without gc the output is unchanged: every batch carries the full dictionary
    for p, rb in partition_batches(part, 0, 2, batch_size=4096):
        assert len(rb.column(1).dictionary) == dn
    with pytest.raises(ValueError):  # one dictionary per partition is required
        g1 = api.DictGC(part, 1, n_windows=1)
        try:
            next(partition_batches(part, 0, P, gc={1: g1}))
        finally:
            g1.destroy()
    g.destroy()
    part.destroy()
    batch.free()
