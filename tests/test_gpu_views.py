"""View columns on the device (marked gpu): dd_view_ingest_run / dd_view_emit_run compared
bit for bit with the numpy models views.ingest_ref / views.emit_ref (themselves pinned to
pyarrow's cast in test_views_cpu.py), on both copy tiers, and carried through the
partitioner. Everything is a pure function of the inputs, so every comparison is exact.
Shapes are the smallest that reach each path: row counts around the 64-lane wave and the
copy tile, lengths around the 12-byte inline limit, one tile that outgrows the LDS image."""

import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_distributed_amd import api, arrow_boundary
from datafusion_distributed_amd.views import emit_ref, from_arrow, ingest_ref, to_arrow

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 4, 11, 12, 13, 64, 300]
T = api.view_tile_rows()
# DD_VIEW_LDS: unset = the default (direct, the tier that measured faster), "0" forces
# direct, "1" asks for the LDS-staged tier
TIERS = [pytest.param(None, id="unset"), pytest.param("0", id="direct"),
         pytest.param("1", id="lds")]


def _set_tier(monkeypatch, knob):
    """Set the knob; returns the tier a run must then report (unless every tile outgrows
    the LDS image)."""
    if knob is None:
        monkeypatch.delenv("DD_VIEW_LDS", raising=False)
    else:
        monkeypatch.setenv("DD_VIEW_LDS", knob)
    return 1 if knob == "1" else 0


def _rand_values(rng, n, lengths=LENGTHS, lo=97, hi=123):
    return [bytes(rng.integers(lo, hi, int(rng.choice(lengths)), dtype=np.uint8))
            for _ in range(n)]


def _make_views(rng, values, n_bufs, null_frac=0.0):
    """Hand-built views over n_bufs data buffers: long values are scattered over the
    buffers in shuffled order with junk between them; nulls get a garbage view (length
    0x7fffffff, buffer_index 99) that must never be interpreted."""
    n = len(values)
    views = np.zeros((n, 16), dtype=np.uint8)
    words = views.view(np.int32).reshape(n, 4)
    chunks = [[b"\xee" * 3] for _ in range(n_bufs)]
    sizes = [3] * n_bufs
    for i in rng.permutation(n):
        v = values[i]
        words[i, 0] = len(v)
        if len(v) <= 12:
            views[i, 4:4 + len(v)] = np.frombuffer(v, dtype=np.uint8)
            continue
        assert n_bufs > 0
        b = int(rng.integers(0, n_bufs))
        views[i, 4:8] = np.frombuffer(v[:4], dtype=np.uint8)
        words[i, 2] = b
        words[i, 3] = sizes[b]
        chunks[b] += [v, b"\xdd"]
        sizes[b] += len(v) + 1
    bufs = [np.frombuffer(b"".join(c), dtype=np.uint8) for c in chunks]
    valid = None
    if null_frac > 0:
        valid = (rng.random(n) >= null_frac).astype(np.uint8)
        words[valid == 0] = [0x7FFFFFFF, -1, 99, -7]
    return views, valid, bufs


def _ingest_and_check(views, valid, bufs, want_tier):
    want_off, want_data = ingest_ref(views, valid, bufs)
    ing = api.ViewIngest.from_host(views, valid, bufs)
    try:
        assert ing.tier() == want_tier
        assert ing.data_len == len(want_data)
        assert np.array_equal(ing.offsets(), want_off)
        assert ing.bytes().tobytes() == want_data.tobytes()
    finally:
        ing.destroy()


# ---------------- ingest ----------------

@pytest.mark.parametrize("knob", TIERS)
@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_ingest_row_counts(n_rows, knob, monkeypatch):
    tier = _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(1000 + n_rows)
    views, valid, bufs = _make_views(rng, _rand_values(rng, n_rows), 3, null_frac=0.1)
    _ingest_and_check(views, valid, bufs, tier)


@pytest.mark.parametrize("knob", TIERS)
@pytest.mark.parametrize("n_bufs", [0, 1, 3])
def test_ingest_buffer_counts(n_bufs, knob, monkeypatch):
    tier = _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(20 + n_bufs)
    lengths = LENGTHS if n_bufs else [0, 1, 4, 11, 12]
    views, valid, bufs = _make_views(rng, _rand_values(rng, T + 70, lengths), n_bufs)
    _ingest_and_check(views, valid, bufs, tier)


@pytest.mark.parametrize("knob", TIERS)
def test_ingest_aliasing_and_reversed_views(knob, monkeypatch):
    tier = _set_tier(monkeypatch, knob)
    n = T + 9
    buf = np.arange(64, dtype=np.uint8)
    views = np.zeros((n, 16), dtype=np.uint8)
    words = views.view(np.int32).reshape(n, 4)
    words[:, 0] = 20  # every row points at the same 20 bytes
    views[:, 4:8] = buf[7:11]
    words[:, 3] = 7
    _ingest_and_check(views, None, [buf], tier)
    # reversed: row i reads the i-th 13-byte value from the END of the buffer
    big = np.random.default_rng(5).integers(0, 256, 13 * n, dtype=np.uint8)
    words[:, 0] = 13
    words[:, 3] = 13 * (n - 1 - np.arange(n))
    views[:, 4:8] = big.reshape(n, 13)[::-1, :4]
    _ingest_and_check(views, None, [big], tier)


@pytest.mark.parametrize("knob", TIERS)
def test_ingest_pyarrow_sliced_and_binary(knob, monkeypatch):
    tier = _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(31)
    vals = [v.decode() for v in _rand_values(rng, 700)]
    for i in np.flatnonzero(rng.random(700) < 0.1):
        vals[i] = None
    arr = pa.concat_arrays([pa.array(vals[:300], type=pa.string_view()),
                            pa.array(vals[300:], type=pa.string_view())]).slice(37, 601)
    views, valid, bufs = from_arrow(arr)
    _ingest_and_check(views, valid, bufs, tier)
    bvals = _rand_values(rng, 200, lo=0, hi=256)
    bvals[3] = b"\x00\xff" * 9
    bvals[4] = b"\x00" * 5
    _ingest_and_check(*from_arrow(pa.array(bvals, type=pa.binary_view())), tier)


@pytest.mark.parametrize("knob", [pytest.param(None, id="unset"),
                                  pytest.param("1", id="lds")])
def test_ingest_tile_larger_than_image_goes_direct(knob, monkeypatch):
    """1024 rows x 200 B: every tile's byte span exceeds the LDS image, so the run must
    report the direct path with the knob unset, and even when the LDS tier is asked for."""
    _set_tier(monkeypatch, knob)
    assert T * 200 > api.view_image_bytes()
    rng = np.random.default_rng(41)
    views, valid, bufs = _make_views(rng, _rand_values(rng, 1024, [200]), 2)
    _ingest_and_check(views, valid, bufs, 0)


@pytest.mark.parametrize("knob", TIERS)
def test_ingest_one_huge_value_between_short_ones(knob, monkeypatch):
    tier = _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(43)
    vals = _rand_values(rng, 2 * T + 5, [0, 3, 12, 13, 40])
    vals[T + 11] = bytes(rng.integers(0, 256, 100_000, dtype=np.uint8))
    views, valid, bufs = _make_views(rng, vals, 2)
    _ingest_and_check(views, valid, bufs, tier)  # the other tiles still stage


@pytest.mark.parametrize("what", ["buffer_index", "one_past_end", "negative_length"])
@pytest.mark.parametrize("knob", [pytest.param(None, id="unset"),
                                  pytest.param("1", id="lds")])
def test_ingest_invalid_views(what, knob, monkeypatch):
    """The bad view points at most a few bytes past the STATED buffer length; the real
    allocation is 4 KiB larger, so even a kernel that wrongly followed the view would read
    allocated memory only."""
    tier = _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(47)
    views, valid, bufs = _make_views(rng, _rand_values(rng, 200, [2, 12, 30]), 1, 0.1)
    stated = len(bufs[0])
    padded = np.concatenate([bufs[0], np.zeros(4096, dtype=np.uint8)])
    words = views.view(np.int32).reshape(-1, 4)
    row = int(np.flatnonzero((words[:, 0] == 30) & (valid == 1))[0])
    if what == "buffer_index":
        words[row, 2] = 1  # n_bufs is 1
    elif what == "one_past_end":
        words[row, 3] = stated - 30 + 1
    else:
        words[row, 0] = -5
    with pytest.raises(ValueError):
        ingest_ref(views, valid, [padded[:stated]])
    with pytest.raises(api.DDError) as ei:
        api.ViewIngest.from_host(views, valid, [padded], buf_lens=[stated]).destroy()
    assert ei.value.status == 1  # DD_ERR_INVALID
    # the same views are fine once the stated length covers them
    if what == "one_past_end":
        _ingest_and_check(views, valid, [padded], tier)


# ---------------- through the partitioner ----------------

def _view_col(views, valid, bufs):
    return {"dtype": "utf8view", "views": views, "bufs": bufs, "valid": valid}


def _utf8_twin(views, valid, bufs):
    off, data = ingest_ref(views, valid, bufs)
    return {"dtype": "utf8", "data": data, "offsets": off, "valid": valid}


def _run(cols, keys, P):
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, keys, P)
    part.run()
    part.sync()
    return batch, part


@pytest.mark.parametrize("P", [7, 128])
def test_view_key_partitions_like_utf8_key(P, monkeypatch):
    monkeypatch.delenv("DD_VIEW_LDS", raising=False)
    rng = np.random.default_rng(53 + P)
    n = 5000
    views, valid, bufs = _make_views(rng, _rand_values(rng, n), 3, null_frac=0.1)
    payload = {"dtype": "i64", "data": rng.integers(-2**62, 2**62, n, dtype=np.int64),
               "valid": None}
    outs = []
    for key in (_view_col(views, valid, bufs), _utf8_twin(views, valid, bufs)):
        batch, part = _run([payload, key], [1], P)
        try:
            outs.append({"pids": part.pids(), "roff": part.row_offsets(),
                         "boff": part.byte_offsets(1), "c0": part.col_out(0),
                         "c1": part.col_out(1)})
        finally:
            part.destroy()
            batch.free()
    a, b = outs
    assert (a["pids"] is None) == (b["pids"] is None)
    if a["pids"] is not None:
        assert np.array_equal(a["pids"], b["pids"])
    assert np.array_equal(a["roff"], b["roff"]) and np.array_equal(a["boff"], b["boff"])
    for c in ("c0", "c1"):
        assert a[c].keys() == b[c].keys()
        assert a[c]["dtype"] == b[c]["dtype"]
        for k in a[c]:
            if k != "dtype":
                assert np.array_equal(a[c][k], b[c][k]), (c, k)


def test_weather_shaped_group_by_view_key(monkeypatch):
    """366 rows, nullable view key over {"Yes", "No"}, two f64 payloads, P = 6: per
    partition aggregation of the shuffled batches equals direct aggregation (counts and
    keys exact, sums within the 1e-6 relative of DESIGN.md §3)."""
    monkeypatch.delenv("DD_VIEW_LDS", raising=False)
    rng = np.random.default_rng(59)
    n = 366
    keys = [None if r < 0.05 else ("Yes" if r < 0.3 else "No") for r in rng.random(n)]
    key_arr = pa.array(keys, type=pa.string_view())
    a, b = rng.uniform(0, 40, n), rng.normal(1000, 50, n)
    views, valid, bufs = from_arrow(key_arr)
    cols = [dict(_view_col(views, valid, bufs), name="RainToday"),
            {"dtype": "f64", "data": a, "valid": None, "name": "a"},
            {"dtype": "f64", "data": b, "valid": None, "name": "b"}]
    batch, part = _run(cols, [0], 6)
    try:
        got = {}
        for p, rb in arrow_boundary.partition_batches(part, 0, 6):
            if rb.num_rows == 0:
                continue
            t = pa.Table.from_batches([rb]).group_by("RainToday").aggregate(
                [("a", "sum"), ("b", "sum"), ("a", "count")])
            for k, sa, sb, c in zip(*(t[x].to_pylist() for x in
                                      ("RainToday", "a_sum", "b_sum", "a_count"))):
                assert k not in got, "a key must live in exactly one partition"
                got[k] = (sa, sb, c)
    finally:
        part.destroy()
        batch.free()
    direct = pa.table({"RainToday": key_arr.cast(pa.string()), "a": a, "b": b}).group_by(
        "RainToday").aggregate([("a", "sum"), ("b", "sum"), ("a", "count")])
    want = {k: (sa, sb, c) for k, sa, sb, c in zip(*(direct[x].to_pylist() for x in
                                                     ("RainToday", "a_sum", "b_sum",
                                                      "a_count")))}
    assert set(got) == set(want) == {None, "Yes", "No"}
    for k in want:
        assert got[k][2] == want[k][2]
        for x in (0, 1):
            assert abs(got[k][x] - want[k][x]) <= 1e-6 * abs(want[k][x])


# ---------------- emit ----------------

def _emit_and_check(part, col, W, strings, order):
    """ViewEmit vs emit_ref fed the partitioner's own output, then every window through
    pyarrow: validate(full=True) and equality with take() of the cast input."""
    out = part.col_out(col)
    roff = part.row_offsets()
    ref = emit_ref(out["lengths"], out.get("valid"), out["data"], roff,
                   part.byte_offsets(col), W)
    em = api.ViewEmit(part, col, W)
    try:
        views = em.views()
        assert np.array_equal(em.counts(), ref["long_byte_off"])
        assert np.array_equal(views, ref["views"])
        ppw = part.nparts // W
        valid = out.get("valid")
        for w in range(W):
            buf = em.window_bytes(w)
            assert buf.tobytes() == ref["bytes"][w].tobytes()
            r0, r1 = int(roff[w * ppw]), int(roff[(w + 1) * ppw])
            arr = to_arrow(views[r0:r1], None if valid is None else valid[r0:r1], buf)
            arr.validate(full=True)
            assert arr.cast(pa.string()).equals(strings.take(pa.array(order[r0:r1])))
        return em.counts().copy(), views
    finally:
        em.destroy()


def _emit_case(rng, n, n_keys):
    """i64 key + view payload whose lengths are shaped by the partition a row lands in:
    the first non-empty partition holds only inline values, the second exactly one long
    value; the rest draw from the whole length set. 10 % nulls."""
    key = {"dtype": "i64", "data": rng.integers(0, n_keys, n, dtype=np.int64),
           "valid": None}
    pid = oracle.repartition([key], [0], 16)["pid"]
    present = np.unique(pid)
    vals = _rand_values(rng, n)
    for i in np.flatnonzero((pid == present[0]) | (pid == present[1])):
        vals[i] = vals[i][:12]
    one = int(np.flatnonzero(pid == present[1])[0])
    vals[one] = b"exactly-one-long-value"
    views, valid, bufs = _make_views(rng, vals, 2, null_frac=0.1)
    if valid[one] == 0:  # keep the one long value valid (its garbage view goes)
        valid[one] = 1
        w = views.view(np.int32).reshape(-1, 4)
        views[one] = 0
        w[one, 0] = len(vals[one])
        views[one, 4:8] = np.frombuffer(vals[one][:4], dtype=np.uint8)
        w[one, 2], w[one, 3] = 0, len(bufs[0])
        bufs[0] = np.concatenate([bufs[0], np.frombuffer(vals[one], dtype=np.uint8)])
    return key, views, valid, bufs, present


@pytest.mark.parametrize("knob", TIERS)
@pytest.mark.parametrize("n_keys", [5, 4000], ids=["empty_partitions", "all_partitions"])
def test_emit_matches_ref_and_pyarrow(n_keys, knob, monkeypatch):
    _set_tier(monkeypatch, knob)
    rng = np.random.default_rng(61 + n_keys)
    n = 3000
    key, views, valid, bufs, present = _emit_case(rng, n, n_keys)
    assert (len(present) < 16) == (n_keys == 5)
    twin = _utf8_twin(views, valid, bufs)
    order = oracle.repartition([key, twin], [0], 16)["order"]
    strings = to_arrow(*_emit_views_of(twin), binary=False).cast(pa.string())
    batch, part = _run([key, _view_col(views, valid, bufs)], [0], 16)
    try:
        for W in (1, 4, 16):
            counts, _ = _emit_and_check(part, 1, W, strings, order)
            if W == 16:
                sizes = np.diff(counts)
                assert sizes[present[0]] == 0  # only inline values: empty data buffer
                assert sizes[present[1]] == len(b"exactly-one-long-value")
        with pytest.raises(api.DDError) as ei:
            api.ViewEmit(part, 1, 3)  # 3 does not divide 16
        assert ei.value.status == 1
        with pytest.raises(api.DDError) as ei:
            api.ViewEmit(part, 0, 4)  # not a utf8 column
        assert ei.value.status == 1
    finally:
        part.destroy()
        batch.free()


def _emit_views_of(twin):
    """(views, valid, buffer) of a utf8 column as ONE window, through the host model."""
    n = len(twin["offsets"]) - 1
    em = emit_ref(np.diff(twin["offsets"]), twin["valid"], twin["data"],
                  np.array([0, n], np.int64), np.array([0, len(twin["data"])], np.int64), 1)
    return em["views"], twin["valid"], em["bytes"][0]


def test_partition_batches_yields_string_view_slices(monkeypatch):
    """One 1000-row partition cut at batch_size 100: ten string_view batches over the
    partition's single compact buffer, equal to the expectation."""
    monkeypatch.delenv("DD_VIEW_LDS", raising=False)
    rng = np.random.default_rng(67)
    n, P = 1000, 16
    key = {"dtype": "i64", "data": np.full(n, 12345, dtype=np.int64), "valid": None}
    views, valid, bufs = _make_views(rng, _rand_values(rng, n), 3, null_frac=0.1)
    twin = _utf8_twin(views, valid, bufs)
    ref = oracle.repartition([key, twin], [0], P)
    strings = to_arrow(*_emit_views_of(twin)).cast(pa.string())
    batch, part = _run([key, dict(_view_col(views, valid, bufs), name="s")], [0], P)
    em = api.ViewEmit(part, 1, P)
    try:
        plain = [rb for _, rb in arrow_boundary.partition_batches(part, 0, P, 100)]
        assert all(rb.column(1).type == pa.string() for rb in plain)  # unchanged default
        seen = []
        for p, rb in arrow_boundary.partition_batches(part, 0, P, 100, views={1: em}):
            col = rb.column(1)
            assert col.type == pa.string_view()
            col.validate(full=True)
            seen.append((p, col))
        full = [c for p, c in seen if len(c)]
        assert [len(c) for c in full] == [100] * 10
        got = pa.concat_arrays([c.cast(pa.string()) for c in full])
        assert got.equals(strings.take(pa.array(ref["order"])))
        assert got.equals(pa.concat_arrays([rb.column(1) for rb in plain]))
        with pytest.raises(ValueError):
            em4 = api.ViewEmit(part, 1, 4)
            try:
                next(arrow_boundary.partition_batches(part, 0, P, 100, views={1: em4}))
            finally:
                em4.destroy()
    finally:
        em.destroy()
        part.destroy()
        batch.free()


def test_full_round_trip_from_pyarrow(monkeypatch):
    """pyarrow view array -> utf8view column -> partition -> emit: the per-partition arrays,
    cast to string, equal take() of the cast input by the oracle's row order."""
    monkeypatch.delenv("DD_VIEW_LDS", raising=False)
    rng = np.random.default_rng(71)
    n, P = 2500, 8
    vals = [v.decode() for v in _rand_values(rng, n)]
    for i in np.flatnonzero(rng.random(n) < 0.1):
        vals[i] = None
    arr = pa.concat_arrays([pa.array(vals[:900], type=pa.string_view()),
                            pa.array(vals[900:], type=pa.string_view())])
    views, valid, bufs = from_arrow(arr)
    strings = arr.cast(pa.string())
    twin = _utf8_twin(views, valid, bufs)
    order = oracle.repartition([twin], [0], P)["order"]  # the view column is the key
    batch, part = _run([_view_col(views, valid, bufs)], [0], P)
    try:
        _emit_and_check(part, 0, P, strings, order)
    finally:
        part.destroy()
        batch.free()
