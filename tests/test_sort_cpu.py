"""CPU tests of the sort / top-k model (sortref.py): sort_ref against pyarrow's
stable sort_indices with the partition id prepended as the first key; ordered_words on its own
against Python comparisons of the specials pyarrow orders differently (-0.0, NaNs) or that
stress the word encoding; and the argument checks that need no device, in the model, in
api.sort_topk and in dd_sort_run (whose every check runs before any device work)."""

import itertools

import numpy as np
import pytest

from datafusion_distributed_amd import api, sortref

KEY_DTYPES = ("u8", "bool", "i16", "i32", "i64", "f32", "f64", "dec128")
FETCHES = (0, 1, 10, "exact", "more", None)


# ---------------- generators shared with nothing: small on purpose ----------------

def make_col(rng, dt, n, null_frac=0.0, few=False):
    """A key column dict of n rows; few=True draws from a handful of values (ties)."""
    if dt == "u8":
        data = rng.integers(0, 4 if few else 256, n).astype(np.uint8)
    elif dt == "bool":
        data = rng.integers(0, 2, n).astype(np.uint8)
    elif dt == "i16":
        data = rng.integers(-3 if few else -(2**15), 3 if few else 2**15, n).astype(np.int16)
    elif dt == "i32":
        data = rng.integers(-3 if few else -(2**31), 3 if few else 2**31, n).astype(np.int32)
    elif dt == "i64":
        data = rng.integers(-3 if few else -(2**63), 3 if few else 2**63 - 1, n, dtype=np.int64)
    elif dt == "f32":  # finite, no -0.0: pyarrow treats +-0 as equal and places NaN its way
        data = (rng.integers(-3, 3, n).astype(np.float32) if few
                else rng.normal(size=n).astype(np.float32) * np.float32(1e6))
        data[data == 0] = np.float32(0.0)
    elif dt == "f64":
        data = (rng.integers(-3, 3, n).astype(np.float64) if few
                else rng.normal(size=n) * 1e12)
        data[data == 0] = 0.0
    else:  # dec128: signed 128-bit values that need both words
        vals = [int(rng.integers(-3, 3)) if few else
                int(rng.integers(-(2**62), 2**62)) * int(rng.integers(1, 2**60))
                + int(rng.integers(0, 2**40))
                for _ in range(n)]
        data = dec_words(vals)
    valid = None
    if null_frac > 0:
        valid = (rng.random(n) >= null_frac).astype(np.uint8)
    return {"dtype": dt, "data": data, "valid": valid}


def dec_words(vals):
    """u64 (n, 2) = [lo, hi] of signed Python ints (two's complement, 128 bits)."""
    out = np.zeros((len(vals), 2), dtype=np.uint64)
    for i, v in enumerate(vals):
        u = v & ((1 << 128) - 1)
        out[i, 0] = u & ((1 << 64) - 1)
        out[i, 1] = u >> 64
    return out


def make_layout(rng, n, n_parts, producers):
    """producers == 1: a partitioner layout (one segment per partition); otherwise an
    exchanged layout: producer-major, partition-major per producer, seg_part[s] = s % P."""
    n_segs = n_parts * producers
    cuts = np.sort(rng.integers(0, n + 1, n_segs - 1)) if n_segs > 1 else np.zeros(0, np.int64)
    off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    part = (np.arange(n_segs) % n_parts).astype(np.int32)
    return {"seg_offsets": off, "seg_part": part, "n_parts": n_parts}


def to_arrow(pa, col, scale=0):
    n = len(col["data"])
    mask = None if col.get("valid") is None else np.asarray(col["valid"]) == 0
    if col["dtype"] == "dec128":
        bitmap = None
        if mask is not None:
            bitmap = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
        return pa.Array.from_buffers(pa.decimal128(38, scale), n,
                                     [bitmap, pa.py_buffer(np.ascontiguousarray(col["data"]))])
    data = np.asarray(col["data"])
    if col["dtype"] == "bool":
        data = data.astype(bool)
    return pa.array(data, mask=mask)


def arrow_sort(pa, pc, cols, keys, layout, fetch):
    """pyarrow's answer in sort_ref's shape: (perm, seg_offsets)."""
    n = len(cols[0]["data"])
    off, part, n_parts = layout["seg_offsets"], layout["seg_part"], layout["n_parts"]
    pid = np.repeat(part.astype(np.int32), np.diff(off))
    names = {"pid": pa.array(pid)}
    sort_keys = [("pid", "ascending", "at_end")]
    for j, (c, desc, nf) in enumerate(keys):
        names[f"k{j}"] = to_arrow(pa, cols[c], scale=j)
        sort_keys.append((f"k{j}", "descending" if desc else "ascending",
                          "at_start" if nf else "at_end"))
    perm = pc.sort_indices(pa.table(names), sort_keys=sort_keys).to_numpy()
    rows_p = np.bincount(pid, minlength=n_parts)
    keep = rows_p if fetch is None else np.minimum(rows_p, fetch)
    in_off = np.concatenate([[0], np.cumsum(rows_p)])
    out = [perm[in_off[p]:in_off[p] + keep[p]] for p in range(n_parts)]
    assert in_off[-1] == n
    return (np.concatenate(out).astype(np.uint32),
            np.concatenate([[0], np.cumsum(keep)]).astype(np.int64))


def resolve_fetch(fetch, layout):
    rows_p = np.bincount(np.repeat(layout["seg_part"], np.diff(layout["seg_offsets"])),
                         minlength=layout["n_parts"])
    if fetch == "exact":
        return int(rows_p.max())
    if fetch == "more":
        return int(rows_p.max()) + 5
    return fetch


def check_against_arrow(cols, keys, layout, fetch):
    import pyarrow as pa
    import pyarrow.compute as pc

    fetch = resolve_fetch(fetch, layout)
    got = sortref.sort_ref(cols, keys, layout, fetch)
    perm, seg = arrow_sort(pa, pc, cols, keys, layout, fetch)
    assert np.array_equal(got["seg_offsets"], seg)
    assert got["perm"].dtype == np.uint32 and np.array_equal(got["perm"], perm)
    for c, out in zip(cols, got["cols"]):  # the gather is the perm applied
        assert np.array_equal(out["data"], np.asarray(c["data"])[perm])
        if c.get("valid") is not None:
            assert np.array_equal(out["valid"], np.asarray(c["valid"])[perm])
        else:
            assert "valid" not in out


# ---------------- sort_ref against pyarrow ----------------

@pytest.mark.parametrize("dt", KEY_DTYPES)
@pytest.mark.parametrize("desc,nf", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("null_frac", (0.0, 0.3, 1.0))
def test_single_key_every_dtype_direction_and_null_placement(dt, desc, nf, null_frac):
    rng = np.random.default_rng([KEY_DTYPES.index(dt), desc, nf, int(10 * null_frac)])
    n = 300
    cols = [make_col(rng, dt, n, null_frac, few=(dt != "dec128" and rng.random() < 0.5)),
            make_col(rng, "i32", n)]
    layout = make_layout(rng, n, 3, 1)
    check_against_arrow(cols, [(0, desc, nf)], layout, None)


@pytest.mark.parametrize("n_keys", (1, 2, 3, 4))
@pytest.mark.parametrize("fetch", FETCHES)
def test_multi_key_ties_and_fetch(n_keys, fetch):
    """Leading keys with few values tie, so later keys and the input rank decide; fetch cuts
    through runs of ties."""
    rng = np.random.default_rng(100 * n_keys + FETCHES.index(fetch))
    n = 400
    dts = list(rng.choice(KEY_DTYPES, size=n_keys, replace=False))
    cols = [make_col(rng, dt, n, null_frac=0.2 * (j % 2), few=True) for j, dt in enumerate(dts)]
    keys = [(j, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for j in range(n_keys)]
    check_against_arrow(cols, keys, make_layout(rng, n, 7, 3), fetch)


@pytest.mark.parametrize("n_parts", (1, 3, 7, 128))
@pytest.mark.parametrize("producers", (1, 3))
@pytest.mark.parametrize("fetch", (10, None))
def test_layouts(n_parts, producers, fetch):
    rng = np.random.default_rng(7 * n_parts + producers)
    n = 1500
    cols = [make_col(rng, "i64", n, 0.1, few=True), make_col(rng, "dec128", n, 0.1),
            make_col(rng, "f64", n)]
    keys = [(0, True, True), (1, False, False)]
    check_against_arrow(cols, keys, make_layout(rng, n, n_parts, producers), fetch)


def test_empty_input_and_empty_partitions():
    cols = [{"dtype": "i32", "data": np.zeros(0, dtype=np.int32), "valid": None}]
    got = sortref.sort_ref(cols, [(0, False, False)],
                           {"seg_offsets": [0, 0, 0], "seg_part": [1, 0], "n_parts": 3})
    assert got["perm"].shape == (0,) and got["seg_offsets"].tolist() == [0, 0, 0, 0]
    cols = [{"dtype": "i32", "data": np.array([5, 1, 3], dtype=np.int32), "valid": None}]
    got = sortref.sort_ref(cols, [(0, False, False)],
                           {"seg_offsets": [0, 3], "seg_part": [2], "n_parts": 4}, fetch=2)
    assert got["perm"].tolist() == [1, 2] and got["seg_offsets"].tolist() == [0, 0, 0, 2, 2]


def test_merge_step_is_a_sort_of_the_sorted_result():
    """sort_ref over a sorted result with the collapsed layout and the same fetch equals
    sort_ref of the whole input as one partition: the SortPreservingMergeExec."""
    rng = np.random.default_rng(11)
    n = 600
    cols = [make_col(rng, "i16", n, 0.1, few=True), make_col(rng, "i64", n)]
    # rows in partition order, so input rank and partition order agree for ties
    layout = make_layout(rng, n, 5, 1)
    keys = [(0, True, False)]
    first = sortref.sort_ref(cols, keys, layout, fetch=10)
    second = sortref.sort_ref(first["cols"], keys,
                              sortref.collapsed_layout(len(first["perm"])), fetch=10)
    whole = sortref.sort_ref(cols, keys, None, fetch=10)
    assert np.array_equal(first["perm"][second["perm"]], whole["perm"])
    assert np.array_equal(second["cols"][1]["data"], whole["cols"][1]["data"])


# ---------------- ordered_words on its own ----------------

def _total_order_int(bits, width):
    """Python-int key of IEEE totalOrder on a raw bit pattern."""
    mag = bits & ((1 << (width - 1)) - 1)
    return -mag - 1 if bits >> (width - 1) else mag


FLOAT_SPECIALS = {
    "f32": (np.uint32, 32, [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000,
                            0x7fc00001, 0xffc00000, 0xffc00001, 0x7f800001, 0x00000001,
                            0x80000001, 0x007fffff, 0x807fffff, 0x3f800000, 0xbf800000,
                            0x7f7fffff, 0xff7fffff]),
    "f64": (np.uint64, 64, [0x0, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000,
                            0x7ff8000000000000, 0x7ff8000000000001, 0xfff8000000000000,
                            0xfff8000000000001, 0x7ff0000000000001, 0x1, 0x8000000000000001,
                            0x000fffffffffffff, 0x800fffffffffffff, 0x3ff0000000000000,
                            0xbff0000000000000, 0x7fefffffffffffff, 0xffefffffffffffff]),
}


@pytest.mark.parametrize("dt", ("f32", "f64"))
def test_float_words_are_total_order_on_the_raw_bits(dt):
    u, width, bits = FLOAT_SPECIALS[dt]
    data = np.array(bits, dtype=u).view(np.float32 if dt == "f32" else np.float64)
    col = {"dtype": dt, "data": data, "valid": None}
    _, (asc,) = sortref.ordered_words(col)
    _, (desc,) = sortref.ordered_words(col, descending=True)
    want = [_total_order_int(b, width) for b in bits]
    for i, j in itertools.product(range(len(bits)), repeat=2):
        assert (asc[i] < asc[j]) == (want[i] < want[j]), (hex(bits[i]), hex(bits[j]))
        assert (desc[i] < desc[j]) == (want[i] > want[j])
    assert asc.max() < 1 << width and desc.max() < 1 << width
    # the named cases: -0.0 < +0.0; a sign-clear NaN above +inf; a sign-set NaN below -inf;
    # payloads order by their bits; nothing is canonicalised
    assert asc[1] < asc[0] and asc[4] > asc[2] and asc[6] < asc[3]
    assert asc[5] > asc[4] and asc[7] < asc[6] and len(set(asc.tolist())) == len(bits)


@pytest.mark.parametrize("dt,lo,hi", [("i16", -(2**15), 2**15 - 1), ("i32", -(2**31), 2**31 - 1),
                                      ("i64", -(2**63), 2**63 - 1), ("u8", 0, 255)])
def test_integer_words_at_the_limits(dt, lo, hi):
    vals = [lo, lo + 1, -1, 0, 1, hi - 1, hi] if lo < 0 else [lo, lo + 1, 127, 128, hi]
    col = {"dtype": dt, "data": np.array(vals, dtype=api.FIXED_NP[dt]), "valid": None}
    _, (asc,) = sortref.ordered_words(col)
    _, (desc,) = sortref.ordered_words(col, descending=True)
    assert asc.tolist() == sorted(asc.tolist()) and len(set(asc.tolist())) == len(vals)
    assert desc.tolist() == sorted(desc.tolist(), reverse=True)
    width = 8 * np.dtype(api.FIXED_NP[dt]).itemsize
    assert int(asc.max()) < 1 << width and int(desc.max()) < 1 << width


def test_decimal_words():
    top = 1 << 63
    vals = [-(2**127), -(2**64) - 1, -(2**64), -top - 1, -top, -1, 0, 1, top - 1, top, top + 1,
            2**64 - 1, 2**64, 2**64 + top, 2**64 + top + 1, 2**127 - 1]
    col = {"dtype": "dec128", "data": dec_words(vals), "valid": None}
    _, (hi, lo) = sortref.ordered_words(col)
    _, (dhi, dlo) = sortref.ordered_words(col, descending=True)
    asc = list(zip(hi.tolist(), lo.tolist()))
    desc = list(zip(dhi.tolist(), dlo.tolist()))
    for i, j in itertools.product(range(len(vals)), repeat=2):
        assert (asc[i] < asc[j]) == (vals[i] < vals[j]), (vals[i], vals[j])
        assert (desc[i] < desc[j]) == (vals[i] > vals[j])


def test_null_rank_and_null_values():
    col = {"dtype": "i32", "data": np.array([7, -9, 3], dtype=np.int32),
           "valid": np.array([1, 0, 1], dtype=np.uint8)}
    for desc in (False, True):
        rank, (w,) = sortref.ordered_words(col, desc, nulls_first=False)
        assert rank.tolist() == [0, 1, 0] and w[1] == 0  # the NULL's bytes are not looked at
        rank, (w,) = sortref.ordered_words(col, desc, nulls_first=True)
        assert rank.tolist() == [1, 0, 1] and w[1] == 0
    a = sortref.sort_ref([col], [(0, True, False)])
    assert a["perm"].tolist() == [0, 2, 1]  # DESC reverses the values; the NULL stays last
    a = sortref.sort_ref([col], [(0, False, True)])
    assert a["perm"].tolist() == [1, 2, 0]


# ---------------- argument checks that need no device ----------------

def test_model_refusals():
    cols = [{"dtype": "i32", "data": np.zeros(4, dtype=np.int32), "valid": None},
            {"dtype": "dict32", "data": np.zeros(4, dtype=np.int32), "valid": None}]
    with pytest.raises(ValueError, match="1..4 sort keys"):
        sortref.sort_ref(cols, [])
    with pytest.raises(ValueError, match="1..4 sort keys"):
        sortref.sort_ref(cols, [(0, False, False)] * 5)
    with pytest.raises(ValueError, match="out of range"):
        sortref.sort_ref(cols, [(2, False, False)])
    with pytest.raises(ValueError, match="not a sort key"):
        sortref.sort_ref(cols, [(1, False, False)])
    with pytest.raises(ValueError, match="fetch"):
        sortref.sort_ref(cols, [(0, False, False)], fetch=-1)
    with pytest.raises(ValueError, match="segment layout"):
        sortref.sort_ref(cols, [(0, False, False)],
                         {"seg_offsets": [0, 3], "seg_part": [0], "n_parts": 1})


def _view(dtypes, n_rows, valid=()):
    """A DeviceBatch of fake device addresses: good for every check that precedes device
    work, which is all of dd_sort_run's."""
    cols = [{"dtype": dt, "data_ptr": 0x10000 * (i + 1),
             "valid_ptr": 0x800000 + 0x10000 * i if i in valid else None}
            for i, dt in enumerate(dtypes)]
    return api.DeviceBatch.from_device(cols, n_rows)


def _refused(status, word, *args, **kwargs):
    kwargs.setdefault("proj", [0])  # the default, every column, would name the utf8 column
    with pytest.raises(api.DDError) as ei:
        api.sort_topk(*args, **kwargs)
    assert api.STATUS_NAMES[ei.value.status] == status and word in str(ei.value), str(ei.value)


def test_library_refusals_run_before_any_device_work():
    b = _view(["i64", "dict32", "utf8", "f64"], 100)
    k = [(0, False, False)]
    _refused("DD_ERR_UNSUPPORTED", "dictionary index order", b, [(1, False, False)])
    _refused("DD_ERR_UNSUPPORTED", "utf8", b, [(2, True, True)])
    _refused("DD_ERR_UNSUPPORTED", "dict32", b, k, proj=[1])
    _refused("DD_ERR_UNSUPPORTED", "var-width", b, k, proj=[0, 2])
    _refused("DD_ERR_INVALID", "1..4 sort keys", b, [])
    _refused("DD_ERR_INVALID", "1..4 sort keys", b, k * 5)
    _refused("DD_ERR_INVALID", "key column index", b, [(4, False, False)])
    _refused("DD_ERR_INVALID", "key column index", b, [(-1, False, False)])
    _refused("DD_ERR_INVALID", "projected column index", b, k, proj=[7])
    _refused("DD_ERR_INVALID", "fetch", b, k, fetch=-1)
    _refused("DD_ERR_INVALID", "fetch", b, k, fetch=-7)
    lay = {"seg_offsets": [0, 60, 100], "seg_part": [0, 1], "n_parts": 2}
    _refused("DD_ERR_INVALID", "0 to n_rows", b, k, dict(lay, seg_offsets=[0, 60, 99]))
    _refused("DD_ERR_INVALID", "0 to n_rows", b, k, dict(lay, seg_offsets=[1, 60, 100]))
    _refused("DD_ERR_INVALID", "decrease", b, k, dict(lay, seg_offsets=[0, 101, 100]))
    _refused("DD_ERR_INVALID", "seg_part outside", b, k, dict(lay, seg_part=[0, 2]))
    _refused("DD_ERR_INVALID", "at least one", b, k, dict(lay, n_parts=0))
    _refused("DD_ERR_INVALID", "below 2^31", _view(["i64"], 2**31), k)
    _refused("DD_ERR_INVALID", "16-byte aligned",
             api.DeviceBatch.from_device([{"dtype": "dec128", "data_ptr": 0x10008,
                                           "valid_ptr": None}], 10), k)


def test_python_side_argument_checks():
    b = _view(["i64"], 10)
    with pytest.raises(ValueError, match="triples"):
        api.sort_topk(b, [0])
    with pytest.raises(ValueError, match="triples"):
        api.sort_topk(b, [(0, False)])
    with pytest.raises(ValueError, match="fetch"):
        api.sort_topk(b, [(0, False, False)], fetch=2.5)
    with pytest.raises(ValueError, match="one entry more"):
        api.sort_topk(b, [(0, False, False)],
                      {"seg_offsets": [0, 10], "seg_part": [0, 1], "n_parts": 2})


def test_empty_results_need_no_device():
    """n_rows == 0 and fetch == 0 succeed with empty segments before any device work."""
    for batch, layout, fetch in (
            (_view(["i32", "f64"], 0), {"seg_offsets": [0, 0, 0], "seg_part": [0, 2],
                                         "n_parts": 3}, None),
            (_view(["i32", "f64"], 50, valid=(1,)), {"seg_offsets": [0, 20, 50],
                                                      "seg_part": [1, 0], "n_parts": 3}, 0)):
        s = api.sort_topk(batch, [(0, True, False)], layout, fetch=fetch)
        try:
            assert s.n_rows == 0 and s.seg_offsets().tolist() == [0, 0, 0, 0]
            assert s.perm().shape == (0,)
            assert s.col(1)["data"].shape == (0,)
            assert ("valid" in s.col(1)) == (fetch == 0)
            assert s.info()["passes_run"] == 0 and s.info()["tile_rows"] > 0
            view, lay = s.batch()
            assert view.n_rows == 0 and lay["n_parts"] == 3
        finally:
            s.destroy()
