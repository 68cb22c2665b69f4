"""GPU sort / top-k per partition (api.sort_topk, dd_sort.hip; marked gpu), held EXACTLY to
sortref.sort_ref: perm, seg_offsets, every gathered byte and validity byte. The shapes are the
smallest at which the kernels can go wrong: row counts around the wave, the tile and the
multi-tile scan; ties across every boundary of the stable scatter; every key dtype, direction
and null placement with the float and decimal specials; layouts past the LDS staging and
past one partition digit; the census-planned passes with and without DD_SORT_SKIP=0."""

import itertools

import numpy as np
import pytest

from datafusion_distributed_amd import api, sortref
from tests.test_sort_cpu import (FLOAT_SPECIALS, KEY_DTYPES, dec_words, make_col,
                                 make_layout)

pytestmark = pytest.mark.gpu


def _bytes(col):
    return np.ascontiguousarray(col["data"]).view(np.uint8).reshape(-1)


def check(cols, keys, layout=None, fetch=None, proj=None, batch=None):
    """Run sort_topk and hold it to sort_ref bit for bit; returns info()."""
    want = sortref.sort_ref(cols, keys, layout, fetch, proj)
    own = batch is None
    if own:
        batch = api.DeviceBatch(cols)
    s = api.sort_topk(batch, keys, layout, fetch, proj)
    try:
        n_parts = 1 if layout is None else layout["n_parts"]
        assert np.array_equal(s.seg_offsets(), want["seg_offsets"])
        assert s.n_rows == len(want["perm"])
        assert np.array_equal(s.perm(), want["perm"]), "perm differs from the model"
        lay = s.layout()
        assert lay["n_parts"] == n_parts
        assert np.array_equal(lay["seg_part"], np.arange(n_parts))
        for i, w in enumerate(want["cols"]):
            got = s.col(i)
            assert got["dtype"] == w["dtype"]
            assert np.array_equal(_bytes(got), _bytes(w)), f"projected column {i}: data"
            assert ("valid" in got) == ("valid" in w)
            if "valid" in w:
                assert np.array_equal(got["valid"], w["valid"]), f"projected column {i}: valid"
        return s.info()
    finally:
        s.destroy()
        if own:
            batch.free()


@pytest.fixture(scope="module")
def T():
    """Rows per scatter tile, from the library."""
    cols = [{"dtype": "u8", "data": np.array([1, 0], dtype=np.uint8), "valid": None}]
    batch = api.DeviceBatch(cols)
    s = api.sort_topk(batch, [(0, False, False)])
    try:
        return s.info()["tile_rows"]
    finally:
        s.destroy()
        batch.free()


# ---------------- row counts ----------------

@pytest.mark.parametrize("which", ("0", "1", "63", "64", "65", "T-1", "T", "T+1", "3*T+17"))
def test_row_counts_around_wave_and_tile(which, T):
    n = eval(which, {"T": T})
    rng = np.random.default_rng(n)
    cols = [make_col(rng, "i16", n, 0.1), make_col(rng, "u8", n, few=True),
            make_col(rng, "i64", n)]
    check(cols, [(1, True, False), (0, False, True)])
    if n:
        check(cols, [(0, False, False)], make_layout(rng, n, 3, 2), fetch=max(1, n // 7))


def test_histogram_scan_past_one_round(T):
    """The scan's one-block middle pass takes 1024 sums of 1024 histogram entries per round,
    256 entries per tile: more than 4096 tiles need a second round. One pass over a u8 key,
    held to numpy's stable argsort."""
    n = 4096 * T + 3 * T + 5
    rng = np.random.default_rng(1)
    key = rng.integers(0, 256, n).astype(np.uint8)
    batch = api.DeviceBatch([{"dtype": "u8", "data": key, "valid": None}])
    s = api.sort_topk(batch, [(0, False, False)], proj=[])
    try:
        assert s.info()["passes_run"] == 1
        assert np.array_equal(s.perm(), np.argsort(key, kind="stable").astype(np.uint32))
    finally:
        s.destroy()
        batch.free()


# ---------------- stability ----------------

def test_three_values_over_several_tiles(T):
    n = 5 * T + 100
    rng = np.random.default_rng(2)
    cols = [{"dtype": "u8", "data": rng.integers(7, 10, n).astype(np.uint8), "valid": None},
            {"dtype": "i32", "data": np.arange(n, dtype=np.int32), "valid": None}]
    for desc in (False, True):
        info = check(cols, [(0, desc, False)])
        assert info["passes_run"] == 1


def test_ties_straddle_wave_step_and_tile_boundaries(T):
    """Runs of equal keys of lengths that are no multiple of 64: every run crosses lane,
    step, wave and tile boundaries somewhere; the second key ties in the leading one."""
    n = 3 * T + 333
    runs = np.repeat(np.arange(n // 37 + 1), 37)[:n]
    cols = [{"dtype": "i32", "data": (runs % 5).astype(np.int32), "valid": None},
            {"dtype": "i16", "data": ((runs * 7) % 3).astype(np.int16), "valid": None},
            {"dtype": "i64", "data": np.arange(n, dtype=np.int64), "valid": None}]
    check(cols, [(0, False, False)])
    check(cols, [(0, True, False), (1, False, False)])
    # a constant leading key: the whole input ties there
    cols[0]["data"] = np.full(n, 3, dtype=np.int32)
    check(cols, [(0, False, False), (1, True, False)])


def test_fetch_cuts_through_a_run_of_ties(T):
    n = T + 700
    rng = np.random.default_rng(3)
    cols = [{"dtype": "u8", "data": rng.integers(0, 2, n).astype(np.uint8), "valid": None},
            {"dtype": "i32", "data": np.arange(n, dtype=np.int32), "valid": None}]
    layout = make_layout(rng, n, 3, 2)
    for fetch in (0, 1, 10, 100, n):
        check(cols, [(0, False, False)], layout, fetch)


# ---------------- keys ----------------

def special_col(rng, dt, n):
    """make_col's values with the dtype's specials sprinkled in, plus NULLs."""
    col = make_col(rng, dt, n, 0.15)
    at = rng.choice(n, size=n // 3, replace=False)
    if dt in ("f32", "f64"):
        u, _, bits = FLOAT_SPECIALS[dt]
        raw = col["data"].view(u).copy()
        raw[at] = rng.choice(np.array(bits, dtype=u), size=len(at))
        col["data"] = raw.view(col["data"].dtype)
    elif dt == "dec128":
        top = 1 << 63
        vals = [-(2**127), -(2**64) - 1, -(2**64), -top - 1, -top, -1, 0, 1, top - 1, top,
                top + 1, 2**64 - 1, 2**64, 2**64 + top, 2**127 - 1]
        col["data"][at] = dec_words([vals[i] for i in rng.integers(0, len(vals), len(at))])
    elif dt in ("i16", "i32", "i64"):
        info = np.iinfo(col["data"].dtype)
        col["data"][at] = rng.choice(np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1,
                                               info.max], dtype=col["data"].dtype),
                                     size=len(at))
    return col


@pytest.mark.parametrize("dt", KEY_DTYPES)
def test_every_dtype_direction_and_null_placement(dt):
    rng = np.random.default_rng(KEY_DTYPES.index(dt))
    n = 1500
    cols = [special_col(rng, dt, n), make_col(rng, "i32", n)]
    batch = api.DeviceBatch(cols)
    try:
        for desc, nf in itertools.product((False, True), repeat=2):
            check(cols, [(0, desc, nf)], batch=batch)
        check(cols, [(0, True, False)], make_layout(rng, n, 7, 3), fetch=20, batch=batch)
    finally:
        batch.free()


@pytest.mark.parametrize("dts", (("u8", "f64"), ("dec128", "i32", "bool"),
                                 ("i16", "dec128", "f32", "i64"),
                                 ("dec128", "dec128", "dec128", "dec128")))
def test_mixed_keys(dts):
    rng = np.random.default_rng(len(dts))
    n = 2500
    cols = [make_col(rng, dt, n, 0.1 * (j % 3), few=(j + 1 < len(dts)))
            for j, dt in enumerate(dts)] + [make_col(rng, "i64", n)]
    keys = [(j, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for j in range(len(dts))]
    check(cols, keys, make_layout(rng, n, 5, 3))
    check(cols, keys[::-1], fetch=33)


def test_a_key_that_is_all_null():
    rng = np.random.default_rng(5)
    n = 700
    cols = [make_col(rng, "f64", n, 1.0), make_col(rng, "i32", n, 0.2, few=True)]
    for nf in (False, True):
        check(cols, [(0, True, nf), (1, False, nf)])
        check(cols, [(1, False, nf), (0, False, nf)], make_layout(rng, n, 3, 1))


# ---------------- layouts ----------------

@pytest.mark.parametrize("n_parts", (1, 2, 3, 7, 61, 128, 257, 300))
def test_partition_counts(n_parts):
    """257 and 300 need two partition digits."""
    rng = np.random.default_rng(n_parts)
    n = 6000
    cols = [make_col(rng, "i32", n, 0.05, few=True), make_col(rng, "f32", n)]
    keys = [(0, True, True), (1, False, False)]
    check(cols, keys, make_layout(rng, n, n_parts, 1))
    check(cols, keys, make_layout(rng, n, n_parts, 3), fetch=10)


def test_more_segments_than_the_lds_staging_holds():
    """9 producers x 128 partitions = 1152 segments: the search reads them from memory."""
    rng = np.random.default_rng(6)
    n = 9000
    cols = [make_col(rng, "i64", n), make_col(rng, "u8", n, 0.3)]
    layout = make_layout(rng, n, 128, 9)
    assert len(layout["seg_part"]) == 1152
    check(cols, [(1, False, True), (0, True, False)], layout)
    check(cols, [(0, False, False)], layout, fetch=5)


def test_empty_partitions_and_every_row_in_one():
    rng = np.random.default_rng(8)
    n = 3000
    cols = [make_col(rng, "i16", n, 0.1), make_col(rng, "i64", n)]
    keys = [(0, False, False)]
    # partitions 0, 2 and 5 of 6 hold rows; 1, 3, 4 are empty (no segment, or empty ones)
    layout = {"seg_offsets": np.array([0, 1000, 1000, 1800, 1800, 3000], dtype=np.int64),
              "seg_part": np.array([5, 3, 0, 1, 2], dtype=np.int32), "n_parts": 6}
    check(cols, keys, layout)
    check(cols, keys, layout, fetch=7)
    one = {"seg_offsets": np.array([0, 1200, 3000], dtype=np.int64),
           "seg_part": np.array([4, 4], dtype=np.int32), "n_parts": 9}
    check(cols, keys, one, fetch=2000)


# ---------------- pass plan ----------------

def test_pass_plan_and_skip_knob(monkeypatch):
    """The census drops every pass whose digit is the same in all rows; DD_SORT_SKIP=0 runs
    every planned pass; the bits are the same either way."""
    rng = np.random.default_rng(9)
    n = 5000
    cases = [
        # (key column, planned, run): a constant key runs no pass at all
        ({"dtype": "i64", "data": np.full(n, -12345, dtype=np.int64), "valid": None}, 8, 0),
        # an i64 key within [0, 200): one digit differs
        ({"dtype": "i64", "data": rng.integers(0, 200, n, dtype=np.int64), "valid": None}, 8, 1),
        # a validity buffer that has no NULL plans a null-rank pass and drops it
        ({"dtype": "i32", "data": rng.integers(0, 60000, n).astype(np.int32),
          "valid": np.ones(n, dtype=np.uint8)}, 5, 2),
    ]
    for key, planned, run in cases:
        cols = [key, make_col(rng, "i32", n)]
        monkeypatch.delenv("DD_SORT_SKIP", raising=False)
        info = check(cols, [(0, True, False)])
        assert (info["passes_planned"], info["passes_run"]) == (planned, run)
        monkeypatch.setenv("DD_SORT_SKIP", "0")
        info = check(cols, [(0, True, False)])
        assert (info["passes_planned"], info["passes_run"]) == (planned, planned)
    # partition digits: one for 200 partitions, planned even when every row sits in one
    cols = [cases[1][0], make_col(rng, "i32", n)]
    one = {"seg_offsets": [0, n], "seg_part": [150], "n_parts": 200}
    monkeypatch.delenv("DD_SORT_SKIP")
    assert check(cols, [(0, False, False)], one)["passes_run"] == 1
    monkeypatch.setenv("DD_SORT_SKIP", "0")
    info = check(cols, [(0, False, False)], one)
    assert (info["passes_planned"], info["passes_run"]) == (9, 9)


# ---------------- projection ----------------

def test_projection_of_every_element_size():
    rng = np.random.default_rng(10)
    n = 2100
    cols = [make_col(rng, "i32", n, 0.1, few=True)]
    for dt in ("u8", "i16", "f32", "i64", "dec128"):  # 1, 2, 4, 8, 16 bytes
        cols.append(make_col(rng, dt, n))
        cols.append(make_col(rng, dt, n, 0.3))
    keys = [(0, False, False)]
    check(cols, keys, make_layout(rng, n, 3, 1))                  # every column, key included
    check(cols, keys, proj=[10, 0, 3, 3, 8], fetch=50)           # a subset, one twice
    info = check(cols, keys, proj=[])                             # perm only
    assert info["words"] == 2
    batch = api.DeviceBatch(cols[:2])
    s = api.sort_topk(batch, keys, proj=[])
    try:
        with pytest.raises(ValueError, match="no projected columns"):
            s.batch()
    finally:
        s.destroy()
        batch.free()


# ---------------- chaining ----------------

def test_merge_step_over_sorted_batch():
    """sort_topk over Sorted.batch() with the collapsed layout equals sort_ref of the whole
    input as one partition with the same fetch: the SortPreservingMergeExec."""
    rng = np.random.default_rng(12)
    n = 5000
    cols = [make_col(rng, "dec128", n, 0.1, few=True), make_col(rng, "i32", n, few=True),
            make_col(rng, "i64", n)]
    keys = [(0, True, False), (1, False, False)]
    layout = make_layout(rng, n, 7, 1)  # partition-major rows: input rank = partition order
    batch = api.DeviceBatch(cols)
    for fetch in (10, None):
        first = api.sort_topk(batch, keys, layout, fetch)
        view, lay = first.batch()
        assert view.n_rows == first.n_rows == lay["seg_offsets"][-1]
        second = api.sort_topk(view, keys, sortref.collapsed_layout(view.n_rows), fetch)
        try:
            whole = sortref.sort_ref(cols, keys, None, fetch)
            assert np.array_equal(first.perm()[second.perm()], whole["perm"])
            for i, w in enumerate(whole["cols"]):
                got = second.col(i)
                assert np.array_equal(_bytes(got), _bytes(w))
                if "valid" in w:
                    assert np.array_equal(got["valid"], w["valid"])
            assert second.seg_offsets().tolist() == [0, len(whole["perm"])]
        finally:
            second.destroy()
            first.destroy()
    batch.free()


def test_sort_of_an_outer_joins_batch():
    """Joined.batch() of a full join, with its two sections and NULL-extended columns, sorted
    directly under the join's own layout."""
    rng = np.random.default_rng(13)
    P = 4

    def side(n, lo, hi):
        k = rng.integers(lo, hi, n).astype(np.int32)
        order = np.argsort(k % P, kind="stable")
        k = k[order]
        off = np.concatenate([[0], np.cumsum(np.bincount(k % P, minlength=P))])
        return ([{"dtype": "i32", "data": k, "valid": None},
                 {"dtype": "i64", "data": rng.integers(-50, 50, n), "valid": None}],
                {"seg_offsets": off.astype(np.int64), "seg_part": np.arange(P, dtype=np.int32),
                 "n_parts": P})

    bcols, blay = side(400, 0, 300)
    pcols, play = side(700, 150, 450)
    build, probe = api.DeviceBatch(bcols), api.DeviceBatch(pcols)
    j = api.outer_join(build, [0], probe, [0], "full", blay, play)
    try:
        jview, jlay = j.batch()
        assert len(jlay["seg_part"]) == 2 * P
        host = [j.col(i) for i in range(4)]
        assert all("valid" in c and (c["valid"] == 0).any() for c in host)
        # build key DESC NULLS FIRST, probe payload ASC NULLS LAST, probe key
        keys = [(0, True, True), (3, False, False), (2, False, False)]
        check(host, keys, jlay, batch=jview)
        check(host, keys, jlay, fetch=25, batch=jview)
    finally:
        j.destroy()
        build.free()
        probe.free()


# ---------------- refusals ----------------

def test_every_refusal_by_status_and_message():
    n = 100
    doff = np.array([0, 1, 2], dtype=np.int32)
    views = np.zeros((n, 16), dtype=np.uint8)
    views[:, 0] = 1  # 1-byte inline strings
    cols = [
        {"dtype": "i64", "data": np.arange(n, dtype=np.int64), "valid": None},
        {"dtype": "dict32", "data": np.zeros(n, dtype=np.int32), "valid": None,
         "dict_bytes": np.frombuffer(b"ab", dtype=np.uint8), "dict_offsets": doff},
        {"dtype": "utf8", "data": np.frombuffer(b"x" * n, dtype=np.uint8),
         "offsets": np.arange(n + 1, dtype=np.int32), "valid": None},
        {"dtype": "utf8view", "valid": None, "bufs": [], "views": views},
    ]
    batch = api.DeviceBatch(cols)
    k = [(0, False, False)]
    lay = {"seg_offsets": [0, 60, 100], "seg_part": [0, 1], "n_parts": 2}
    cases = [
        ("DD_ERR_UNSUPPORTED", "dictionary index order", dict(keys=[(1, False, False)])),
        ("DD_ERR_UNSUPPORTED", "utf8", dict(keys=[(2, False, False)])),
        ("DD_ERR_UNSUPPORTED", "utf8view", dict(keys=[(3, True, True)])),
        ("DD_ERR_UNSUPPORTED", "var-width", dict(keys=k, proj=[0, 2])),
        ("DD_ERR_UNSUPPORTED", "var-width", dict(keys=k, proj=[3])),
        ("DD_ERR_UNSUPPORTED", "dict32", dict(keys=k, proj=[1])),
        ("DD_ERR_UNSUPPORTED", "projection", dict(keys=k, proj=None)),  # default: all columns
        ("DD_ERR_INVALID", "1..4 sort keys", dict(keys=[])),
        ("DD_ERR_INVALID", "1..4 sort keys", dict(keys=k * 5)),
        ("DD_ERR_INVALID", "key column index", dict(keys=[(4, False, False)])),
        ("DD_ERR_INVALID", "projected column index", dict(keys=k, proj=[-1])),
        ("DD_ERR_INVALID", "fetch", dict(keys=k, fetch=-1)),
        ("DD_ERR_INVALID", "0 to n_rows", dict(keys=k, layout=dict(lay, seg_offsets=[0, 60, 99]))),
        ("DD_ERR_INVALID", "decrease", dict(keys=k, layout=dict(lay, seg_offsets=[0, 101, 100]))),
        ("DD_ERR_INVALID", "seg_part outside", dict(keys=k, layout=dict(lay, seg_part=[0, 2]))),
        ("DD_ERR_INVALID", "at least one", dict(keys=k, layout=dict(lay, n_parts=0))),
    ]
    try:
        for status, word, kw in cases:
            kw.setdefault("proj", [0])
            with pytest.raises(api.DDError) as ei:
                api.sort_topk(batch, **kw)
            assert api.STATUS_NAMES[ei.value.status] == status, str(ei.value)
            assert word in str(ei.value), str(ei.value)
        # and the batch still sorts after all of that
        check(cols[:1], k, lay, fetch=3, proj=[0])
    finally:
        batch.free()
