"""GPU partitioned hash join vs its exact model (marked gpu).

One checker, check_join, runs dd_hash_join_run through api.hash_join and holds it to
hashjoin.hash_join_ref: seg_offsets monotone from 0 to n_rows and equal to the model's; per
output position the emitting side's row index exactly the model's; for inner the multiset
of build rows per probe row equal (their order is unspecified); every gathered column and
validity byte equal to src[idx], with a validity buffer exactly when the source has one.
Every assertion is exact: a join moves bits.

The scan's single-round span is DD_J_SCAN_TILE * DD_J_SUMS_THREADS = 1024 * 1024 rows of the
emitting side; test_emitting_side_past_one_scan_round crosses it and checks against a
vectorised numpy expectation instead of the Python model.

The refusal of an output of 2^31 rows or more is run too, in
test_refuses_an_output_of_2_31_rows_or_more: one key value on both sides reaches 2^31 and
2^32 + 4096 pairs with chains of 2048 and 4096 steps per probe lane, and the message must
name the exact 64-bit total."""

import time

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api, finalagg, hashjoin

pytestmark = pytest.mark.gpu

JOIN_TYPES = ["inner", "left_semi", "left_anti", "right_semi", "right_anti"]
NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64}
INVALID, UNSUPPORTED = 1, 6
LDS_SEGS = 1024  # DD_F_LDS_SEGS: segment offsets are staged in LDS up to this many
SCAN_SPAN = 1024 * 1024


def col(dtype, data, valid=None):
    return {"dtype": dtype, "data": data, "valid": valid}


def make_sides(seed, dtypes, nb, npr, n_values, null_frac=0.1):
    """Key columns of two sides whose key TUPLES draw from one pool of n_values tuples, so
    both sides repeat and most keys meet; NULLs fall per component."""
    rng = np.random.default_rng(seed)
    picks = (rng.integers(0, n_values, nb), rng.integers(0, n_values, npr))
    build, probe = [], []
    for dt in dtypes:
        if dt == "bool":
            pool = rng.integers(0, 2, n_values).astype(np.uint8)
        else:
            info = np.iinfo(NP[dt])
            pool = rng.integers(info.min, info.max, n_values, dtype=NP[dt], endpoint=True)
        for side, pick in zip((build, probe), picks):
            valid = (rng.random(len(pick)) >= null_frac).astype(np.uint8) if null_frac else None
            side.append(col(dt, pool[pick], valid))
    return build, probe


def payload(seed, n):
    """Two payload columns: an i32 with validity, an f64 without."""
    rng = np.random.default_rng(seed)
    return [col("i32", rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
                (rng.random(n) < 0.8).astype(np.uint8)),
            col("f64", rng.normal(size=n))]


def take(c, order):
    data = api.fixed_host(c)[order]
    return col(c["dtype"], data, None if c.get("valid") is None else c["valid"][order])


def route(cols, key_idx, P, producers=1):
    """Rows routed by the shuffle's hash as `producers` producers would leave them in an
    exchanged window: producer-major, partition-major per producer, S = producers * P
    segments with seg_part[s] = s % P (one producer: a Partitioner's output)."""
    n = len(api.fixed_host(cols[0]))
    pid = oracle.pids(oracle.hash_cols([cols[k] for k in key_idx], n), P).astype(np.int64)
    prod = np.arange(n) * producers // max(n, 1)
    order = np.lexsort((np.arange(n), pid, prod))
    counts = np.bincount(prod[order] * P + pid[order], minlength=producers * P)
    off = np.zeros(producers * P + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return ([take(c, order) for c in cols],
            {"seg_offsets": off, "seg_part": (np.arange(producers * P) % P).astype(np.int32),
             "n_parts": P})


def check_join(build, bkeys, probe, pkeys, join_type, blay=None, play=None, bproj=None,
               pproj=None):
    """Run the join and hold it to the model. Returns (seg_offsets, build_idx, probe_idx)."""
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    try:
        j = api.hash_join(bb, bkeys, pb, pkeys, join_type, blay, play, bproj, pproj)
        try:
            off = j.seg_offsets()
            bi, pi = j.pairs()
            ncols = len(j._out_cols)
            got_cols = [j.col(i) for i in range(ncols)]
            n_rows = j.n_rows
            ms = j.kernel_ms()
        finally:
            j.destroy()
    finally:
        bb.free()
        pb.free()
    want = hashjoin.hash_join_ref(build, bkeys, probe, pkeys, join_type, blay, play)
    woff = hashjoin.seg_offsets_of(want)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == n_rows
    assert np.array_equal(off, woff)
    assert len(ms) == 5 and all(m >= 0 for m in ms)
    flat = [x for seg in want for x in seg]
    if join_type == "inner":
        wb = np.array([b for b, _ in flat], dtype=np.uint32)
        wp = np.array([p for _, p in flat], dtype=np.uint32)
        assert np.array_equal(pi, wp)
        assert len(bi) == len(wb)
        # a probe row's matches are adjacent; the model lists them in ascending build row
        assert np.array_equal(bi[np.lexsort((bi, pi))], wb)
    elif join_type.startswith("left"):
        assert pi is None
        assert np.array_equal(bi, np.array(flat, dtype=np.uint32))
    else:
        assert bi is None
        assert np.array_equal(pi, np.array(flat, dtype=np.uint32))
    # gathered columns: bits of src[idx], validity exactly when the source has it
    if bproj is None:
        bproj = [] if join_type.startswith("right") else list(range(len(build)))
    if pproj is None:
        pproj = [] if join_type.startswith("left") else list(range(len(probe)))
    srcs = [(build[c], bi) for c in bproj] + [(probe[c], pi) for c in pproj]
    assert len(srcs) == ncols
    for i, ((src, idx), got) in enumerate(zip(srcs, got_cols)):
        assert got["dtype"] == src["dtype"]
        data = api.fixed_host(src)[idx]
        assert got["data"].shape == data.shape, f"output column {i}"
        assert got["data"].tobytes() == data.tobytes(), f"output column {i}"
        assert ("valid" in got) == (src.get("valid") is not None), f"output column {i}"
        if "valid" in got:
            assert np.array_equal(got["valid"], np.asarray(src["valid"], np.uint8)[idx])
    return off, bi, pi


# ---------------- the main shape ----------------

@pytest.fixture(scope="module")
def main_sides():
    """About 5 000 x 7 000 rows over 7 partitions: ragged ends against the 2048-row blocks
    and the 1024-entry scan tiles, ~3 000 key values so both sides repeat, ~10 % NULLs."""
    bk, pk = make_sides(1, ("i64",), 5003, 7001, 3000)
    build, blay = route(bk + payload(2, 5003), [0], 7)
    probe, play = route(pk + payload(3, 7001), [0], 7)
    return build, blay, probe, play


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_main_shape(main_sides, join_type):
    build, blay, probe, play = main_sides
    off, _, _ = check_join(build, [0], probe, [0], join_type, blay, play)
    assert off[-1] > 1000


@pytest.mark.parametrize("dtypes", [("i64",), ("i32",), ("i16",), ("u8",), ("bool",),
                                    ("i64", "i32"), ("u8", "bool"),
                                    ("i64", "i32", "i16", "u8")])
@pytest.mark.parametrize("join_type", ["inner", "left_anti", "right_semi"])
def test_key_dtypes(dtypes, join_type):
    nk = len(dtypes)
    # a lone bool key has two values: every probe row meets half the build side
    nb, npr = (150, 210) if dtypes == ("bool",) else (1500, 2100)
    bk, pk = make_sides(10 + nk, dtypes, nb, npr, 400)
    keys = list(range(nk))
    build, blay = route(bk + payload(4, nb), keys, 3)
    probe, play = route(pk + payload(5, npr), keys, 3)
    off, _, _ = check_join(build, keys, probe, keys, join_type, blay, play)
    assert off[-1] > 0


def test_key_columns_in_different_positions():
    bk, pk = make_sides(20, ("i32", "i64"), 900, 1100, 200)
    build = payload(6, 900) + bk          # keys at 2, 3
    probe = [pk[1], pk[0]] + payload(7, 1100)  # keys at 1, 0
    check_join(build, [2, 3], probe, [1, 0], "inner")


# ---------------- chains ----------------

@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_long_chain(join_type):
    """One build key 1 000 times against 50 probe rows of it, among other keys."""
    rng = np.random.default_rng(30)
    bkey = np.concatenate([np.full(1000, 77, dtype=np.int64),
                           rng.integers(1000, 1300, 800, dtype=np.int64)])
    pkey = np.concatenate([np.full(50, 77, dtype=np.int64),
                           rng.integers(1000, 1600, 600, dtype=np.int64)])
    rng.shuffle(bkey)
    rng.shuffle(pkey)
    off, _, _ = check_join([col("i64", bkey)], [0], [col("i64", pkey)], [0], join_type)
    if join_type == "inner":
        assert off[-1] >= 50 * 1000


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_all_distinct_build_keys(join_type):
    rng = np.random.default_rng(31)
    bkey = rng.permutation(4000).astype(np.int32)[:2500]
    pkey = rng.integers(0, 4000, 3000).astype(np.int32)
    check_join([col("i32", bkey)], [0], [col("i32", pkey)], [0], join_type)


# ---------------- NULLs and empties ----------------

@pytest.mark.parametrize("null_side", ["build", "probe"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_all_null_keys(null_side, join_type):
    bk, pk = make_sides(40, ("i32",), 300, 400, 50, null_frac=0)
    side = bk if null_side == "build" else pk
    side[0]["valid"] = np.zeros(len(side[0]["data"]), dtype=np.uint8)
    off, _, _ = check_join(bk, [0], pk, [0], join_type)
    want_rows = {"left_anti": 300, "right_anti": 400}.get(join_type, 0)
    assert off[-1] == want_rows


@pytest.mark.parametrize("empty", ["build", "probe", "both"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_empty_sides(empty, join_type):
    bk, pk = make_sides(41, ("i64",), 0 if empty in ("build", "both") else 200,
                        0 if empty in ("probe", "both") else 300, 50)
    P = 3
    build, blay = route(bk + payload(8, len(bk[0]["data"])), [0], P)
    probe, play = route(pk + payload(9, len(pk[0]["data"])), [0], P)
    off, _, _ = check_join(build, [0], probe, [0], join_type, blay, play)
    assert len(off) == P + 1


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_empty_partitions_on_one_side_only(join_type):
    """Partitions 1 and 3 of the build side hold nothing; the probe side fills all five."""
    bk, pk = make_sides(42, ("i64",), 1200, 1500, 300)
    build, blay = route(bk, [0], 5)
    probe, play = route(pk, [0], 5)
    o = blay["seg_offsets"]
    keep = np.concatenate([np.arange(o[p], o[p + 1]) for p in (0, 2, 4)])
    build = [take(c, keep) for c in build]
    sizes = np.diff(o) * np.array([1, 0, 1, 0, 1])
    blay = dict(blay, seg_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    check_join(build, [0], probe, [0], join_type, blay, play)


# ---------------- layouts ----------------

@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_exchanged_style_layout(join_type):
    """S = producers * parts on both sides, with different producer counts and so many
    producers on the build side that most of its segments are empty."""
    bk, pk = make_sides(50, ("i64", "i16"), 150, 2500, 100)
    build, blay = route(bk + payload(10, 150), [0, 1], 6, producers=40)
    probe, play = route(pk + payload(11, 2500), [0, 1], 6, producers=3)
    assert (np.diff(blay["seg_offsets"]) == 0).sum() > 20
    check_join(build, [0, 1], probe, [0, 1], join_type, blay, play)


@pytest.mark.parametrize("join_type", ["inner", "left_semi", "right_anti"])
def test_more_segments_than_lds_stages(join_type):
    """Past DD_F_LDS_SEGS segments the kernels search seg_offsets in global memory."""
    bk, pk = make_sides(51, ("i32",), 3000, 4100, 900)
    build, blay = route(bk, [0], 5, producers=260)
    probe, play = route(pk, [0], 5, producers=230)
    assert len(blay["seg_part"]) > LDS_SEGS and len(play["seg_part"]) > LDS_SEGS
    check_join(build, [0], probe, [0], join_type, blay, play)


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_not_co_partitioned_pair_matches_nothing_across_partitions(join_type):
    """Key 5 sits in partition 0 of the build side and partition 1 of the probe side."""
    build = [col("i64", np.array([5, 5, 9], dtype=np.int64))]
    probe = [col("i64", np.array([7, 5, 5, 5], dtype=np.int64))]
    blay = {"seg_offsets": [0, 2, 3], "seg_part": [0, 1], "n_parts": 2}
    play = {"seg_offsets": [0, 1, 4], "seg_part": [0, 1], "n_parts": 2}
    off, _, _ = check_join(build, [0], probe, [0], join_type, blay, play)
    assert off[-1] == {"left_anti": 3, "right_anti": 4}.get(join_type, 0)


# ---------------- projections ----------------

def wide_side(seed, n, keys):
    """keys, then one column of every element size 1, 2, 4, 8, 16 without validity and one
    of each with."""
    rng = np.random.default_rng(seed)
    cols = list(keys)
    for with_valid in (False, True):
        v = (lambda: (rng.random(n) < 0.7).astype(np.uint8)) if with_valid else (lambda: None)
        cols += [col("u8", rng.integers(0, 256, n).astype(np.uint8), v()),
                 col("i16", rng.integers(-2**15, 2**15, n).astype(np.int16), v()),
                 col("f32", rng.normal(size=n).astype(np.float32), v()),
                 col("f64", rng.normal(size=n), v()),
                 col("dec128", rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64), v())]
    return cols


@pytest.fixture(scope="module")
def wide_sides():
    bk, pk = make_sides(60, ("i64",), 1100, 1300, 300)
    return wide_side(61, 1100, bk), wide_side(62, 1300, pk)


@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_every_element_size_with_and_without_validity(wide_sides, join_type):
    build, probe = wide_sides
    check_join(build, [0], probe, [0], join_type)


@pytest.mark.parametrize("bproj,pproj", [([10, 1, 5], [0, 7]), ([], [3, 10, 4, 9, 2]),
                                         ([5, 5], []), ([], [])])
def test_projection_lists(wide_sides, bproj, pproj):
    """A subset in a different order (and a column twice), an empty list on either side,
    both empty (pairs only)."""
    build, probe = wide_sides
    check_join(build, [0], probe, [0], "inner", bproj=bproj, pproj=pproj)


def test_pairs_only_has_no_batch(wide_sides):
    build, probe = wide_sides
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    j = api.hash_join(bb, [0], pb, [0], "inner", build_proj=[], probe_proj=[])
    try:
        assert j.n_rows > 0 and all(p for p in j.pairs_ptr())
        with pytest.raises(ValueError, match="pairs only"):
            j.batch()
    finally:
        j.destroy()
        bb.free()
        pb.free()


# ---------------- past one scan round ----------------

@pytest.mark.parametrize("join_type", ["inner", "right_anti"])
def test_emitting_side_past_one_scan_round(join_type):
    """1.2 M probe rows: more than the 1024 x 1024 rows the scan's middle pass covers in one
    round. Unique build keys, so every probe row has at most one match and the expectation
    is a searchsorted."""
    rng = np.random.default_rng(70)
    nb, npr, P = 300_000, SCAN_SPAN + 150_001, 4
    bkey = rng.permutation(2 * nb).astype(np.int64)[:nb] * 3
    pkey = rng.integers(0, 2 * nb, npr, dtype=np.int64) * 3
    build, blay = route([col("i64", bkey), col("i32", np.arange(nb, dtype=np.int32))], [0], P)
    probe, play = route([col("i64", pkey), col("f64", rng.normal(size=npr))], [0], P)
    bkey, pkey = build[0]["data"], probe[0]["data"]
    order = np.argsort(bkey)
    pos = np.minimum(np.searchsorted(bkey[order], pkey), nb - 1)
    hit = bkey[order][pos] == pkey
    sel = hit if join_type == "inner" else ~hit
    want_p = np.flatnonzero(sel).astype(np.uint32)
    want_b = order[pos[hit]].astype(np.uint32)

    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    j = api.hash_join(bb, [0], pb, [0], join_type, blay, play)
    try:
        off, (bi, pi) = j.seg_offsets(), j.pairs()
        got = [j.col(i) for i in range(len(j._out_cols))]
    finally:
        j.destroy()
        bb.free()
        pb.free()
    assert np.array_equal(pi, want_p)
    cum = np.concatenate([[0], np.cumsum(sel)])
    assert np.array_equal(off, cum[play["seg_offsets"]])
    if join_type == "inner":
        assert np.array_equal(bi, want_b)
        assert np.array_equal(got[0]["data"], bkey[want_b])
        assert np.array_equal(got[1]["data"], build[1]["data"][want_b])
        got = got[2:]
    else:
        assert bi is None
    assert np.array_equal(got[0]["data"], pkey[want_p])
    assert got[1]["data"].tobytes() == probe[1]["data"][want_p].tobytes()


# ---------------- refusals ----------------

def fake(dtypes, n_rows=8, valid=()):
    """A batch the library must refuse before it touches the device: the pointers are
    made up."""
    return api.DeviceBatch.from_device(
        [{"dtype": dt, "data_ptr": 0x100000 * (i + 1),
          "valid_ptr": 0x800000 * (i + 1) if i in valid else None,
          "offsets_ptr": 0x900000 if dt == "utf8" else None}
         for i, dt in enumerate(dtypes)], n_rows)


def refuse(status, cause, build, bkeys, probe, pkeys, join_type="inner", **kw):
    with pytest.raises(api.DDError) as ei:
        api.hash_join(build, bkeys, probe, pkeys, join_type, **kw)
    assert ei.value.status == status, str(ei.value)
    assert cause in str(ei.value), str(ei.value)


@pytest.mark.parametrize("dt,cause", [("f32", "f32 / f64 keys"), ("f64", "f32 / f64 keys"),
                                      ("dict32", "dict32 keys"), ("utf8", "utf8"),
                                      ("dec128", "dec128 keys")])
def test_refuses_key_dtypes(dt, cause):
    refuse(UNSUPPORTED, cause, fake([dt, "i64"]), [0], fake([dt, "i64"]), [0])
    refuse(UNSUPPORTED, cause, fake(["i64", dt]), [0, 1], fake(["i64", dt]), [0, 1])


@pytest.mark.parametrize("dt,cause", [("utf8", "var-width"), ("dict32", "dict32 column")])
def test_refuses_projection_dtypes(dt, cause):
    refuse(UNSUPPORTED, cause, fake(["i64", dt]), [0], fake(["i64"]), [0])
    refuse(UNSUPPORTED, cause, fake(["i64"]), [0], fake(["i64", dt]), [0])
    # not projected: not refused for it (no device work either: the probe side is empty)
    j = api.hash_join(fake(["i64", dt]), [0], fake(["i64"], n_rows=0), [0], build_proj=[0])
    assert j.n_rows == 0
    j.destroy()


def test_refuses_more_than_four_keys():
    five = fake(["i32"] * 5)
    refuse(UNSUPPORTED, "more than 4 key", five, list(range(5)), five, list(range(5)))


@pytest.mark.parametrize("join_type", ["left", "right", "full"])
def test_refuses_outer_joins(join_type):
    refuse(UNSUPPORTED, "outer joins", fake(["i64"]), [0], fake(["i64"]), [0], join_type)


def test_refuses_invalid_arguments():
    a, b = fake(["i64", "i32"]), fake(["i64", "i32"])
    refuse(INVALID, "key dtypes differ pairwise", a, [0], b, [1])
    refuse(INVALID, "key dtypes differ pairwise", fake(["u8"]), [0], fake(["bool"]), [0])
    refuse(INVALID, "key column index out of range", a, [2], b, [0])
    refuse(INVALID, "key column index out of range", a, [0], b, [-1])
    refuse(INVALID, "projected column index out of range", a, [0], b, [0], build_proj=[2])
    refuse(INVALID, "projected column index out of range", a, [0], b, [0], probe_proj=[-1])
    refuse(INVALID, "probe-side projection list is not allowed", a, [0], b, [0], "left_semi",
           probe_proj=[0])
    refuse(INVALID, "probe-side projection list is not allowed", a, [0], b, [0], "left_anti",
           probe_proj=[1])
    refuse(INVALID, "build-side projection list is not allowed", a, [0], b, [0], "right_semi",
           build_proj=[0])
    refuse(INVALID, "build-side projection list is not allowed", a, [0], b, [0], "right_anti",
           build_proj=[1])
    big = fake(["i64"], n_rows=2**31)
    refuse(INVALID, "build side: n_rows must be below 2^31", big, [0], fake(["i64"]), [0])
    refuse(INVALID, "probe side: n_rows must be below 2^31", fake(["i64"]), [0], big, [0])


def test_refuses_layouts():
    a, b = fake(["i64"]), fake(["i64"])
    lay = lambda off, part, P: {"seg_offsets": off, "seg_part": part, "n_parts": P}
    ok2 = lay([0, 3, 8], [0, 1], 2)
    refuse(INVALID, "unequal n_parts", a, [0], b, [0], build_layout=ok2,
           probe_layout=lay([0, 8], [0], 1))
    refuse(INVALID, "unequal n_parts", a, [0], b, [0], build_layout=ok2)
    for bad, cause in [(lay([0, 3, 7], [0, 1], 2), "seg_offsets must run from 0 to n_rows"),
                       (lay([1, 3, 8], [0, 1], 2), "seg_offsets must run from 0 to n_rows"),
                       (lay([0, 9, 8], [0, 1], 2), "seg_offsets decrease"),
                       (lay([0, 3, 8], [0, 2], 2), "seg_part outside"),
                       (lay([0, 3, 8], [-1, 1], 2), "seg_part outside"),
                       (lay([0, 8], [0], 0), "at least one segment and one partition")]:
        refuse(INVALID, "malformed build segment layout: " + cause, a, [0], b, [0],
               build_layout=bad, probe_layout=ok2)
        refuse(INVALID, "malformed probe segment layout: " + cause, a, [0], b, [0],
               build_layout=ok2, probe_layout=bad)
    with pytest.raises(ValueError, match="one entry more"):
        api.hash_join(a, [0], b, [0], build_layout=lay([0, 8], [0, 1], 2), probe_layout=ok2)


# ---------------- the 2^31-row limit ----------------

@pytest.mark.parametrize("nb,npr,total", [(2048, 2**20, 2147483648),
                                          (4096, 2**20 + 1, 4294971392)])
def test_refuses_an_output_of_2_31_rows_or_more(main_sides, nb, npr, total):
    """One i32 key value on both sides, one partition, no projected column: nb * npr pairs.
    2048 x 2^20 is exactly 2^31, the smallest refused output; 4096 x (2^20 + 1) is
    2^32 + 4096, which a 32-bit total anywhere between the scan and the host check would
    read as 4096 rows and accept. Each probe lane walks an nb-step chain inside a next
    array of 4 * nb bytes, and a wave's lanes walk the same addresses, so the count pass
    takes milliseconds (the printed wall time). Nothing is emitted. After the
    refusal the same entry joins the main shape and matches the model."""
    assert nb * npr == total >= 2**31
    bb = api.DeviceBatch([col("i32", np.full(nb, 7, dtype=np.int32))])
    pb = api.DeviceBatch([col("i32", np.full(npr, 7, dtype=np.int32))])
    try:
        t0 = time.perf_counter()
        with pytest.raises(api.DDError) as ei:
            api.hash_join(bb, [0], pb, [0], "inner", build_proj=[], probe_proj=[])
        seconds = time.perf_counter() - t0
    finally:
        bb.free()
        pb.free()
    print(f"inner {nb} x {npr}: refused after {seconds * 1e3:.1f} ms")
    assert ei.value.status == UNSUPPORTED, str(ei.value)
    assert f"output of {total} rows is 2^31 or more" in str(ei.value), str(ei.value)
    build, blay, probe, play = main_sides
    off, _, _ = check_join(build, [0], probe, [0], "inner", blay, play)
    assert off[-1] > 1000


# ---------------- reuse and what follows the join ----------------

def test_two_joins_from_the_same_inputs_agree(main_sides):
    build, blay, probe, play = main_sides
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    runs = []
    for _ in range(2):
        j = api.hash_join(bb, [0], pb, [0], "inner", blay, play)
        bi, pi = j.pairs()
        order = np.lexsort((bi, pi))  # the order among one probe row's matches is free
        cols = [api.fixed_host(j.col(i))[order] for i in range(len(j._out_cols))]
        runs.append((j.seg_offsets(), bi[order], pi[order], cols))
        j.destroy()
    bb.free()
    pb.free()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    for c0, c1 in zip(runs[0][3], runs[1][3]):
        assert c0.tobytes() == c1.tobytes()


def test_joined_batch_feeds_partitioner_and_final_merge():
    """Joined.batch() is a device batch plus a layout: a Partitioner repartitions it and
    final_merge aggregates it per partition, neither through a host copy."""
    rng = np.random.default_rng(80)
    nb, npr, P = 800, 3000, 4
    bkey = (rng.permutation(1200)[:nb]).astype(np.int64)
    build, blay = route([col("i64", bkey), col("i32", (bkey % 7).astype(np.int32))], [0], P)
    probe, play = route([col("i64", rng.integers(0, 1200, npr, dtype=np.int64)),
                         col("i64", rng.integers(-1000, 1000, npr, dtype=np.int64)),
                         col("i64", rng.integers(1, 4, npr, dtype=np.int64))], [0], P)
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    j = api.hash_join(bb, [0], pb, [0], "inner", blay, play, build_proj=[1],
                      probe_proj=[0, 1, 2])
    try:
        view, layout = j.batch()
        host = [dict(j.col(i), valid=None) for i in range(4)]
        assert view.n_rows == j.n_rows > 0
        # group by (o.payload, key) within each partition; sum_i64 of col 2 with nn col 3
        aggs = [(2, "sum_i64", 3), (3, "count", None)]
        res = api.final_merge(view, [0, 1], aggs, **layout)
        want = finalagg.final_merge_ref(host, [0, 1], aggs, **layout)
        goff = res["group_offsets"]
        assert np.array_equal(np.diff(goff), [len(w) for w in want])
        lo = np.ascontiguousarray(res["aggs"]).view(np.uint64)
        for p, wp in enumerate(want):
            for r in range(goff[p], goff[p + 1]):
                ent = wp[(tuple(res["keys"][r].tolist()), int(res["keynull"][r]))]
                for g in range(2):
                    assert int(lo[r, g]) == ent[g]["value"] & (2**64 - 1)
                    assert int(res["nn"][r, g]) == ent[g]["nn"]
        # and a further shuffle of the join's output on another key
        part = api.Partitioner(view, [0], 5)
        part.run()
        part.sync()
        ref = oracle.repartition(host, [0], 5)
        assert np.array_equal(part.row_offsets(), ref["part_offsets"])
        for i in range(4):
            assert np.array_equal(part.col_out(i)["data"], ref["cols"][i]["data"])
        part.destroy()
    finally:
        j.destroy()
        bb.free()
        pb.free()
