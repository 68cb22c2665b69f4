"""GPU outer joins (left, right, full) vs their exact model (marked gpu).

One checker, check_outer, runs dd_hash_join_outer_run through api.outer_join and holds it to
hashjoin.outer_join_ref: the segment count (S_p, or S_p + S_b), seg_offsets monotone from 0
to n_rows and equal to the model's; probe_idx per position, JOIN_NONE where the model has
None; build_idx exact per position in the build section and as a multiset per probe row in
the probe section (the order among one probe row's matches is unspecified); every gathered
column equal to src[idx] bit for bit on real rows and zero on NONE rows; validity bytes as
specified and present exactly where specified. Every assertion is exact: a join moves bits.

The count array is cnt[n_probe + n_build] with the build part at index n_probe, unpadded:
test_cnt_seam puts that index off the 4-entry vector, the 1024-entry scan tile and the
2048-row block; test_past_one_scan_round puts it in the scan's second round.

The refusal of an output of 2^31 rows or more is run with test_gpu_hash_join.py's shapes,
for right and for full (one count array over both sections)."""

import time

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api, hashjoin
from oracle import reduce_ref as rr

pytestmark = pytest.mark.gpu

TYPES = ["left", "right", "full"]
NONE = 0xFFFFFFFF
NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64}
INVALID, UNSUPPORTED = 1, 6
LDS_SEGS = 1024  # DD_F_LDS_SEGS
SCAN_SPAN = 1024 * 1024
# which sides a type NULL-extends: (build, probe)
NULL_EXT = {"left": (False, True), "right": (True, False), "full": (True, True)}


def col(dtype, data, valid=None):
    return {"dtype": dtype, "data": data, "valid": valid}


def i64(a):
    return col("i64", np.asarray(a, dtype=np.int64))


def make_sides(seed, dtypes, nb, npr, n_values, null_frac=0.1):
    """Key columns of two sides whose key TUPLES draw from one pool of n_values tuples;
    NULLs fall per component."""
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
    """Rows as `producers` producers leave them in an exchanged window: producer-major,
    partition-major per producer, S = producers * P segments, seg_part[s] = s % P."""
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


def run_outer(build, bkeys, probe, pkeys, join_type, blay=None, play=None, bproj=None,
              pproj=None):
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    try:
        j = api.outer_join(bb, bkeys, pb, pkeys, join_type, blay, play, bproj, pproj)
        try:
            bi, pi = j.pairs()
            return {"off": j.seg_offsets(), "bi": bi, "pi": pi, "n_rows": j.n_rows,
                    "cols": [j.col(i) for i in range(len(j._out_cols))],
                    "ms": j.kernel_ms(), "layout": j.layout()}
        finally:
            j.destroy()
    finally:
        bb.free()
        pb.free()


def check_columns(got_cols, build, probe, join_type, bi, pi, bproj, pproj):
    """Gathered columns: src[idx] on real rows, zero bytes on NONE rows; validity always on
    a NULL-extended side (source byte, or 1; 0 on NONE), else exactly when the source has."""
    if bproj is None:
        bproj = list(range(len(build)))
    if pproj is None:
        pproj = list(range(len(probe)))
    ext_b, ext_p = NULL_EXT[join_type]
    srcs = [(build[c], bi, ext_b) for c in bproj] + [(probe[c], pi, ext_p) for c in pproj]
    assert len(srcs) == len(got_cols)
    for i, ((src, idx, ext), got) in enumerate(zip(srcs, got_cols)):
        assert got["dtype"] == src["dtype"]
        real = idx != NONE
        assert ext or real.all()
        host = api.fixed_host(src)
        data = np.zeros((len(idx),) + host.shape[1:], dtype=host.dtype)
        data[real] = host[idx[real]]
        assert got["data"].shape == data.shape, f"output column {i}"
        assert got["data"].tobytes() == data.tobytes(), f"output column {i}"
        has_valid = src.get("valid") is not None
        assert ("valid" in got) == (ext or has_valid), f"output column {i}"
        if "valid" in got:
            want = np.zeros(len(idx), dtype=np.uint8)
            want[real] = np.asarray(src["valid"], np.uint8)[idx[real]] if has_valid else 1
            assert np.array_equal(got["valid"], want), f"output column {i}"


def check_outer(build, bkeys, probe, pkeys, join_type, blay=None, play=None, bproj=None,
                pproj=None):
    """Run the join and hold it to the model. Returns the run."""
    r = run_outer(build, bkeys, probe, pkeys, join_type, blay, play, bproj, pproj)
    off, bi, pi = r["off"], r["bi"], r["pi"]
    want = hashjoin.outer_join_ref(build, bkeys, probe, pkeys, join_type, blay, play)
    S_p = len(play["seg_part"]) if play else 1
    S_b = len(blay["seg_part"]) if blay else 1
    n_segs = S_p if join_type == "right" else S_p + S_b
    assert len(off) == n_segs + 1 == len(want) + 1
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == r["n_rows"]
    assert np.array_equal(off, hashjoin.seg_offsets_of(want))
    ppart = np.asarray(play["seg_part"] if play else [0], dtype=np.int32)
    bpart = np.asarray(blay["seg_part"] if blay else [0], dtype=np.int32)
    assert np.array_equal(r["layout"]["seg_part"],
                          ppart if join_type == "right" else np.concatenate([ppart, bpart]))
    assert r["layout"]["n_parts"] == (play["n_parts"] if play else 1)
    assert len(r["ms"]) == 5 and all(m >= 0 for m in r["ms"])
    flat = [x for seg in want for x in seg]
    wb = np.array([NONE if b is None else b for b, _ in flat], dtype=np.uint32)
    wp = np.array([NONE if p is None else p for _, p in flat], dtype=np.uint32)
    assert bi is not None and pi is not None and len(bi) == len(pi) == len(flat)
    assert np.array_equal(pi, wp)
    cut = int(off[S_p])  # probe section | build section
    assert np.array_equal(bi[cut:], wb[cut:])
    # a probe row's matches are adjacent; the model lists them in ascending build row
    assert np.array_equal(bi[:cut][np.lexsort((bi[:cut], pi[:cut]))], wb[:cut])
    check_columns(r["cols"], build, probe, join_type, bi, pi, bproj, pproj)
    return r


# ---------------- the main shape ----------------

@pytest.fixture(scope="module")
def main_sides():
    """5 003 x 7 001 rows over 7 partitions: ragged ends against the 2048-row blocks and the
    1024-entry scan tiles, ~3 000 key values so both sides repeat, ~10 % NULLs."""
    bk, pk = make_sides(1, ("i64",), 5003, 7001, 3000)
    build, blay = route(bk + payload(2, 5003), [0], 7)
    probe, play = route(pk + payload(3, 7001), [0], 7)
    return build, blay, probe, play


@pytest.mark.parametrize("join_type", TYPES)
def test_main_shape(main_sides, join_type):
    build, blay, probe, play = main_sides
    r = check_outer(build, [0], probe, [0], join_type, blay, play)
    assert r["n_rows"] > 7001 and (r["bi"] == NONE).any() == (join_type != "left")
    assert (r["pi"] == NONE).any() == (join_type != "right")


@pytest.mark.parametrize("dtypes", [("i32",), ("u8", "bool"), ("i16", "i64", "i32", "u8")])
@pytest.mark.parametrize("join_type", TYPES)
def test_key_signatures(dtypes, join_type):
    nk = len(dtypes)
    bk, pk = make_sides(10 + nk, dtypes, 300, 420, 90)
    keys = list(range(nk))
    build, blay = route(bk + payload(4, 300), keys, 3)
    probe, play = route(pk + payload(5, 420), keys, 3)
    check_outer(build, keys, probe, keys, join_type, blay, play)


def test_key_columns_in_different_positions():
    bk, pk = make_sides(20, ("i32", "i64"), 300, 400, 80)
    build = payload(6, 300) + bk          # keys at 2, 3
    probe = [pk[1], pk[0]] + payload(7, 400)  # keys at 1, 0
    check_outer(build, [2, 3], probe, [1, 0], "full")


# ---------------- layouts ----------------

@pytest.mark.parametrize("join_type", TYPES)
def test_producers_three_against_two_with_empty_segments(join_type):
    bk, pk = make_sides(50, ("i64", "i16"), 40, 600, 30)
    build, blay = route(bk + payload(10, 40), [0, 1], 5, producers=3)
    probe, play = route(pk + payload(11, 600), [0, 1], 5, producers=2)
    assert (np.diff(blay["seg_offsets"]) == 0).any()
    r = check_outer(build, [0, 1], probe, [0, 1], join_type, blay, play)
    assert len(r["off"]) - 1 == (10 if join_type == "right" else 25)


@pytest.mark.parametrize("many", ["build", "probe"])
@pytest.mark.parametrize("join_type", TYPES)
def test_more_segments_than_lds_stages(many, join_type):
    """Past DD_F_LDS_SEGS segments build / count search seg_offsets in global memory; the
    other side stays staged."""
    bk, pk = make_sides(51, ("i32",), 3800, 4100, 1500)
    build, blay = route(bk, [0], 345, producers=3 if many == "build" else 1)
    probe, play = route(pk, [0], 345, producers=3 if many == "probe" else 1)
    assert (len(blay["seg_part"]) > LDS_SEGS) == (many == "build")
    assert (len(play["seg_part"]) > LDS_SEGS) == (many == "probe")
    check_outer(build, [0], probe, [0], join_type, blay, play)


@pytest.mark.parametrize("join_type", TYPES)
def test_default_layout(join_type):
    bk, pk = make_sides(52, ("i64",), 700, 900, 400)
    r = check_outer(bk, [0], pk, [0], join_type)
    assert len(r["off"]) == (2 if join_type == "right" else 3)


def test_not_co_partitioned_pair_matches_nothing_across_partitions():
    build, probe = [i64([5, 5, 9])], [i64([7, 5, 5, 5])]
    blay = {"seg_offsets": [0, 2, 3], "seg_part": [0, 1], "n_parts": 2}
    play = {"seg_offsets": [0, 1, 4], "seg_part": [0, 1], "n_parts": 2}
    r = check_outer(build, [0], probe, [0], "full", blay, play)
    assert r["off"].tolist() == [0, 1, 4, 6, 7]


# ---------------- the seam inside cnt ----------------

@pytest.mark.parametrize("join_type", ["left", "full"])
@pytest.mark.parametrize("nb", [5, 1030])
@pytest.mark.parametrize("npr", [1, 2, 3, 1023, 1025, 2047, 2049])
def test_cnt_seam(npr, nb, join_type):
    """The build rows' counts start at cnt[n_probe]: off the uint4 the scan loads, off its
    1024-entry tile, off the count kernel's 2048-row block."""
    bk, pk = make_sides(100 + npr + nb, ("i32",), nb, npr, max(4, (nb + npr) // 3))
    bk[0]["valid"][0] = 0  # a NULL key: at least one build row comes out of the build part
    build, blay = route(bk + payload(12, nb), [0], 2)
    probe, play = route(pk + payload(13, npr), [0], 2)
    r = check_outer(build, [0], probe, [0], join_type, blay, play)
    assert (r["pi"] == NONE).any()


def test_past_one_scan_round():
    """full with 1 048 579 probe rows: the probe rows alone pass the 1024 x 1024 entries the
    scan's middle pass covers in one round, so the build part of cnt lies in the second.
    Unique build keys: every probe row stands once, and the expectation is a searchsorted."""
    rng = np.random.default_rng(70)
    nb, npr, P = 4099, SCAN_SPAN + 3, 4
    bkey = rng.permutation(4 * nb).astype(np.int64)[:nb] * 3
    pkey = rng.integers(0, 2 * nb, npr, dtype=np.int64) * 3  # build keys >= 6 nb: no partner
    build, blay = route([col("i64", bkey), col("i32", np.arange(nb, dtype=np.int32))], [0], P)
    probe, play = route([col("i64", pkey), col("f64", rng.normal(size=npr))], [0], P)
    bkey, pkey = build[0]["data"], probe[0]["data"]
    order = np.argsort(bkey)
    pos = np.minimum(np.searchsorted(bkey[order], pkey), nb - 1)
    hit = bkey[order][pos] == pkey
    seen = np.zeros(nb, dtype=bool)
    seen[order[pos[hit]]] = True
    lone = np.flatnonzero(~seen)
    assert 0 < len(lone) < nb and hit.any() and not hit.all()
    want_b = np.concatenate([np.where(hit, order[pos], NONE), lone]).astype(np.uint32)
    want_p = np.concatenate([np.arange(npr), np.full(len(lone), NONE)]).astype(np.uint32)
    cum = np.concatenate([[0], np.cumsum(~seen)])
    want_off = np.concatenate([play["seg_offsets"], npr + cum[blay["seg_offsets"][1:]]])

    r = run_outer(build, [0], probe, [0], "full", blay, play)
    assert np.array_equal(r["off"], want_off) and r["n_rows"] == npr + len(lone)
    assert np.array_equal(r["pi"], want_p)
    assert np.array_equal(r["bi"], want_b)
    check_columns(r["cols"], build, probe, "full", r["bi"], r["pi"], None, None)


# ---------------- degenerate inputs ----------------

@pytest.mark.parametrize("empty", ["build", "probe", "both"])
@pytest.mark.parametrize("join_type", TYPES)
def test_empty_sides(empty, join_type):
    nb = 0 if empty in ("build", "both") else 200
    npr = 0 if empty in ("probe", "both") else 300
    bk, pk = make_sides(41, ("i64",), nb, npr, 50)
    P = 3
    build, blay = route(bk + payload(8, nb), [0], P)
    probe, play = route(pk + payload(9, npr), [0], P)
    r = check_outer(build, [0], probe, [0], join_type, blay, play)
    assert len(r["off"]) == (P if join_type == "right" else 2 * P) + 1
    assert r["n_rows"] == (npr if join_type != "left" else 0) + (nb if join_type != "right"
                                                                 else 0)


@pytest.mark.parametrize("null_side", ["build", "probe", "both"])
@pytest.mark.parametrize("join_type", TYPES)
def test_all_null_keys(null_side, join_type):
    bk, pk = make_sides(40, ("i32",), 300, 400, 50, null_frac=0)
    for side, name in ((bk, "build"), (pk, "probe")):
        if null_side in (name, "both"):
            side[0]["valid"] = np.zeros(len(side[0]["data"]), dtype=np.uint8)
    r = check_outer(bk + payload(14, 300), [0], pk + payload(15, 400), [0], join_type)
    assert r["n_rows"] == (400 if join_type != "left" else 0) + (300 if join_type != "right"
                                                                 else 0)


@pytest.mark.parametrize("join_type", TYPES)
def test_no_key_meets(join_type):
    r = check_outer([i64(np.arange(300))], [0], [i64(np.arange(1000, 1400))], [0], join_type)
    assert r["n_rows"] == {"left": 300, "right": 400, "full": 700}[join_type]


@pytest.mark.parametrize("join_type", TYPES)
def test_every_key_meets(join_type):
    rng = np.random.default_rng(43)
    r = check_outer([i64(rng.permutation(np.arange(300) % 100))], [0],
                    [i64(rng.permutation(np.arange(400) % 100))], [0], join_type)
    assert r["n_rows"] == 3 * 4 * 100 and not (r["bi"] == NONE).any()
    assert not (r["pi"] == NONE).any()


@pytest.mark.parametrize("join_type", TYPES)
def test_single_key_value(join_type):
    r = check_outer([i64(np.full(40, 7))] + payload(16, 40), [0],
                    [i64(np.full(50, 7))] + payload(17, 50), [0], join_type)
    assert r["n_rows"] == 40 * 50


@pytest.mark.parametrize("join_type", TYPES)
def test_one_probe_row_against_a_long_chain(join_type):
    rng = np.random.default_rng(44)
    bkey = np.concatenate([np.full(3000, 77), rng.integers(1000, 1300, 500)])
    rng.shuffle(bkey)
    r = check_outer([i64(bkey)], [0], [i64([77])], [0], join_type)
    assert r["n_rows"] == 3000 + (500 if join_type != "right" else 0)


# ---------------- columns ----------------

def wide_side(seed, n, keys):
    """keys, then one column of every element size 1, 2, 4, 8, 16 without validity and one
    of each with."""
    rng = np.random.default_rng(seed)
    cols = list(keys)
    for with_valid in (False, True):
        v = (lambda: (rng.random(n) < 0.7).astype(np.uint8)) if with_valid else (lambda: None)
        cols += [col("u8", rng.integers(1, 256, n).astype(np.uint8), v()),
                 col("i16", rng.integers(-2**15, 2**15, n).astype(np.int16), v()),
                 col("f32", rng.normal(size=n).astype(np.float32), v()),
                 col("f64", rng.normal(size=n), v()),
                 col("dec128", rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64), v())]
    return cols


@pytest.fixture(scope="module")
def wide_sides():
    bk, pk = make_sides(60, ("i64",), 1100, 1300, 800)
    return wide_side(61, 1100, bk), wide_side(62, 1300, pk)


@pytest.mark.parametrize("join_type", TYPES)
def test_every_element_size_with_and_without_validity(wide_sides, join_type):
    build, probe = wide_sides
    r = check_outer(build, [0], probe, [0], join_type)
    assert (r["bi"] == NONE).any() or (r["pi"] == NONE).any()


@pytest.mark.parametrize("join_type,bproj,pproj", [
    ("left", [0], [3, 10, 4, 9, 2]),                    # 5 columns on the NULL-extended side
    ("right", [10, 1, 5, 2, 7, 3, 8, 4, 9], [0, 7]),    # 9: two full gather groups and one
    ("full", [], [1, 2, 3, 4, 5, 6, 7, 8, 9]),          # an empty list
    ("full", [5, 5, 10, 0], []),                        # a column twice, reordered
    ("full", [], []),                                   # pairs only
])
def test_projection_lists(wide_sides, join_type, bproj, pproj):
    build, probe = wide_sides
    check_outer(build, [0], probe, [0], join_type, bproj=bproj, pproj=pproj)


# ---------------- reuse and what follows the join ----------------

def test_two_joins_from_the_same_inputs_agree(main_sides):
    build, blay, probe, play = main_sides
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    runs = []
    for _ in range(2):
        j = api.outer_join(bb, [0], pb, [0], "full", blay, play)
        bi, pi = j.pairs()
        order = np.lexsort((bi, pi))  # the order among one probe row's matches is free
        cols = [api.fixed_host(j.col(i))[order] for i in range(len(j._out_cols))]
        valid = [j.col(i)["valid"][order] for i in range(len(j._out_cols))]
        runs.append((j.seg_offsets(), bi[order], pi[order], cols + valid))
        j.destroy()
    bb.free()
    pb.free()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    for c0, c1 in zip(runs[0][3], runs[1][3]):
        assert c0.tobytes() == c1.tobytes()


@pytest.fixture(scope="module")
def full_join_inputs():
    rng = np.random.default_rng(80)
    nb, npr, P = 800, 3000, 4
    bkey = (rng.permutation(1600)[:nb]).astype(np.int64)
    build, blay = route([col("i64", bkey),
                         col("i64", rng.integers(-1000, 1000, nb, dtype=np.int64),
                             (rng.random(nb) < 0.8).astype(np.uint8))], [0], P)
    probe, play = route([col("i64", rng.integers(0, 1200, npr, dtype=np.int64)),
                         col("i64", rng.integers(-1000, 1000, npr, dtype=np.int64))], [0], P)
    return build, blay, probe, play


def test_full_join_batch_feeds_partitioner(full_join_inputs):
    """Joined.batch() of a full join is a device batch whose NULL-extended columns travel
    through a further shuffle as nullable payload and key."""
    build, blay, probe, play = full_join_inputs
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    j = api.outer_join(bb, [0], pb, [0], "full", blay, play)
    try:
        view, layout = j.batch()
        host = [j.col(i) for i in range(4)]
        assert view.n_rows == j.n_rows == layout["seg_offsets"][-1] > 3000
        assert all((h["valid"] == 0).any() for h in host)
        part = api.Partitioner(view, [2], 5)  # the probe key: NULL on the build section
        part.run()
        part.sync()
        ref = oracle.repartition(host, [2], 5)
        assert np.array_equal(part.row_offsets(), ref["part_offsets"])
        for i in range(4):
            got = part.col_out(i)
            assert np.array_equal(got["data"], ref["cols"][i]["data"])
            assert np.array_equal(got["valid"], ref["cols"][i]["valid"])
        part.destroy()
    finally:
        j.destroy()
        bb.free()
        pb.free()


def test_full_join_batch_feeds_partial_reduce(full_join_inputs):
    build, blay, probe, play = full_join_inputs
    bb, pb = api.DeviceBatch(build), api.DeviceBatch(probe)
    j = api.outer_join(bb, [0], pb, [0], "full", blay, play)
    try:
        view, _ = j.batch()
        host = [j.col(i) for i in range(4)]
        # group by the (nullable) build key; aggregates over NULL-extended payload
        aggs = [(1, "sum_i64"), (3, "max_i64"), (2, "min_i64"), (None, "count")]
        res = api.partial_reduce(view, [0], aggs)
    finally:
        j.destroy()
        bb.free()
        pb.free()
    got = rr.final_merge(res, [o for _, o in aggs])
    want = rr.reduce_ref(host, [0], aggs)
    assert set(got) == set(want) and any(kn for _, kn in want)
    for gid, ent in want.items():
        for g in range(len(aggs)):
            assert got[gid][g]["nn"] == ent[g]["nn"], (gid, g)
            assert got[gid][g]["value"] == ent[g]["value"], (gid, g)


# ---------------- refusals ----------------

def fake(dtypes, n_rows=8, valid=()):
    """A batch the library must refuse before it touches the device: the pointers are
    made up."""
    return api.DeviceBatch.from_device(
        [{"dtype": dt, "data_ptr": 0x100000 * (i + 1),
          "valid_ptr": 0x800000 * (i + 1) if i in valid else None,
          "offsets_ptr": 0x900000 if dt == "utf8" else None}
         for i, dt in enumerate(dtypes)], n_rows)


def refuse(status, cause, build, bkeys, probe, pkeys, join_type="full", **kw):
    with pytest.raises(api.DDError) as ei:
        api.outer_join(build, bkeys, probe, pkeys, join_type, **kw)
    assert ei.value.status == status, str(ei.value)
    assert cause in str(ei.value), str(ei.value)


@pytest.mark.parametrize("join_type", ["inner", "left_semi", "left_anti", "right_semi",
                                       "right_anti"])
def test_refuses_the_other_join_types(join_type):
    refuse(INVALID, "dd_hash_join_run", fake(["i64"]), [0], fake(["i64"]), [0], join_type)


@pytest.mark.parametrize("join_type,nb,npr,total", [("right", 2048, 2**20, 2147483648),
                                                    ("right", 4096, 2**20 + 1, 4294971392),
                                                    ("full", 2048, 2**20, 2147483648)])
def test_refuses_an_output_of_2_31_rows_or_more(main_sides, join_type, nb, npr, total):
    """test_gpu_hash_join.py's limit shapes through the outer entry: one i32 key value on
    both sides, one partition, no projected column. 2048 x 2^20 is exactly 2^31 rows;
    4096 x (2^20 + 1) is 2^32 + 4096, which 32 bits read as 4096. Under "full" the total
    comes from the one count array that spans both sections: 2^31 from the probe rows, 0
    from the build rows, every one of which is matched. The printed wall time is the
    measurement DESIGN.md §20 quotes. After the refusal the same entry joins the main shape
    and matches the model."""
    assert nb * npr == total >= 2**31
    bb = api.DeviceBatch([col("i32", np.full(nb, 7, dtype=np.int32))])
    pb = api.DeviceBatch([col("i32", np.full(npr, 7, dtype=np.int32))])
    try:
        t0 = time.perf_counter()
        with pytest.raises(api.DDError) as ei:
            api.outer_join(bb, [0], pb, [0], join_type, build_proj=[], probe_proj=[])
        seconds = time.perf_counter() - t0
    finally:
        bb.free()
        pb.free()
    print(f"{join_type} {nb} x {npr}: refused after {seconds * 1e3:.1f} ms")
    assert ei.value.status == UNSUPPORTED, str(ei.value)
    assert f"output of {total} rows is 2^31 or more" in str(ei.value), str(ei.value)
    build, blay, probe, play = main_sides
    r = check_outer(build, [0], probe, [0], join_type, blay, play)
    assert r["n_rows"] > 7001


def test_refuses_unknown_join_types():
    with pytest.raises(ValueError, match="unknown join type"):
        api.outer_join(fake(["i64"]), [0], fake(["i64"]), [0], "left_mark")
    import ctypes
    a = fake(["i64"])
    k = (ctypes.c_int32 * 1)(0)
    off = (ctypes.c_int64 * 2)(0, 8)
    part = (ctypes.c_int32 * 1)(0)
    h = ctypes.c_void_p()
    for t in (-1, 8):
        st = api.lib().dd_hash_join_outer_run(
            ctypes.byref(a.desc), k, ctypes.byref(a.desc), k, ctypes.c_int32(1),
            ctypes.c_int32(t), off, part, ctypes.c_int32(1), ctypes.c_int32(1), off, part,
            ctypes.c_int32(1), ctypes.c_int32(1), k, ctypes.c_int32(0), k, ctypes.c_int32(0),
            None, ctypes.byref(h))
        assert st == INVALID and b"unknown join type" in api.lib().dd_last_error()


@pytest.mark.parametrize("dt,cause", [("f32", "f32 / f64 keys"), ("f64", "f32 / f64 keys"),
                                      ("dict32", "dict32 keys"), ("utf8", "utf8"),
                                      ("dec128", "dec128 keys")])
@pytest.mark.parametrize("join_type", TYPES)
def test_refuses_key_dtypes(dt, cause, join_type):
    refuse(UNSUPPORTED, cause, fake([dt, "i64"]), [0], fake([dt, "i64"]), [0], join_type)
    refuse(UNSUPPORTED, cause, fake(["i64", dt]), [0, 1], fake(["i64", dt]), [0, 1], join_type)


@pytest.mark.parametrize("dt,cause", [("utf8", "var-width"), ("dict32", "dict32 column")])
def test_refuses_projection_dtypes(dt, cause):
    refuse(UNSUPPORTED, cause, fake(["i64", dt]), [0], fake(["i64"]), [0])
    refuse(UNSUPPORTED, cause, fake(["i64"]), [0], fake(["i64", dt]), [0])
    # not projected: not refused for it (no device work either: right, empty probe side)
    j = api.outer_join(fake(["i64", dt]), [0], fake(["i64"], n_rows=0), [0], "right",
                       build_proj=[0])
    assert j.n_rows == 0 and j.seg_offsets().tolist() == [0, 0]
    j.destroy()


def test_refuses_invalid_arguments():
    five = fake(["i32"] * 5)
    refuse(UNSUPPORTED, "more than 4 key", five, list(range(5)), five, list(range(5)))
    a, b = fake(["i64", "i32"]), fake(["i64", "i32"])
    refuse(INVALID, "key dtypes differ pairwise", a, [0], b, [1])
    refuse(INVALID, "key column index out of range", a, [2], b, [0])
    refuse(INVALID, "projected column index out of range", a, [0], b, [0], build_proj=[2])
    refuse(INVALID, "projected column index out of range", a, [0], b, [0], probe_proj=[-1])
    big = fake(["i64"], n_rows=2**31)
    refuse(INVALID, "build side: n_rows must be below 2^31", big, [0], fake(["i64"]), [0])
    refuse(INVALID, "probe side: n_rows must be below 2^31", fake(["i64"]), [0], big, [0])
    with pytest.raises(ValueError, match="same number of key columns"):
        api.outer_join(a, [0, 1], b, [0], "left")


def test_refuses_layouts():
    a, b = fake(["i64"]), fake(["i64"])
    lay = lambda off, part, P: {"seg_offsets": off, "seg_part": part, "n_parts": P}
    ok2 = lay([0, 3, 8], [0, 1], 2)
    refuse(INVALID, "unequal n_parts", a, [0], b, [0], build_layout=ok2,
           probe_layout=lay([0, 8], [0], 1))
    for bad, cause in [(lay([0, 3, 7], [0, 1], 2), "seg_offsets must run from 0 to n_rows"),
                       (lay([0, 9, 8], [0, 1], 2), "seg_offsets decrease"),
                       (lay([0, 3, 8], [0, 2], 2), "seg_part outside"),
                       (lay([0, 8], [0], 0), "at least one segment and one partition")]:
        refuse(INVALID, "malformed build segment layout: " + cause, a, [0], b, [0],
               build_layout=bad, probe_layout=ok2)
        refuse(INVALID, "malformed probe segment layout: " + cause, a, [0], b, [0],
               build_layout=ok2, probe_layout=bad)
    with pytest.raises(ValueError, match="one entry more"):
        api.outer_join(a, [0], b, [0], "full", build_layout=lay([0, 8], [0, 1], 2),
                       probe_layout=ok2)


def test_both_sides_empty_needs_no_device_work():
    """Made-up pointers: the run returns before anything could follow them."""
    for t in TYPES:
        j = api.outer_join(fake(["i64"], n_rows=0), [0], fake(["i64"], n_rows=0), [0], t)
        assert j.n_rows == 0 and not j.seg_offsets().any()
        assert len(j.seg_offsets()) == (2 if t == "right" else 3)
        j.destroy()
