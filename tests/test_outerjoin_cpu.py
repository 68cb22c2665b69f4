"""hashjoin.outer_join_ref (the model api.outer_join is held to) against
pyarrow.Table.join, with no GPU: left, right and full, duplicate keys on both sides, NULL
keys (rows without a match, kept by the side that preserves them), one partition and many.

Row ids ride along as columns; pyarrow runs one join per partition and the multiset of
(b_id | None, p_id | None) per partition must be the model's. WHERE the rows stand (two
sections, probe row order, a probe row's matches adjacent and ascending, the unmatched
build rows of build segment s in segment S_p + s in row order) is asserted against the
definition in §20, not against pyarrow, which promises no order."""

import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_distributed_amd import hashjoin

PA_TYPE = {"left": "left outer", "right": "right outer", "full": "full outer"}
TYPES = sorted(PA_TYPE)
NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64}


def make_sides(seed, dtypes, nb, npr, n_values, null_frac=0.1):
    """Two sides whose key TUPLES draw from one pool of n_values tuples, so both sides
    repeat and most keys meet; NULLs fall per component."""
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
            n = len(pick)
            valid = (rng.random(n) >= null_frac).astype(np.uint8) if null_frac else None
            side.append({"dtype": dt, "data": pool[pick], "valid": valid})
    return build, probe


def table(cols, rows, id_name):
    arrays = {}
    for k, c in enumerate(cols):
        mask = None if c.get("valid") is None else ~np.asarray(c["valid"])[rows].astype(bool)
        arrays[f"k{k}"] = pa.array(np.asarray(c["data"])[rows], mask=mask)
    arrays[id_name] = pa.array(np.asarray(rows, dtype=np.int64))
    return pa.table(arrays)


def arrow_pairs(build, probe, brows, prows, join_type):
    """pyarrow's (b_id | None, p_id | None) for the rows brows x prows, sorted."""
    keys = [f"k{k}" for k in range(len(build))]
    j = table(build, brows, "b_id").join(table(probe, prows, "p_id"), keys=keys,
                                         right_keys=keys, join_type=PA_TYPE[join_type])
    return sorted(zip(j["b_id"].to_pylist(), j["p_id"].to_pylist()), key=sort_key)


def sort_key(bp):
    return (bp[0] is None, bp[0] or 0, bp[1] is None, bp[1] or 0)


def route(cols, P):
    """Rows routed to P partitions by the shuffle's hash, one segment per partition."""
    ref = oracle.repartition(cols, list(range(len(cols))), P)
    out = [{"dtype": c["dtype"], "data": oc["data"], "valid": oc.get("valid")}
           for c, oc in zip(cols, ref["cols"])]
    return out, {"seg_offsets": np.asarray(ref["part_offsets"], dtype=np.int64),
                 "seg_part": np.arange(P, dtype=np.int32), "n_parts": P}


def rows_of(lay, p):
    off, part = np.asarray(lay["seg_offsets"]), np.asarray(lay["seg_part"])
    return np.concatenate([np.arange(off[s], off[s + 1]) for s in range(len(part))
                           if part[s] == p] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def check_structure(got, join_type, blay, play):
    """§20's layout and order, from the definition alone."""
    S_p, S_b = len(play["seg_part"]), len(blay["seg_part"])
    assert len(got) == (S_p if join_type == "right" else S_p + S_b)
    poff, boff = np.asarray(play["seg_offsets"]), np.asarray(blay["seg_offsets"])
    matched = set()
    for s in range(S_p):
        seg = got[s]
        assert all(p is not None and poff[s] <= p < poff[s + 1] for _, p in seg)
        # probe row order, a row's matches adjacent and in ascending build row
        assert [p for _, p in seg] == sorted(p for _, p in seg)
        by_row = {}
        for b, p in seg:
            by_row.setdefault(p, []).append(b)
        for p, bs in by_row.items():
            assert bs == [None] or (None not in bs and bs == sorted(set(bs)))
        if join_type == "left":
            assert all(b is not None for b, _ in seg)
        else:  # every probe row of the segment stands there at least once
            assert sorted(by_row) == list(range(int(poff[s]), int(poff[s + 1])))
        matched.update(b for b, _ in seg if b is not None)
    for s in range(S_b if join_type != "right" else 0):
        rows = [r for r in range(int(boff[s]), int(boff[s + 1])) if r not in matched]
        assert got[S_p + s] == [(r, None) for r in rows], f"build segment {s}"


def check_against_arrow(build, probe, join_type, blay=None, play=None):
    nk = len(build)
    got = hashjoin.outer_join_ref(build, list(range(nk)), probe, list(range(nk)), join_type,
                                  blay, play)
    blay = blay or hashjoin.default_layout(hashjoin.n_rows_of(build))
    play = play or hashjoin.default_layout(hashjoin.n_rows_of(probe))
    check_structure(got, join_type, blay, play)
    part = np.concatenate([play["seg_part"], blay["seg_part"]])
    total = 0
    for p in range(blay["n_parts"]):
        mine = sorted((x for s, seg in enumerate(got) if part[s] == p for x in seg),
                      key=sort_key)
        want = arrow_pairs(build, probe, rows_of(blay, p), rows_of(play, p), join_type)
        assert mine == want, f"partition {p}"
        total += len(mine)
    assert total == sum(len(s) for s in got)
    return got, total


@pytest.mark.parametrize("join_type", TYPES)
@pytest.mark.parametrize("dtypes", [("i64",), ("i32",), ("i16",), ("u8",), ("bool",),
                                    ("i64", "i32"), ("u8", "bool"), ("i16", "i64", "i32"),
                                    ("i64", "i32", "i16", "u8")])
def test_single_partition_matches_pyarrow(join_type, dtypes):
    build, probe = make_sides(sum(map(ord, join_type)) + 10 * len(dtypes), dtypes, 300, 400, 60)
    got, total = check_against_arrow(build, probe, join_type)
    assert total > 400 and any(None in x for seg in got for x in seg)


@pytest.mark.parametrize("join_type", TYPES)
@pytest.mark.parametrize("P", [2, 7])
def test_partitioned_matches_per_partition_pyarrow(join_type, P):
    build, probe = make_sides(40 + P, ("i64", "i32"), 500, 700, 120)
    b, blay = route(build, P)
    p, play = route(probe, P)
    check_against_arrow(b, p, join_type, blay, play)


def producers(cols, P, n_prod, empty=()):
    """n_prod producers' windows one behind the other (S = n_prod * P, seg_part = s % P);
    the producers in `empty` contribute P empty segments."""
    live = [i for i in range(n_prod) if i not in empty]
    parts = {i: route([{**c, "data": c["data"][k::len(live)],
                        "valid": None if c["valid"] is None else c["valid"][k::len(live)]}
                       for c in cols], P) for k, i in enumerate(live)}
    off, base, chunks = [0], 0, []
    for i in range(n_prod):
        if i in parts:
            off += (parts[i][1]["seg_offsets"][1:] + base).tolist()
            base = off[-1]
            chunks.append(parts[i][0])
        else:
            off += [base] * P
    out = [{"dtype": c["dtype"], "data": np.concatenate([ch[k]["data"] for ch in chunks]),
            "valid": None if c["valid"] is None else
            np.concatenate([ch[k]["valid"] for ch in chunks])} for k, c in enumerate(cols)]
    return out, {"seg_offsets": np.array(off, dtype=np.int64),
                 "seg_part": (np.arange(n_prod * P) % P).astype(np.int32), "n_parts": P}


@pytest.mark.parametrize("join_type", TYPES)
def test_several_producers_and_empty_segments(join_type):
    """3 producers on the build side (the middle one empty) against 2 on the probe side:
    a partition owns several segments in both sections."""
    build, probe = make_sides(77, ("i32",), 200, 300, 40)
    b, blay = producers(build, 5, 3, empty=(1,))
    p, play = producers(probe, 5, 2)
    got, _ = check_against_arrow(b, p, join_type, blay, play)
    assert len(got) == (10 if join_type == "right" else 25)


@pytest.mark.parametrize("join_type", TYPES)
@pytest.mark.parametrize("empty", ["build", "probe", "both"])
def test_empty_sides(join_type, empty):
    nb = 0 if empty in ("build", "both") else 50
    npr = 0 if empty in ("probe", "both") else 70
    build, probe = make_sides(5, ("i64",), nb, npr, 20)
    b, blay = route(build, 3)
    p, play = route(probe, 3)
    _, total = check_against_arrow(b, p, join_type, blay, play)
    assert total == (npr if join_type != "left" else 0) + (nb if join_type != "right" else 0)


@pytest.mark.parametrize("join_type", TYPES)
@pytest.mark.parametrize("null_side", ["build", "probe", "both"])
def test_all_null_keys(join_type, null_side):
    build, probe = make_sides(6, ("i32", "u8"), 40, 50, 10, null_frac=0)
    for side, name in ((build, "build"), (probe, "probe")):
        if null_side in (name, "both"):
            side[1]["valid"] = np.zeros(len(side[1]["data"]), dtype=np.uint8)
    got, total = check_against_arrow(build, probe, join_type)
    assert total == (50 if join_type != "left" else 0) + (40 if join_type != "right" else 0)
    assert all(None in x for seg in got for x in seg)


@pytest.mark.parametrize("join_type", TYPES)
def test_no_key_meets_and_every_key_meets(join_type):
    i64 = lambda a: [{"dtype": "i64", "data": np.asarray(a, dtype=np.int64), "valid": None}]
    _, total = check_against_arrow(i64(np.arange(30)), i64(np.arange(100, 140)), join_type)
    assert total == {"left": 30, "right": 40, "full": 70}[join_type]
    got, total = check_against_arrow(i64(np.arange(30) % 10), i64(np.arange(40) % 10),
                                     join_type)
    assert total == 3 * 4 * 10 and not any(None in x for seg in got for x in seg)


def test_small_example_by_hand():
    v = np.array([1, 0, 1, 1], dtype=np.uint8)
    build = [{"dtype": "i32", "data": np.array([4, 4, 8, 4], dtype=np.int32), "valid": v}]
    probe = [{"dtype": "i32", "data": np.array([4, 9, 4], dtype=np.int32),
              "valid": np.array([0, 1, 1], dtype=np.uint8)}]
    ref = lambda t: hashjoin.outer_join_ref(build, [0], probe, [0], t)
    assert ref("right") == [[(None, 0), (None, 1), (0, 2), (3, 2)]]
    assert ref("left") == [[(0, 2), (3, 2)], [(1, None), (2, None)]]
    assert ref("full") == [[(None, 0), (None, 1), (0, 2), (3, 2)], [(1, None), (2, None)]]
    assert hashjoin.seg_offsets_of(ref("full")).tolist() == [0, 4, 6]


def test_equal_keys_in_different_partitions_do_not_match():
    build = [{"dtype": "i64", "data": np.array([5, 5, 9], dtype=np.int64), "valid": None}]
    probe = [{"dtype": "i64", "data": np.array([7, 5, 5, 5], dtype=np.int64), "valid": None}]
    blay = {"seg_offsets": [0, 2, 3], "seg_part": [0, 1], "n_parts": 2}
    play = {"seg_offsets": [0, 1, 4], "seg_part": [0, 1], "n_parts": 2}
    got, _ = check_against_arrow(build, probe, "full", blay, play)
    assert got == [[(None, 0)], [(None, 1), (None, 2), (None, 3)],
                   [(0, None), (1, None)], [(2, None)]]


def test_model_refuses_what_the_join_refuses():
    i64 = [{"dtype": "i64", "data": np.zeros(2, dtype=np.int64), "valid": None}]
    i32 = [{"dtype": "i32", "data": np.zeros(2, dtype=np.int32), "valid": None}]
    f64 = [{"dtype": "f64", "data": np.zeros(2), "valid": None}]
    assert hashjoin.OUTER_JOIN_TYPES == ("left", "right", "full")
    for t in hashjoin.JOIN_TYPES + ("cross",):
        with pytest.raises(ValueError, match="join type"):
            hashjoin.outer_join_ref(i64, [0], i64, [0], t)
    with pytest.raises(ValueError, match="differ pairwise"):
        hashjoin.outer_join_ref(i64, [0], i32, [0], "left")
    with pytest.raises(ValueError, match="f64 key"):
        hashjoin.outer_join_ref(f64, [0], f64, [0], "full")
    with pytest.raises(ValueError, match="1..4 key"):
        hashjoin.outer_join_ref(i64 * 5, list(range(5)), i64 * 5, list(range(5)), "right")
    with pytest.raises(ValueError, match="n_parts"):
        hashjoin.outer_join_ref(i64, [0], i64, [0], "left",
                                {"seg_offsets": [0, 2], "seg_part": [0], "n_parts": 1},
                                {"seg_offsets": [0, 2], "seg_part": [0], "n_parts": 2})
