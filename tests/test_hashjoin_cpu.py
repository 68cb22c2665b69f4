"""hashjoin.hash_join_ref (the model api.hash_join is held to) against
pyarrow.Table.join, with no GPU: all five join types, duplicate keys on both sides, NULL
keys (which never match, and which an anti join returns), one partition and many.

Row ids ride along as columns, so a pyarrow result names the (build row, probe row) pairs
or the surviving rows. In the multi-partition cases rows are routed with
oracle.repartition, one pyarrow join runs per partition, and the model must give exactly
the concatenation, segment by segment."""

import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_distributed_amd import hashjoin

PA_TYPE = {"inner": "inner", "left_semi": "left semi", "left_anti": "left anti",
           "right_semi": "right semi", "right_anti": "right anti"}
NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64}


def make_sides(seed, dtypes, nb, npr, n_values, null_frac=0.1):
    """Two sides whose key TUPLES draw from one pool of n_values tuples, so both sides
    repeat and most keys meet; NULLs fall per component. Row ids are positions."""
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
    """pyarrow table of `rows` of key columns `cols` plus their row ids."""
    arrays = {}
    for k, c in enumerate(cols):
        mask = None if c.get("valid") is None else ~np.asarray(c["valid"][rows]).astype(bool)
        arrays[f"k{k}"] = pa.array(np.asarray(c["data"])[rows], mask=mask)
    arrays[id_name] = pa.array(np.asarray(rows, dtype=np.int64))
    return pa.table(arrays)


def arrow_join(build, probe, brows, prows, join_type):
    """What pyarrow says for the rows brows x prows: sorted (b, p) pairs, or sorted ids."""
    nk = len(build)
    keys = [f"k{k}" for k in range(nk)]
    tb, tp = table(build, brows, "b_id"), table(probe, prows, "p_id")
    j = tb.join(tp, keys=keys, right_keys=keys, join_type=PA_TYPE[join_type])
    if join_type == "inner":
        return sorted(zip(j["b_id"].to_pylist(), j["p_id"].to_pylist()),
                      key=lambda bp: (bp[1], bp[0]))
    return sorted(j["b_id" if join_type.startswith("left") else "p_id"].to_pylist())


def route(cols, P):
    """Rows routed to P partitions by the shuffle's hash: (cols in partition-major order,
    layout with one segment per partition)."""
    ref = oracle.repartition(cols, list(range(len(cols))), P)
    out = [{"dtype": c["dtype"], "data": oc["data"], "valid": oc.get("valid")}
           for c, oc in zip(cols, ref["cols"])]
    return out, {"seg_offsets": np.asarray(ref["part_offsets"], dtype=np.int64),
                 "seg_part": np.arange(P, dtype=np.int32), "n_parts": P}


def check_against_arrow(build, probe, join_type, blay=None, play=None):
    nk = len(build)
    got = hashjoin.hash_join_ref(build, list(range(nk)), probe, list(range(nk)), join_type,
                                 blay, play)
    nb, npr = len(build[0]["data"]), len(probe[0]["data"])
    blay = blay or hashjoin.default_layout(nb)
    play = play or hashjoin.default_layout(npr)
    P = blay["n_parts"]
    rows_b = [np.concatenate([np.arange(blay["seg_offsets"][s], blay["seg_offsets"][s + 1])
                              for s in range(len(blay["seg_part"]))
                              if blay["seg_part"][s] == p] + [np.zeros(0, dtype=np.int64)])
              .astype(np.int64) for p in range(P)]
    rows_p = [np.concatenate([np.arange(play["seg_offsets"][s], play["seg_offsets"][s + 1])
                              for s in range(len(play["seg_part"]))
                              if play["seg_part"][s] == p] + [np.zeros(0, dtype=np.int64)])
              .astype(np.int64) for p in range(P)]
    emit = blay if join_type.startswith("left") else play
    assert len(got) == len(emit["seg_part"])
    per_part = [arrow_join(build, probe, rows_b[p], rows_p[p], join_type) for p in range(P)]
    total = 0
    for s, seg in enumerate(got):
        lo, hi = int(emit["seg_offsets"][s]), int(emit["seg_offsets"][s + 1])
        p = int(emit["seg_part"][s])
        if join_type == "inner":
            want = [bp for bp in per_part[p] if lo <= bp[1] < hi]
            # the model lists a probe row's matches in ascending build row
            assert [tuple(x) for x in seg] == want, f"segment {s}"
        else:
            want = [r for r in per_part[p] if lo <= r < hi]
            assert list(seg) == want, f"segment {s}"
        total += len(seg)
    assert total == sum(len(x) for x in per_part)
    return got, total


@pytest.mark.parametrize("join_type", sorted(PA_TYPE))
@pytest.mark.parametrize("dtypes", [("i64",), ("i32",), ("i16",), ("u8",), ("bool",),
                                    ("i64", "i32"), ("u8", "bool"),
                                    ("i64", "i32", "i16", "u8")])
def test_single_partition_matches_pyarrow(join_type, dtypes):
    build, probe = make_sides(sum(map(ord, join_type)) + 10 * len(dtypes), dtypes, 300, 400, 60)
    _, total = check_against_arrow(build, probe, join_type)
    assert total > 0


@pytest.mark.parametrize("join_type", sorted(PA_TYPE))
@pytest.mark.parametrize("P", [2, 7])
def test_partitioned_matches_per_partition_pyarrow(join_type, P):
    build, probe = make_sides(40 + P, ("i64", "i32"), 500, 700, 120)
    b, blay = route(build, P)
    p, play = route(probe, P)
    _, total = check_against_arrow(b, p, join_type, blay, play)
    assert total > 0


@pytest.mark.parametrize("join_type", sorted(PA_TYPE))
def test_exchanged_style_layout_with_empty_segments(join_type):
    """S = producers * parts on the probe side, one segment per partition on the build
    side: the output keeps the emitting side's segments."""
    build, probe = make_sides(77, ("i32",), 200, 300, 40)
    P = 3
    b, blay = route(build, P)
    halves = [route([{**c, "data": c["data"][h::2],
                      "valid": None if c["valid"] is None else c["valid"][h::2]}
                     for c in probe], P) for h in (0, 1)]
    p = [{"dtype": c0["dtype"], "data": np.concatenate([c0["data"], c1["data"]]),
          "valid": np.concatenate([c0["valid"], c1["valid"]])}
         for c0, c1 in zip(halves[0][0], halves[1][0])]
    n0 = int(halves[0][1]["seg_offsets"][-1])
    # three producers, the middle one empty: P empty segments between the real ones
    off = np.concatenate([halves[0][1]["seg_offsets"], np.full(P, n0, dtype=np.int64),
                          halves[1][1]["seg_offsets"][1:] + n0])
    part = (np.arange(3 * P) % P).astype(np.int32)
    play = {"seg_offsets": off, "seg_part": part, "n_parts": P}
    check_against_arrow(b, p, join_type, blay, play)


@pytest.mark.parametrize("join_type", sorted(PA_TYPE))
def test_equal_keys_in_different_partitions_do_not_match(join_type):
    """Key 5 sits in partition 0 of the build side and partition 1 of the probe side."""
    build = [{"dtype": "i64", "data": np.array([5, 5, 9], dtype=np.int64), "valid": None}]
    probe = [{"dtype": "i64", "data": np.array([7, 5, 5, 5], dtype=np.int64), "valid": None}]
    blay = {"seg_offsets": [0, 2, 3], "seg_part": [0, 1], "n_parts": 2}
    play = {"seg_offsets": [0, 1, 4], "seg_part": [0, 1], "n_parts": 2}
    got, total = check_against_arrow(build, probe, join_type, blay, play)
    want = {"inner": [[], []], "left_semi": [[], []], "right_semi": [[], []],
            "left_anti": [[0, 1], [2]], "right_anti": [[0], [1, 2, 3]]}[join_type]
    assert [list(s) for s in got] == want
    # the same rows in ONE partition do match
    flat = hashjoin.hash_join_ref(build, [0], probe, [0], "inner")
    assert sorted(flat[0]) == [(b, p) for b in (0, 1) for p in (1, 2, 3)]


def test_null_keys_never_match_and_anti_returns_them():
    v = np.array([1, 0, 1], dtype=np.uint8)
    build = [{"dtype": "i32", "data": np.array([4, 4, 8], dtype=np.int32), "valid": v}]
    probe = [{"dtype": "i32", "data": np.array([4, 8, 4], dtype=np.int32),
              "valid": np.array([0, 1, 1], dtype=np.uint8)}]
    ref = lambda t: hashjoin.hash_join_ref(build, [0], probe, [0], t)[0]
    assert ref("inner") == [(2, 1), (0, 2)]
    assert ref("left_semi") == [0, 2] and ref("left_anti") == [1]
    assert ref("right_semi") == [1, 2] and ref("right_anti") == [0]
    for t in PA_TYPE:
        check_against_arrow(build, probe, t)


def test_model_refuses_what_the_join_refuses():
    i64 = [{"dtype": "i64", "data": np.zeros(2, dtype=np.int64), "valid": None}]
    i32 = [{"dtype": "i32", "data": np.zeros(2, dtype=np.int32), "valid": None}]
    f64 = [{"dtype": "f64", "data": np.zeros(2), "valid": None}]
    with pytest.raises(ValueError, match="join type"):
        hashjoin.hash_join_ref(i64, [0], i64, [0], "left")
    with pytest.raises(ValueError, match="differ pairwise"):
        hashjoin.hash_join_ref(i64, [0], i32, [0])
    with pytest.raises(ValueError, match="f64 key"):
        hashjoin.hash_join_ref(f64, [0], f64, [0])
    with pytest.raises(ValueError, match="n_parts"):
        hashjoin.hash_join_ref(i64, [0], i64, [0], "inner",
                               {"seg_offsets": [0, 2], "seg_part": [0], "n_parts": 1},
                               {"seg_offsets": [0, 2], "seg_part": [0], "n_parts": 2})
