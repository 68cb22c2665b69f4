"""Wide rounds of the pre path (marked gpu): k_scatter_pre_wide scatters 8192-row rounds
in two column passes (gmax 8 x wpb 16, round layout only) on the headline (8,8,8,4),
dictkey (4,8,8,4) and multikey (8,8,8,4,4) shapes at P <= 128. Every case is bit-exact
against the CPU oracle and asserts Partitioner.pre_wide() and the plan info() reports.
Row counts sit on the edges of R = 8192: a single row, a wave group plus a row, one wave
segment (512) plus a row, R-1, R, R+1, whole rounds, whole rounds plus a ragged one, and
~12 rounds."""

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from tests.test_gpu_fuzz import random_col
from tests.test_gpu_parity import check_against_oracle, compare_to_oracle

pytestmark = pytest.mark.gpu

R = 8192
Q3 = ["i64", "f64", "f64", "i32"]      # headline: elems 8, 8, 8, 4
DK = ["dict32", "f64", "f64", "i32"]   # dictkey: 4, 8, 8, 4
MK = Q3 + ["i32"]                      # multikey: 8, 8, 8, 4, 4
Q1 = ["u8", "bool", "f64", "f64", "f64", "f64", "i32"]  # q1: not a wide shape

SHAPES = {"q3": (Q3, [0]), "dk": (DK, [0]), "mk": (MK, [0, 4]), "q1": (Q1, [0, 1])}
KNOBS = ("DD_PRE_WIDE", "DD_PRE_WIDE_MIN_ROWS", "DD_PRE_LAYOUT", "DD_PRE_XCD",
         "DD_PRE_RPB", "DD_PID8", "DD_PRE_WPB", "DD_PRE_GMAX", "DD_PRE_SCAN_SPAN",
         "DD_K3_PRE", "DD_K3_HL", "DD_RHASH", "DD_K1_SPEC")
NMAX = 100_003
ROWS = [1, 65, 513, R - 1, R, R + 1, 3 * R, 3 * R + 17, NMAX]
WIDE = {"path": 2, "gmax": 8, "wpb": 16, "round_rows": R}
NARROW = {"path": 2, "gmax": 4, "wpb": 16, "round_rows": 4096}

_DATA = {}


def shape_cols(shape, n):
    """The first n rows of the shape's (cached, seeded) NMAX-row batch."""
    if shape not in _DATA:
        rng = np.random.default_rng(sum(map(ord, shape)) + 606)
        _DATA[shape] = [random_col(rng, NMAX, dt, 0) for dt in SHAPES[shape][0]]
    return [{**c, "data": c["data"][:n], "valid": None} for c in _DATA[shape]]


def clear_knobs(monkeypatch, env=None):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)


def check(monkeypatch, cols, key_idx, nparts, env, wide, expect=None):
    """check_against_oracle under `env`, asserting pre_wide() == wide and the matching
    gmax / round_rows (plus `expect`) on the partitioner the run creates."""
    clear_knobs(monkeypatch, env)
    seen = []

    class Checked(api.Partitioner):
        def run(self, stream=None):
            seen.append(self.pre_wide())
            super().run(stream)

    monkeypatch.setattr(api, "Partitioner", Checked)
    check_against_oracle(cols, key_idx, nparts,
                         expect={**(WIDE if wide else {}), **(expect or {})})
    assert seen == [1 if wide else 0], f"pre_wide() = {seen}"


EDGE_CASES = [(s, p, n) for s in ("q3", "dk", "mk") for p in (1, 2, 100, 128) for n in ROWS]


@pytest.mark.parametrize("shape,nparts,n", EDGE_CASES,
                         ids=[f"{s}_p{p}-{n}" for s, p, n in EDGE_CASES])
def test_round_edges(shape, nparts, n, monkeypatch):
    check(monkeypatch, shape_cols(shape, n), SHAPES[shape][1], nparts,
          {"DD_PRE_WIDE": "1"}, True, expect={"n_launch": -(-n // R)})


@pytest.mark.parametrize("shape", ["q3", "dk", "mk"])
@pytest.mark.parametrize("skew", ["one_key", "two_keys", "presorted"])
def test_skew(shape, skew, monkeypatch):
    """one_key: every row in one partition, so roundcnt = 8192, the last segment's
    segoff = 7680 (the u16 edges), a wave's rank reaches 512 and pslot is constant;
    two_keys; presorted: input already in partition order."""
    key_idx, nparts, n = SHAPES[shape][1], 128, 3 * R + 17
    cols = shape_cols(shape, n)
    if skew == "presorted":
        pid = oracle.pids(oracle.hash_cols([cols[k] for k in key_idx], n), nparts)
        perm = np.argsort(pid, kind="stable")
        cols = [{**c, "data": np.ascontiguousarray(c["data"][perm])} for c in cols]
    else:
        for k in key_idx:
            d = np.zeros(n, dtype=cols[k]["data"].dtype)
            if skew == "two_keys":  # dict32: index 1 needs a second dictionary value
                hi = 1 if cols[k]["dtype"] != "dict32" else \
                    min(1, len(cols[k]["dict_offsets"]) - 2)
                d[np.random.default_rng(5).random(n) < 0.3] = hi
            cols[k] = {**cols[k], "data": d}
    check(monkeypatch, cols, key_idx, nparts, {"DD_PRE_WIDE": "1"}, True)


KNOB_CASES = [
    ({"DD_PRE_RPB": "1"}, {"rpb": 1}),
    ({"DD_PRE_RPB": "2"}, {"rpb": 2}),
    ({"DD_PRE_RPB": "256"}, {"rpb": 256}),
    ({"DD_PRE_XCD": "0"}, {}),
    ({"DD_PRE_XCD": "1"}, {}),
    ({"DD_PRE_XCD": "1", "DD_PRE_RPB": "1"}, {"rpb": 1}),
    ({"DD_PID8": "0"}, {"pid_elem": 4}),
    ({"DD_PRE_SCAN_SPAN": "1"}, {}),
    ({"DD_K1_SPEC": "0"}, {}),
]


@pytest.mark.parametrize("shape", ["q3", "mk"])
@pytest.mark.parametrize("env,expect", KNOB_CASES,
                         ids=["-".join(f"{k}={v}" for k, v in e.items())
                              for e, _ in KNOB_CASES])
def test_knobs(shape, env, expect, monkeypatch):
    """The pre path's knobs under the wide form. 100,003 rows are 13 rounds, the last
    ragged: rpb 1 and 2 give 13 and 7 blocks, rpb 256 one block that walks every round;
    DD_PRE_SCAN_SPAN=1 gives 13 one-round ranges (one level; the two-level scan has its
    own case below)."""
    check(monkeypatch, shape_cols(shape, NMAX), SHAPES[shape][1], 128,
          {"DD_PRE_WIDE": "1", **env}, True, expect=expect)
    if "DD_K1_SPEC" in env:
        clear_knobs(monkeypatch, {"DD_PRE_WIDE": "1", **env})
        batch = api.DeviceBatch(shape_cols(shape, 65))
        part = api.Partitioner(batch, SHAPES[shape][1], 128)
        try:
            assert part.k1_spec() == 0 and part.pre_wide() == 1
        finally:
            part.destroy()
            batch.free()


def test_two_level_scan(monkeypatch):
    """DD_PRE_SCAN_SPAN=1 with more than 16 rounds: 17 ranges > 16 * span, so the
    round-granular scan takes its two-level form under the wide geometry."""
    n = 16 * R + 100
    rng = np.random.default_rng(n)
    cols = [random_col(rng, n, dt, 0) for dt in Q3]
    check(monkeypatch, cols, [0], 128, {"DD_PRE_WIDE": "1", "DD_PRE_SCAN_SPAN": "1"},
          True, expect={"n_launch": 17})


def test_selection(monkeypatch):
    """Default at 100,003 rows is narrow; DD_PRE_WIDE_MIN_ROWS=20000 makes the same batch
    wide (and leaves a 10,000-row one narrow); DD_PRE_WIDE=0 and DD_PRE_LAYOUT=seg keep it
    narrow whatever else is set."""
    cols, small = shape_cols("q3", NMAX), shape_cols("q3", 10_000)
    check(monkeypatch, cols, [0], 128, {}, False, expect=NARROW)
    check(monkeypatch, cols, [0], 128, {"DD_PRE_WIDE_MIN_ROWS": "20000"}, True)
    check(monkeypatch, small, [0], 128, {"DD_PRE_WIDE_MIN_ROWS": "20000"}, False,
          expect=NARROW)
    check(monkeypatch, cols, [0], 128, {"DD_PRE_WIDE": "0"}, False, expect=NARROW)
    check(monkeypatch, cols, [0], 128,
          {"DD_PRE_WIDE": "0", "DD_PRE_WIDE_MIN_ROWS": "20000"}, False, expect=NARROW)
    check(monkeypatch, cols, [0], 128, {"DD_PRE_WIDE": "1", "DD_PRE_LAYOUT": "seg"},
          False, expect=NARROW)


@pytest.mark.parametrize("shape,nparts,expect", [
    ("q1", 128, {"path": 2, "gmax": 2, "round_rows": 2048}),   # not a wide shape
    ("q3", 129, NARROW),                                       # past the P <= 128 tier
])
def test_ineligible_stays_narrow(shape, nparts, expect, monkeypatch):
    check(monkeypatch, shape_cols(shape, 3 * R + 17), SHAPES[shape][1], nparts,
          {"DD_PRE_WIDE": "1"}, False, expect=expect)


@pytest.mark.parametrize("shape", ["q3", "dk", "mk"])
def test_reuse_and_narrow_equal(shape, monkeypatch):
    """One wide partitioner: run twice, then refill the input in place with other data of
    the same shape (every key equal, then reversed keys, then the first batch again).
    Each result equals the oracle's, and the narrow form's output of the first batch is
    array_equal to the wide form's."""
    key_idx, nparts, n = SHAPES[shape][1], 128, 3 * R + 17
    k0 = key_idx[0]
    a = shape_cols(shape, n)
    b = [dict(c) for c in a]
    b[k0]["data"] = np.zeros(n, dtype=a[k0]["data"].dtype)
    c = [dict(x) for x in a]
    c[k0]["data"] = np.ascontiguousarray(a[k0]["data"][::-1])
    refs = [oracle.repartition(x, key_idx, nparts) for x in (a, b, c)]

    outs = {}
    for form in ("1", "0"):
        clear_knobs(monkeypatch, {"DD_PRE_WIDE": form})
        batch = api.DeviceBatch(a)
        part = api.Partitioner(batch, key_idx, nparts)
        try:
            info = part.info()
            assert part.pre_wide() == int(form)
            assert (info["gmax"], info["round_rows"]) == ((8, R) if form == "1"
                                                          else (4, 4096))
            for _ in range(2):
                part.run()
                part.sync()
                compare_to_oracle(part, a, key_idx, nparts, ref=refs[0])
            outs[form] = (part.row_offsets(),
                          [part.col_out(i)["data"].copy() for i in range(len(a))])
            if form == "1":
                for cols, ref in ((b, refs[1]), (c, refs[2]), (a, refs[0])):
                    batch.refill(cols)
                    part.run()
                    part.sync()
                    compare_to_oracle(part, cols, key_idx, nparts, ref=ref)
                assert np.array_equal(outs["1"][0], part.row_offsets())
        finally:
            part.destroy()
            batch.free()
    assert np.array_equal(outs["1"][0], outs["0"][0])
    for w, nrw in zip(outs["1"][1], outs["0"][1]):
        assert np.array_equal(w.view(np.uint8), nrw.view(np.uint8))
