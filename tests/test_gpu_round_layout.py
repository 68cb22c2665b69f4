"""Pre-path layout precompute (marked gpu): DD_PRE_LAYOUT=seg (k_hash_count_seg, the
segment-granular scan, k_round_roff) against DD_PRE_LAYOUT=round (k_hash_count_round, the
round-granular scan). Every case runs under both values, asserts Partitioner.pre_layout()
and is bit-exact against the CPU oracle, whose result is computed once per case and shared
by the two runs. Row counts sit on the edges of the round size R (4096 or 2048 rows,
read from info()): a single row, one wave segment plus a row, R-1, R, R+1, whole rounds,
whole rounds plus a ragged one, and ~25-49 rounds."""

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from tests.test_gpu_fuzz import random_col
from tests.test_gpu_parity import check_against_oracle, compare_to_oracle

pytestmark = pytest.mark.gpu

Q3 = ["i64", "f64", "f64", "i32"]                        # elems 8, 8, 8, 4
MK = Q3 + ["i32"]                                        # multikey: 8, 8, 8, 4, 4
Q1 = ["u8", "bool", "f64", "f64", "f64", "f64", "i32"]   # q1: 1, 1, 8, 8, 8, 8, 4

# id -> (dtypes, key columns, P, round rows R)
TIERS = {
    "q3_p1": (Q3, [0], 1, 4096), "q3_p2": (Q3, [0], 2, 4096),
    "q3_p100": (Q3, [0], 100, 4096), "q3_p128": (Q3, [0], 128, 4096),
    "q3_p129": (Q3, [0], 129, 4096), "q3_p256": (Q3, [0], 256, 4096),
    "q3_p257": (Q3, [0], 257, 2048), "q3_p300": (Q3, [0], 300, 2048),
    "q3_p512": (Q3, [0], 512, 2048),
    "mk_p128": (MK, [0, 4], 128, 4096), "mk_p512": (MK, [0, 4], 512, 2048),
    "q1_p7": (Q1, [0, 1], 7, 2048), "q1_p128": (Q1, [0, 1], 128, 2048),
}
LAYOUTS = {"seg": 1, "round": 2}
KNOBS = ("DD_PRE_LAYOUT", "DD_PRE_XCD", "DD_PRE_RPB", "DD_PID8", "DD_PRE_WPB",
         "DD_PRE_GMAX", "DD_PRE_SCAN_SPAN", "DD_K3_PRE", "DD_K3_HL", "DD_RHASH")
NMAX = 100_003


def row_counts(R):
    return [1, 65, R - 1, R, R + 1, 3 * R, 3 * R + 17, NMAX]


_DATA = {}


def tier_cols(tier, n):
    """The first n rows of the tier's (cached, seeded) NMAX-row batch."""
    dtypes = TIERS[tier][0]
    if tier not in _DATA:
        rng = np.random.default_rng(sum(map(ord, tier)))
        _DATA[tier] = [random_col(rng, NMAX, dt, 0) for dt in dtypes]
    return [{"dtype": c["dtype"], "data": c["data"][:n], "valid": None}
            for c in _DATA[tier]]


def both_layouts(monkeypatch, cols, key_idx, nparts, env=None, expect=None):
    """check_against_oracle under DD_PRE_LAYOUT=seg and =round, with pre_layout() (and
    the pre path, plus `expect`) asserted on the partitioner each run creates."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    seen = []

    class Checked(api.Partitioner):
        def run(self, stream=None):
            seen.append(self.pre_layout())
            super().run(stream)

    monkeypatch.setattr(api, "Partitioner", Checked)
    refs, repartition = [], oracle.repartition

    def shared_reference(*args):  # one oracle run serves both layouts
        if not refs:
            refs.append(repartition(*args))
        return refs[0]

    monkeypatch.setattr(oracle, "repartition", shared_reference)
    for layout, code in LAYOUTS.items():
        monkeypatch.setenv("DD_PRE_LAYOUT", layout)
        check_against_oracle(cols, key_idx, nparts, expect={"path": 2, **(expect or {})})
        assert seen[-1] == code, f"DD_PRE_LAYOUT={layout}: pre_layout() = {seen[-1]}"
    assert len(seen) == 2


CASES = [(t, i) for t in TIERS for i in range(8)]


@pytest.mark.parametrize("tier,ni", CASES,
                         ids=[f"{t}-{row_counts(TIERS[t][3])[i]}" for t, i in CASES])
def test_round_edges(tier, ni, monkeypatch):
    _, key_idx, nparts, R = TIERS[tier]
    n = row_counts(R)[ni]
    both_layouts(monkeypatch, tier_cols(tier, n), key_idx, nparts,
                 expect={"round_rows": R})


@pytest.mark.parametrize("tier", ["q3_p128", "q3_p512", "mk_p128", "q1_p128"])
@pytest.mark.parametrize("skew", ["one_key", "two_keys", "presorted"])
def test_skew(tier, skew, monkeypatch):
    """one_key: every row in one partition, so roundcnt = R and the last segment's
    segoff = R - SEG (the u16 edges); two_keys; presorted: input already in partition
    order, so each round touches few partitions."""
    _, key_idx, nparts, R = TIERS[tier]
    n = 3 * R + 17
    cols = tier_cols(tier, n)
    if skew == "presorted":
        pid = oracle.pids(oracle.hash_cols([cols[k] for k in key_idx], n), nparts)
        perm = np.argsort(pid, kind="stable")
        cols = [{**c, "data": np.ascontiguousarray(c["data"][perm])} for c in cols]
    else:
        for k in key_idx:
            d = np.full(n, 1, dtype=cols[k]["data"].dtype)
            if skew == "two_keys":
                d[np.random.default_rng(5).random(n) < 0.3] = 0
            cols[k] = {**cols[k], "data": d}
    both_layouts(monkeypatch, cols, key_idx, nparts)


KNOB_CASES = [
    ({"DD_PRE_RPB": "1"}, {"rpb": 1}),
    ({"DD_PRE_RPB": "2"}, {"rpb": 2}),
    ({"DD_PRE_RPB": "3"}, {"rpb": 3}),
    ({"DD_PID8": "0"}, {"pid_elem": 4}),
    ({"DD_PRE_WPB": "8"}, {"wpb": 8, "round_rows": 2048}),
    ({"DD_PRE_GMAX": "2"}, {"gmax": 2, "round_rows": 2048}),
]


@pytest.mark.parametrize("env,expect", KNOB_CASES,
                         ids=["-".join(f"{k}={v}" for k, v in e.items())
                              for e, _ in KNOB_CASES])
def test_knobs(env, expect, monkeypatch):
    both_layouts(monkeypatch, tier_cols("q3_p128", 5 * 4096 + 17), [0], 128, env=env,
                 expect=expect)


@pytest.mark.parametrize("xcd", ["0", "1"])
@pytest.mark.parametrize("nblocks", [1, 7, 8, 9, 17])
def test_xcd_order(nblocks, xcd, monkeypatch):
    """DD_PRE_XCD=1 (the round layout's default) re-orders which block scatters which
    rounds, =0 keeps launch order; neither changes an output. One round per block, the
    last round ragged."""
    n = nblocks * 4096 - 100
    both_layouts(monkeypatch, tier_cols("q3_p128", n), [0], 128,
                 env={"DD_PRE_XCD": xcd, "DD_PRE_RPB": "1"},
                 expect={"rpb": 1, "n_launch": nblocks})


def test_xcd_order_two_rounds_per_block(monkeypatch):
    both_layouts(monkeypatch, tier_cols("q3_p128", 21 * 4096 + 5), [0], 128,
                 env={"DD_PRE_XCD": "1"}, expect={"rpb": 2, "n_launch": 22})


@pytest.mark.parametrize("tier,n,span", [
    ("q3_p128", NMAX, "1"),           # 25 rounds: 25 ranges > 16, two levels, 25 groups
    ("q3_p128", NMAX, "3"),           # 9 ranges of 3 rounds (the last one short), one level
    ("q3_p300", NMAX, "1"),           # 49 rounds of 2048 rows: two levels, 49 groups
    ("q3_p257", 71 * 2048 + 5, "2"),  # 71 rounds: 36 ranges > 32, two levels, 18 groups
    ("q3_p257", 71 * 2048 + 5, "5"),  # 15 ranges, one level, odd P (zero pad column)
])
def test_scan_levels(tier, n, span, monkeypatch):
    """The round-granular scan at both depths. The two-level form serves > 65 k rounds
    (> 268 M rows) at the default span of 64 rounds per range; DD_PRE_SCAN_SPAN shrinks the
    span so a small batch takes it: ranges = ceil(rounds / span), two levels when
    ranges > 16 * span."""
    dtypes, key_idx, nparts, R = TIERS[tier]
    if n <= NMAX:
        cols = tier_cols(tier, n)
    else:
        rng = np.random.default_rng(n)
        cols = [random_col(rng, n, dt, 0) for dt in dtypes]
    both_layouts(monkeypatch, cols, key_idx, nparts, env={"DD_PRE_SCAN_SPAN": span},
                 expect={"n_launch": -(-n // R)})


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ranged(layout, monkeypatch):
    """create_ranged on the pre path: 512 fine partitions in 128 contiguous buckets."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DD_PRE_LAYOUT", layout)
    total, div, n = 512, 4, 3 * 4096 + 17
    cols = tier_cols("q3_p128", n)
    pid = (oracle.pids(oracle.hash_cols([cols[0]], n), total) // div).astype(np.uint32)
    ordr, poff = oracle.order(pid, total // div)
    ref = {"pid": pid, "part_offsets": poff,
           "cols": [{"data": oracle.gather_fixed(c["data"], ordr)} for c in cols]}
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], None, ranged=(total, div))
    try:
        assert part.info()["path"] == 2 and part.pre_layout() == LAYOUTS[layout]
        part.run()
        part.sync()
        compare_to_oracle(part, cols, [0], total // div, ref=ref)
    finally:
        part.destroy()
        batch.free()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("tier", ["q3_p128", "q3_p300"])
def test_rerun_and_refill(tier, layout, monkeypatch):
    """One handle: run twice, then refill the input in place with every key equal (all
    other partitions' counts must read as zero again) and with fresh keys. Offsets and
    outputs equal the oracle's — hence each other's — every time."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DD_PRE_LAYOUT", layout)
    _, key_idx, nparts, R = TIERS[tier]
    n = 3 * R + 17
    a = tier_cols(tier, n)
    b = [dict(c) for c in a]
    b[0]["data"] = np.full(n, 37, dtype=np.int64)
    c = [dict(x) for x in a]
    c[0]["data"] = np.ascontiguousarray(a[0]["data"][::-1])
    refs = [oracle.repartition(x, key_idx, nparts) for x in (a, b, c)]
    batch = api.DeviceBatch(a)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        assert part.info()["path"] == 2 and part.pre_layout() == LAYOUTS[layout]
        first = None
        for _ in range(2):
            part.run()
            part.sync()
            compare_to_oracle(part, a, key_idx, nparts, ref=refs[0])
            offs = part.row_offsets()
            assert first is None or np.array_equal(first, offs)
            first = offs
        for cols, ref in ((b, refs[1]), (c, refs[2]), (a, refs[0])):
            batch.refill(cols)
            part.run()
            part.sync()
            compare_to_oracle(part, cols, key_idx, nparts, ref=ref)
        assert np.array_equal(first, part.row_offsets())
    finally:
        part.destroy()
        batch.free()
