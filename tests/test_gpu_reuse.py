"""Partitioner reuse (marked gpu): one handle, many runs — the way bench.py and a worker
use it. Every scatter tier dd_partitioner_create can pick is pinned through
Partitioner.info() and then re-run, refilled in place with other data of the same shape
(reuse contract: include/dd_shuffle.h above dd_partitioner_run), run back to back without
a host sync, phase-split across two streams, and fed from a copy stream — each result
bit-exact against the CPU oracle of the data that run carried. The tuning knobs the README
lists (DD_PID8, DD_PRE_*, DD_K5_WPB, DD_K4_BLOCKS, DD_V2_BLOCKS) are covered the same way.

Three datasets of one shape per tier: A uniform keys, B one key value for every row (all
rows in one partition: every other partition's slots must read as empty again), C
Zipf(1.1) keys. The oracle's offsets, not the device's, prove that B empties at least P-1
partitions and that A fills all of them, so a workspace slot written in one run and not in
the next is actually exercised."""

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from tests.test_gpu_fuzz import random_col
from tests.test_gpu_parity import assert_info, compare_to_oracle

pytestmark = pytest.mark.gpu

Q3 = [("i64",), ("f64",), ("f64",), ("i32",)]
TWO_VAR = [("i64",), ("utf8", 0, 48, 0.15, 0), ("utf8", 0, 8, 0, 0), ("f64",)]

# id -> (column specs, key columns, P, env, expected info(), row-count rule)
# column spec: (dtype,) | (dtype, null fraction) | ("utf8", minlen, maxlen, null fraction,
# one extra-long string's length or 0) | ("dict32",)
TIERS = {
    "pre128": (Q3, [0], 128, {},
               {"path": 2, "gmax": 4, "wpb": 16, "pid_elem": 1}, "pre"),
    "pre256": (Q3, [3, 0], 256, {}, {"path": 2, "gmax": 4, "pid_elem": 1}, "pre"),
    "pre512": (Q3, [0], 300, {}, {"path": 2, "gmax": 2, "pid_elem": 4}, "pre"),
    "pre_q1": ([("u8",), ("bool",), ("f64",), ("f64",), ("f64",), ("f64",), ("i32",)],
               [0, 1], 7, {}, {"path": 2, "gmax": 2}, "pre"),
    "hl": (Q3, [0], 100, {"DD_K3_PRE": "0"},
           {"path": 1, "hl": 1, "gmax": 4, "wpb": 16}, 70_001),
    "hlg": (Q3 + [("i32",)], [0, 4], 128, {"DD_K3_PRE": "0"},
            {"path": 1, "hl": 2}, 70_001),
    "spec": (Q3, [0], 128, {"DD_K3_PRE": "0", "DD_K3_HL": "0"},
             {"path": 1, "hl": 0, "wpb": 16}, 70_001),
    "rhash": (Q3, [0], 128, {"DD_RHASH": "1"}, {"rhash": 1, "path": 1}, 70_001),
    "staged_valid": ([("i64", 0.10), ("f64",), ("bool", 0.30)], [0, 2], 32, {},
                     {"path": 1, "hl": 0}, 70_001),
    "staged_p2048": ([("i64",)], [0], 2048, {},
                     {"path": 1, "wpb": lambda w: 0 < w < 16}, 70_001),
    "k5": ([("i64",), ("utf8", 0, 17, 0, 0), ("i32",)], [0], 16, {},
           {"path": 1, "k5": 1, "k5_maxlen": 17}, 5 * 1024 + 3),
    "k4": ([("i64",), ("utf8", 0, 300, 0, 5000)], [0], 64, {},
           {"path": 1, "k5": 0}, 70_001),
    "k4_2var": (TWO_VAR, [0], 64, {}, {"path": 1, "k5": 0}, 70_001),
    "v1_var": (TWO_VAR, [0], 64, {"DD_V2_VAR": "0"}, {"path": 0}, 20_001),
    "v1_wide": ([("i64",), ("f64",), ("i32",), ("i16",), ("u8",), ("f32",), ("bool",),
                 ("f64",), ("i32",)], [0, 8], 100, {}, {"path": 0}, 20_001),
    # dict32 + i64 is no pre/HL shape: the plain staged scatter with the key hash
    # gathered from the create-time dictionary hashes
    "dictkey": ([("dict32",), ("i64",)], [0], 16, {},
                {"path": 1, "hl": 0, "wpb": 16, "k5": 0}, 70_001),
}
PIPELINED = ["pre128", "staged_valid", "k5", "k4"]

NPDT = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32,
        "i64": np.int64, "f32": np.float32, "f64": np.float64}


def set_env(monkeypatch, env):
    for name in ("DD_K3_PRE", "DD_K3_HL", "DD_RHASH", "DD_V2_VAR", "DD_K5", "DD_PID8",
                 "DD_PRE_RPB", "DD_PRE_GMAX", "DD_PRE_WPB", "DD_K5_WPB", "DD_K4_BLOCKS",
                 "DD_V2_BLOCKS", "DD_V2_WPB", "DD_V2_GMAX"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def make_dictionary(rng, nparts):
    """50 dictionary values whose hashes reach every one of `nparts` partitions (placed
    with the oracle), with one value stored under three indices and two empty values."""
    cand = [bytes(rng.integers(0, 256, rng.integers(1, 13), dtype=np.int64)
                  .astype(np.uint8)) for _ in range(400)]
    coff = np.zeros(len(cand) + 1, dtype=np.int32)
    coff[1:] = np.cumsum([len(v) for v in cand])
    probe = {"dtype": "dict32", "data": np.arange(len(cand), dtype=np.int32),
             "dict_bytes": np.frombuffer(b"".join(cand), dtype=np.uint8).copy(),
             "dict_offsets": coff, "valid": None}
    pid = oracle.pids(oracle.hash_cols([probe]), nparts)
    vals = [cand[int(np.flatnonzero(pid == p)[0])] for p in range(nparts)]
    vals += [c for c in cand if c not in vals][:46 - nparts]
    vals += [vals[3], vals[3], b"", b""]
    assert len(vals) == 50
    doff = np.zeros(51, dtype=np.int32)
    doff[1:] = np.cumsum([len(v) for v in vals])
    return np.frombuffer(b"".join(vals), dtype=np.uint8).copy(), doff


def key_values(rng, n, dtype, which, hi):
    """Key data of dataset `which`; `hi` bounds the value range (dictionary size)."""
    if which == "A":
        if hi is not None:
            return rng.integers(0, hi, n).astype(np.int32)
        return random_col(rng, n, dtype, 0)["data"]
    if which == "B":
        v = np.full(n, 1 if dtype == "bool" else 37)
    else:
        v = rng.zipf(1.1, n) % 1000
    if hi is not None:
        v = v % hi
    elif dtype == "bool":
        v = v % 2
    return v.astype(np.int32 if hi is not None else NPDT[dtype])


def permuted_strings(rng, base, fresh_bytes):
    """A utf8 column with the strings of `base` in another row order (same byte total,
    same longest string); fresh_bytes keeps only the lengths and draws new bytes."""
    n = len(base["offsets"]) - 1
    perm = rng.permutation(n)
    off0 = np.asarray(base["offsets"], dtype=np.int64)
    lens = np.diff(off0)[perm]
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    if fresh_bytes:
        data = rng.integers(0, 256, int(off[-1]), dtype=np.int64).astype(np.uint8)
    else:
        src = np.repeat(off0[:-1][perm] - off[:-1], lens) + np.arange(int(off[-1]))
        data = np.asarray(base["data"])[src]
    return data, off.astype(np.int32)


def make_dataset(rng, specs, key_idx, n, which, base, dictionary):
    cols = []
    for i, spec in enumerate(specs):
        dtype = spec[0]
        is_key = i in key_idx
        null_p = spec[3] if dtype == "utf8" else (spec[1] if len(spec) > 1 else 0)
        valid = None
        if null_p:
            valid = (np.ones(n, dtype=np.uint8) if is_key and which == "B"
                     else (rng.random(n) >= null_p).astype(np.uint8))
        if dtype == "utf8":
            assert not is_key
            if base is None:
                lens = rng.integers(spec[1], spec[2] + 1, n)
                lens[n // 2] = spec[2]  # the nominal maximum is present
                if spec[4]:
                    lens[n // 3] = spec[4]
                off = np.zeros(n + 1, dtype=np.int32)
                off[1:] = np.cumsum(lens)
                data = rng.integers(0, 256, int(off[-1]), dtype=np.int64).astype(np.uint8)
            else:
                data, off = permuted_strings(rng, base[i], fresh_bytes=(which == "C"))
            cols.append({"dtype": "utf8", "data": data, "offsets": off, "valid": valid})
        elif dtype == "dict32":
            dbytes, doff = dictionary
            idx = (key_values(rng, n, dtype, which, 50) if is_key
                   else rng.integers(0, 50, n).astype(np.int32))
            cols.append({"dtype": "dict32", "data": idx, "dict_bytes": dbytes,
                         "dict_offsets": doff, "valid": valid})
        elif is_key:
            cols.append({"dtype": dtype, "data": key_values(rng, n, dtype, which, None),
                         "valid": valid})
        else:
            col = random_col(rng, n, dtype, 0)
            col["valid"] = valid
            cols.append(col)
    return cols


def probe_round_rows(specs, key_idx, nparts):
    """round_rows of the tier, read from a one-row batch of the same dtypes (the block
    shape does not depend on the row count)."""
    cols = [{"dtype": s[0], "data": np.zeros(1, dtype=NPDT[s[0]]), "valid": None}
            for s in specs]
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        return part.info()["round_rows"]
    finally:
        part.destroy()
        batch.free()


_CASES = {}


def tier_case(tier, monkeypatch):
    """Set the tier's environment and return its (cached) datasets A/B/C with their
    oracle results. Checks on the CPU that B empties >= P-1 partitions and A none."""
    specs, key_idx, nparts, env, expect, rows = TIERS[tier]
    set_env(monkeypatch, env)
    if tier in _CASES:
        return _CASES[tier]
    if rows == "pre":
        # three full rounds + a ragged one: with rpb = 2, two blocks, the second ending
        # on the ragged round
        rows = 3 * probe_round_rows(specs, key_idx, nparts) + 17
    rng = np.random.default_rng(sum(map(ord, tier)))
    dictionary = (make_dictionary(rng, nparts)
                  if any(s[0] == "dict32" for s in specs) else None)
    data, refs = {}, {}
    for which in "ABC":
        data[which] = make_dataset(rng, specs, key_idx, rows, which, data.get("A"),
                                   dictionary)
        refs[which] = oracle.repartition(data[which], key_idx, nparts)
    filled = {w: int((np.diff(refs[w]["part_offsets"]) > 0).sum()) for w in "ABC"}
    if nparts > 1:
        assert filled["B"] == 1, f"{tier}: dataset B fills {filled['B']} partitions"
    if rows >= 64 * nparts:
        assert filled["A"] == nparts, f"{tier}: dataset A leaves a partition empty"
    for i, spec in enumerate(specs):  # every refill stays inside the reuse contract
        if spec[0] == "utf8":
            for which in "BC":
                assert data[which][i]["offsets"][-1] == data["A"][i]["offsets"][-1]
                assert (np.diff(data[which][i]["offsets"]).max()
                        == np.diff(data["A"][i]["offsets"]).max())
    _CASES[tier] = {"key_idx": key_idx, "nparts": nparts, "expect": expect, "rows": rows,
                    "data": data, "refs": refs}
    return _CASES[tier]


class Handle:
    """One device batch + one partitioner, created on dataset `which`."""

    def __init__(self, case, which="A"):
        self.case = case
        self.batch = api.DeviceBatch(case["data"][which])
        try:
            self.part = api.Partitioner(self.batch, case["key_idx"], case["nparts"])
        except Exception:
            self.batch.free()
            raise

    def check_tier(self, expect=None):
        info = assert_info(self.part, self.case["expect"] if expect is None else expect)
        assert info["pid_elem"] == api.lib().dd_partitioner_pid_elem(self.part.h)
        if info["rhash"]:
            assert self.part.pids() is None
        else:
            assert self.part.has_pid_array()
        return info

    def compare(self, which):
        case = self.case
        compare_to_oracle(self.part, case["data"][which], case["key_idx"], case["nparts"],
                          ref=case["refs"][which])

    def close(self):
        self.part.destroy()
        self.batch.free()


@pytest.fixture
def handle_factory():
    made = []

    def make(case, which="A"):
        h = Handle(case, which)
        made.append(h)
        return h

    yield make
    api.lib().dd_device_sync()
    for h in made:
        h.close()


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_tier_and_rerun(tier, monkeypatch, handle_factory):
    """The tier's gate picks the kernel the table names, and three synced runs of one
    handle over unchanged input give the oracle's result every time."""
    case = tier_case(tier, monkeypatch)
    h = handle_factory(case)
    info = h.check_tier()
    if info["path"] == 2:
        assert case["rows"] == 3 * info["round_rows"] + 17 and info["n_launch"] == 4
        assert info["rpb"] == 2
    elif info["path"] == 1 and tier != "k5":
        # more than one round per tile
        assert case["rows"] > info["n_launch"] * info["round_rows"]
    for _ in range(3):
        h.part.run()
        h.part.sync()
        h.compare("A")


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_refill(tier, monkeypatch, handle_factory):
    """A -> B -> C -> A through DeviceBatch.refill on one handle: a workspace slot written
    only in A's run (B leaves all partitions but one empty) or only in B's must not leak
    into the next result."""
    case = tier_case(tier, monkeypatch)
    h = handle_factory(case)
    h.check_tier()
    h.part.run()
    h.part.sync()
    h.compare("A")
    for which in "BCA":
        h.batch.refill(case["data"][which])
        h.part.run()
        h.part.sync()
        h.compare(which)


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_back_to_back_no_sync(tier, monkeypatch, handle_factory):
    """Two runs queued on one stream with no host sync between them."""
    case = tier_case(tier, monkeypatch)
    h = handle_factory(case)
    h.check_tier()
    h.part.run()
    h.part.run()
    h.part.sync()
    h.compare("A")


def phase_split(case, make):
    """bench.py's pipelined_steps schedule, five passes: phase 1 of one partitioner on
    stream 1 overlapped with phase 2 of the other on stream 2, ordered only by
    wait_phase1 / wait_phase2. Both end bit-exact on their own (different) data."""
    import torch

    parts2 = [make(case, "A"), make(case, "C")]
    for h in parts2:
        h.check_tier()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    k = 5
    for i in range(k):
        cur = parts2[i % 2].part
        cur.wait_phase2(s1)
        cur.run_phase1(s1)
        if i > 0:
            prv = parts2[(i + 1) % 2].part
            prv.wait_phase1(s2)
            prv.run_phase2(s2)
    last = parts2[(k - 1) % 2].part
    last.wait_phase1(s2)
    last.run_phase2(s2)
    torch.cuda.synchronize()
    parts2[0].compare("A")
    parts2[1].compare("C")


def pinned(cols, keep):
    """The same columns with every array in pinned host memory (tensors kept in `keep`)."""
    import torch

    out = []
    for col in cols:
        col = dict(col)
        for name in ("data", "offsets", "valid"):
            if col.get(name) is not None and len(col[name]):
                t = torch.from_numpy(np.ascontiguousarray(col[name])).pin_memory()
                keep.append(t)
                col[name] = t.numpy()
        out.append(col)
    return out


def staged_ingest(case, make):
    """bench.py's ingest leg with changing data, six passes: pass i refills buffer i % 2
    with dataset [A, B, C][i % 3] on the copy stream once wait_phase2 says the buffer is
    free, and the compute stream runs after the copy's event. The last two passes'
    outputs match the oracle of the datasets they carried."""
    import torch

    keep = []
    host = {w: pinned(case["data"][w], keep) for w in "ABC"}
    bufs = [make(case, "A"), make(case, "A")]
    for h in bufs:
        h.check_tier()
    copy_s, comp_s = torch.cuda.Stream(), torch.cuda.Stream()
    evs = [torch.cuda.Event() for _ in range(2)]
    carried = [None, None]
    for i in range(6):
        b, which = i % 2, "ABC"[i % 3]
        with torch.cuda.stream(copy_s):
            bufs[b].part.wait_phase2(copy_s)
            bufs[b].batch.refill(host[which], stream=copy_s)
            evs[b].record(copy_s)
        comp_s.wait_event(evs[b])
        bufs[b].part.run(stream=comp_s)
        carried[b] = which
    torch.cuda.synchronize()
    assert carried == ["B", "C"]
    for b in range(2):
        bufs[b].compare(carried[b])


PIPELINE_SCENARIOS = {"phase_split": phase_split, "staged_ingest": staged_ingest}


def pipelined_child():
    """Body of the child process behind the pipelined tests: every scenario x tier, one
    JSON line {"scenario/tier": "ok" | failure text} on stdout. torch brings its own HIP
    runtime, which has to be the first one the process loads, so this cannot run inside
    the pytest process (its collection has already loaded libdd_shuffle.so). A device
    error ends the child at once; scenarios after it are reported as not run."""
    import json
    import traceback

    import torch

    torch.cuda.set_device(0)
    torch.cuda.synchronize()
    results = {}
    for name, scenario in PIPELINE_SCENARIOS.items():
        for tier in PIPELINED:
            results[f"{name}/{tier}"] = "not run: an earlier scenario hit a device error"
    for name, scenario in PIPELINE_SCENARIOS.items():
        for tier in PIPELINED:
            made = []

            def make(case, which):
                made.append(Handle(case, which))
                return made[-1]

            mp = pytest.MonkeyPatch()
            try:
                scenario(tier_case(tier, mp), make)
                results[f"{name}/{tier}"] = "ok"
            except AssertionError:
                results[f"{name}/{tier}"] = traceback.format_exc()
            except Exception:
                results[f"{name}/{tier}"] = traceback.format_exc()
                print(json.dumps(results))
                return
            finally:
                mp.undo()
            torch.cuda.synchronize()
            for h in made:
                h.close()
    print(json.dumps(results))


@pytest.fixture(scope="module")
def pipelined_results():
    import json
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          ["-c", "import tests.test_gpu_reuse as t; t.pipelined_child()"]
    env = dict(os.environ, PYTHONPATH=repo)
    out = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True,
                         timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and lines, \
        f"pipelined child failed (exit {out.returncode}):\n{out.stdout}\n{out.stderr}"
    return json.loads(lines[-1])


@pytest.mark.parametrize("tier", PIPELINED)
@pytest.mark.parametrize("scenario", sorted(PIPELINE_SCENARIOS))
def test_pipelined(scenario, tier, pipelined_results):
    """phase_split and staged_ingest (see their docstrings) on torch streams, the way
    bench.py drives them; run in one child process for all cases."""
    assert pipelined_results[f"{scenario}/{tier}"] == "ok", \
        pipelined_results[f"{scenario}/{tier}"]


KNOBS = [  # (tier, knob environment, info() the knob must produce)
    ("pre128", {"DD_PID8": "0"}, {"path": 2, "pid_elem": 4}),
    ("pre128", {"DD_PRE_RPB": "1"}, {"path": 2, "rpb": 1}),
    ("pre128", {"DD_PRE_RPB": "4"}, {"path": 2, "rpb": 4}),
    # more rounds per block than rounds: one block walks every round
    ("pre128", {"DD_PRE_RPB": "256"}, {"path": 2, "rpb": 256, "n_launch": 4}),
    ("pre128", {"DD_PRE_GMAX": "2"}, {"path": 2, "gmax": 2, "round_rows": 2048}),
    ("pre128", {"DD_PRE_WPB": "8"}, {"path": 2, "wpb": 8, "round_rows": 2048}),
    ("k5", {"DD_K5_WPB": "8"}, {"k5": 1, "k5_wpb": 8}),
    # the K4 grid cap is read at launch and is no plan field: the row pins that the K4
    # gather (not K5) copies the bytes, 256 blocks striding over 70 001 rows
    ("k4", {"DD_K4_BLOCKS": "256"}, {"path": 1, "k5": 0}),
    ("staged_valid", {"DD_V2_BLOCKS": "8"}, {"path": 1, "n_launch": 8}),
    ("staged_valid", {"DD_V2_BLOCKS": "64"}, {"path": 1, "n_launch": 64}),
]


@pytest.mark.parametrize("tier,knob,expect", KNOBS,
                         ids=[f"{t}-{'-'.join(f'{k}={v}' for k, v in e.items())}"
                              for t, e, _ in KNOBS])
def test_tuning_knobs(tier, knob, expect, monkeypatch, handle_factory):
    """Every README tuning knob takes effect (seen through info()) and changes
    scheduling only: two runs of the knobbed plan are bit-exact against the oracle."""
    case = tier_case(tier, monkeypatch)
    for name, value in knob.items():
        monkeypatch.setenv(name, value)
    h = handle_factory(case)
    h.check_tier({**case["expect"], **expect})
    for _ in range(2):
        h.part.run()
        h.part.sync()
        h.compare("A")
