"""The three var-width byte engines on sliced offsets and hard length patterns (marked gpu).

A utf8 column's bytes move through one of
  v1  the direct scatter k_scatter                      (DD_V2_VAR=0, info path 0),
  K4  the slot-order gather k4_len_partials .. k4_copy  (DD_K5=0, info path 1 / k5 0),
  K5  the LDS-staged byte scatter k5_count .. k5_scatter (the default for one var column
      whose strings fit the LDS image, info k5 1).
Every case names its engines, pins each through info() before the run, and compares pids,
row offsets, lengths, bytes, validity, all P+1 partition byte offsets and (staged engines)
all n+1 rebuilt Arrow offsets with the CPU oracle.

Columns come from utf8_col: offsets may start past zero (`base`) and the buffer may be longer
than the strings (`slack`), which is what an Arrow slice or filter hands over. String bytes
are random in 33..126; the base and slack regions hold FILL, which no string contains, so a
byte leaked from them shows.

Base shape: n = 3089 rows = three K5 rounds of 1024 plus 17 ragged rows = 48 K4 groups of 64
plus a ragged one, and fewer rows than K4 has ranges (8192), so most K4 ranges are empty.
Columns [i64 key, utf8, i32]."""

import functools

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from tests.test_gpu_parity import assert_info, compare_to_oracle

pytestmark = pytest.mark.gpu

N = 3089
FILL = 0xEE
ENGINES = ["v1", "k4", "k5"]
K5_LDS_BUDGET = 163840


def utf8_col(lens, base=0, slack=0, rng=None, valid=None):
    """utf8 column dict with offsets = base + cumsum(lens) over a buffer of base + sum(lens)
    + slack bytes: random bytes in 33..126 for the strings, FILL before and after them."""
    rng = np.random.default_rng(0) if rng is None else rng
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    off = np.full(len(lens) + 1, base, dtype=np.int64)
    off[1:] += np.cumsum(lens)
    data = np.full(base + total + slack, FILL, dtype=np.uint8)
    data[base:base + total] = rng.integers(33, 127, total, dtype=np.int64).astype(np.uint8)
    return {"dtype": "utf8", "data": data, "offsets": off.astype(np.int32), "valid": valid}


def i64_col(data):
    return {"dtype": "i64", "data": np.ascontiguousarray(data, dtype=np.int64), "valid": None}


def i32_col(rng, n):
    return {"dtype": "i32", "data": rng.integers(-99, 99, n).astype(np.int32), "valid": None}


def keys_avoiding(rng, n, nparts, banned):
    """n random i64 keys none of which the oracle sends to a partition in `banned`."""
    cand = rng.integers(0, 10**12, 8 * n, dtype=np.int64)
    pid = oracle.pids(oracle.hash_cols([i64_col(cand)]), nparts)
    keep = cand[~np.isin(pid, banned)]
    assert len(keep) >= n
    return keep[:n]


def maxlen_of(col):
    return int(np.diff(col["offsets"]).max())


def pin_engine(monkeypatch, eng, maxlen):
    """Set the environment that selects engine `eng`; returns the info() fields that prove
    the partitioner took it."""
    for name in ("DD_V2_VAR", "DD_K5", "DD_K5_WPB"):
        monkeypatch.delenv(name, raising=False)
    if eng == "v1":
        monkeypatch.setenv("DD_V2_VAR", "0")
        return {"path": 0}
    if eng == "k4":
        monkeypatch.setenv("DD_K5", "0")
        return {"path": 1, "k5": 0}
    assert eng == "k5"
    return {"path": 1, "k5": 1, "k5_maxlen": maxlen}


_REFS = {}


def oracle_ref(case_id, cols, key_idx, nparts):
    """The oracle's repartition of a cached case, computed once for all engines."""
    k = (case_id, tuple(key_idx), nparts)
    if k not in _REFS:
        _REFS[k] = oracle.repartition(cols, key_idx, nparts)
    return _REFS[k]


def run_and_compare(cols, key_idx, nparts, expect, ref):
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        assert_info(part, expect)
        part.run()
        part.sync()
        compare_to_oracle(part, cols, key_idx, nparts, ref=ref)
    finally:
        part.destroy()
        batch.free()


def check_engine(monkeypatch, eng, case_id, cols, key_idx, nparts, var=1):
    expect = pin_engine(monkeypatch, eng, maxlen_of(cols[var]))
    run_and_compare(cols, key_idx, nparts, expect, oracle_ref(case_id, cols, key_idx, nparts))


# ---------------- sliced offsets ----------------

SLICES = [(0, 0), (37, 0), (0, 53), (37, 53)]


@functools.lru_cache(maxsize=None)
def sliced_cols(base, slack, keymode):
    """[i64, utf8 with 20 % nulls (null rows keep their bytes), i32]; lengths 0..17.
    keymode: "rand" random keys, "holes" keys that leave partition 0 and the last three of
    64 empty, "const" one key value."""
    rng = np.random.default_rng([base, slack, ["rand", "holes", "const"].index(keymode)])
    if keymode == "rand":
        keys = rng.integers(0, 10**12, N, dtype=np.int64)
    elif keymode == "holes":
        keys = keys_avoiding(rng, N, 64, [0, 61, 62, 63])
    else:
        keys = np.full(N, 424242, dtype=np.int64)
    valid = (rng.random(N) > 0.2).astype(np.uint8)
    u = utf8_col(rng.integers(0, 18, N), base, slack, rng=rng, valid=valid)
    assert (np.diff(u["offsets"])[valid == 0] > 0).any()
    return [i64_col(keys), u, i32_col(rng, N)]


@pytest.mark.parametrize("key_idx", [[0], [1], [1, 0]], ids=["k0", "k1", "k10"])
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("base,slack", SLICES)
def test_sliced_offsets(base, slack, eng, key_idx, monkeypatch):
    cols = sliced_cols(base, slack, "rand")
    check_engine(monkeypatch, eng, ("sliced", base, slack), cols, key_idx, 16)


@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("base,slack", SLICES)
def test_sliced_offsets_empty_edge_partitions(base, slack, eng, monkeypatch):
    cols = sliced_cols(base, slack, "holes")
    ref = oracle_ref(("holes", base, slack), cols, [0], 64)
    rows = np.diff(ref["part_offsets"])
    assert rows[0] == 0 and (rows[61:] == 0).all() and rows[1] > 0 and rows[60] > 0
    check_engine(monkeypatch, eng, ("holes", base, slack), cols, [0], 64)


@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("base,slack", SLICES)
def test_sliced_offsets_constant_key(base, slack, eng, monkeypatch):
    cols = sliced_cols(base, slack, "const")
    ref = oracle_ref(("const", base, slack), cols, [0], 16)
    assert (np.diff(ref["part_offsets"]) > 0).sum() == 1
    check_engine(monkeypatch, eng, ("const", base, slack), cols, [0], 16)


# ---------------- full image ----------------

@functools.lru_cache(maxsize=None)
def full_image_cols(constant_key):
    rng = np.random.default_rng(128 + constant_key)
    keys = (np.full(N, 7, dtype=np.int64) if constant_key
            else rng.integers(0, 10**12, N, dtype=np.int64))
    return [i64_col(keys), utf8_col(np.full(N, 128), rng=rng), i32_col(rng, N)]


@pytest.mark.parametrize("eng", ["k4", "k5"])
@pytest.mark.parametrize("constant_key", [1, 0], ids=["const", "rand"])
def test_full_image(constant_key, eng, monkeypatch):
    """Every string 128 B. With one key a K5 round's image is all one partition: 1024 x 128
    = 131072 B, and 64 x 128 = 8192 B in one u16 segment count."""
    cols = full_image_cols(constant_key)
    check_engine(monkeypatch, eng, ("full", constant_key), cols, [0], 16)


# ---------------- alignment sweep ----------------

@functools.lru_cache(maxsize=None)
def sweep_cols(pattern):
    rng = np.random.default_rng(1700 + pattern)
    i = np.arange(N)
    lens = i % 17 if pattern == 0 else (7 * i) % 13
    return [i64_col(rng.integers(0, 10**12, N, dtype=np.int64)), utf8_col(lens, rng=rng),
            i32_col(rng, N)]


@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("nparts", [3, 16])
@pytest.mark.parametrize("pattern", [0, 1], ids=["i%17", "7i%13"])
def test_alignment_sweep(pattern, nparts, eng, monkeypatch):
    """Lengths cycle through every residue while the running image position cycles through
    every alignment: each (destination alignment, len % 8) pair of the LDS byte copy and of
    the flush occurs."""
    check_engine(monkeypatch, eng, ("sweep", pattern), sweep_cols(pattern), [0], nparts)


# ---------------- sparse ----------------

@functools.lru_cache(maxsize=None)
def sparse_cols(m):
    rng = np.random.default_rng(9700 + m)
    lens = np.zeros(N, dtype=np.int64)
    lens[::97] = m
    lens[0] = lens[N - 1] = m
    return [i64_col(rng.integers(0, 10**12, N, dtype=np.int64)), utf8_col(lens, rng=rng),
            i32_col(rng, N)]


SPARSE_SHORT = [1, 7, 8, 9, 128]
SPARSE_LONG = [129, 511, 512, 513, 5000]


@pytest.mark.parametrize("eng,m", [("k5", m) for m in SPARSE_SHORT] +
                         [(e, m) for e in ("k4", "v1") for m in SPARSE_SHORT + SPARSE_LONG])
def test_sparse_strings(eng, m, monkeypatch):
    """Empty strings except rows 0, n-1 and every 97th: runs of 96 empties hold whole empty
    waves (a K4 group with no bytes, the skip over empty strings inside a chunk), and the
    long lengths span several 512 B wave strides of the K4 copy."""
    check_engine(monkeypatch, eng, ("sparse", m), sparse_cols(m), [0], 16)


# ---------------- tiny runs ----------------

@functools.lru_cache(maxsize=None)
def tiny_cols():
    rng = np.random.default_rng(777)
    lens = rng.integers(0, 4, N)
    return [i64_col(rng.integers(0, 10**12, N, dtype=np.int64)), utf8_col(lens, rng=rng),
            i32_col(rng, N)]


@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("nparts", [777, 2048])
def test_tiny_runs(nparts, eng, monkeypatch):
    """Lengths 0..3 at a partition count near a round's 1024 rows: per-partition runs in a
    K5 image are shorter than 8 B, so only the flush's tail loop writes them."""
    cols = tiny_cols()
    assert maxlen_of(cols[1]) == 3
    check_engine(monkeypatch, eng, "tiny", cols, [0], nparts)


# ---------------- K5's LDS gate ----------------

def k5_lds_bytes(nparts, maxlen, wpb=16):
    """LDS of k5_scatter: per-wave base tables, the round's offsets, the byte image."""
    return wpb * nparts * 4 + (nparts + 1) * 4 + 64 * wpb * maxlen + 8


def k5_gate_maxlen(nparts):
    return max(m for m in range(1, 129) if k5_lds_bytes(nparts, m) <= K5_LDS_BUDGET)


@functools.lru_cache(maxsize=None)
def gate_cols(maxlen):
    rng = np.random.default_rng(4000 + maxlen)
    lens = rng.integers(0, 6, N)
    lens[int(rng.integers(0, N))] = maxlen  # the one string that decides the gate
    return [i64_col(rng.integers(0, 10**12, N, dtype=np.int64)), utf8_col(lens, rng=rng)]


@pytest.mark.parametrize("past", [0, 1], ids=["fits", "over"])
@pytest.mark.parametrize("nparts", [2048, 1024])
def test_k5_lds_gate(nparts, past, monkeypatch):
    """K5 is taken up to the longest string whose image still fits beside P-sized tables,
    and the K4 gather from the next length on; both sides match the oracle. The budget is
    all of a block's LDS: any static __shared__ in k5_scatter makes the "fits" side fail
    to launch (invalid argument), as it did while the kernel kept 8 KB of length tables."""
    assert k5_gate_maxlen(2048) == 23 and k5_gate_maxlen(1024) == 91
    maxlen = k5_gate_maxlen(nparts) + past
    cols = gate_cols(maxlen)
    assert maxlen_of(cols[1]) == maxlen
    expect = pin_engine(monkeypatch, "k5", maxlen)
    if past:
        expect = {"path": 1, "k5": 0}
    run_and_compare(cols, [0], nparts, expect,
                    oracle_ref(("gate", maxlen), cols, [0], nparts))


# ---------------- more than one wave step per K4 range ----------------

N_BIG = 2 * 64 * 8192 + 77


@functools.lru_cache(maxsize=None)
def big_cols():
    rng = np.random.default_rng(1048653)
    lens = rng.integers(0, 4, N_BIG)
    return [i64_col(rng.integers(0, 10**12, N_BIG, dtype=np.int64)),
            utf8_col(lens, rng=rng), i32_col(rng, N_BIG)]


@pytest.mark.parametrize("eng", ["k4", "k5"])
def test_two_wave_steps_per_k4_range(eng, monkeypatch):
    """n = 1 048 653: every one of K4's 8192 ranges holds at least 128 slots, so the strided
    sum of k4_len_partials and the carry across 64-slot steps of k4_off_rewrite both run;
    K5's scan walks about eight segments per range."""
    check_engine(monkeypatch, eng, "big", big_cols(), [0], 64)


# ---------------- consumers of the offsets ----------------

@functools.lru_cache(maxsize=None)
def arrow_sliced():
    """A pyarrow string array of N rows cut out of a longer one with .slice: 37 bytes of
    other rows before its strings and 53 after. Returns (array, column dicts)."""
    import pyarrow as pa

    rng = np.random.default_rng(3753)

    def text(length):
        return bytes(rng.integers(33, 127, length, dtype=np.int64).astype(np.uint8)).decode()

    head = [text(10), text(0), text(27)]
    tail = [text(50), text(3)]
    body = [None if rng.random() < 0.1 else text(int(l)) for l in rng.integers(0, 18, N)]
    arr = pa.array(head + body + tail, type=pa.string()).slice(len(head), N)
    _, obuf, dbuf = arr.buffers()
    off = np.frombuffer(obuf, dtype=np.int32)[arr.offset:arr.offset + N + 1].copy()
    data = np.frombuffer(dbuf, dtype=np.uint8).copy()
    assert off[0] == 37 and len(data) - off[-1] == 53
    valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=np.uint8)
    cols = [i64_col(rng.integers(0, 10**12, N, dtype=np.int64)),
            {"dtype": "utf8", "data": data, "offsets": off, "valid": valid},
            i32_col(rng, N)]
    return arr, cols


@pytest.mark.parametrize("eng", ["k5", "k4"])
def test_partition_batches_of_sliced_arrow_column(eng, monkeypatch):
    import pyarrow as pa

    from datafusion_distributed_amd import arrow_boundary

    arr, cols = arrow_sliced()
    nparts = 16
    ref = oracle_ref("arrow", cols, [0], nparts)
    direct = pa.table({"c0": cols[0]["data"], "c1": arr, "c2": cols[2]["data"]})
    expect = pin_engine(monkeypatch, eng, maxlen_of(cols[1]))
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], nparts)
    try:
        assert_info(part, expect)
        part.run()
        part.sync()
        emitted = {p: [] for p in range(nparts)}
        for p, rb in arrow_boundary.partition_batches(part, 0, nparts, batch_size=100):
            emitted[p].append(rb)
        for p in range(nparts):
            lo, hi = ref["part_offsets"][p], ref["part_offsets"][p + 1]
            want = direct.take(pa.array(ref["order"][lo:hi], type=pa.int64()))
            got = pa.Table.from_batches(emitted[p])
            assert got.num_rows == hi - lo
            assert got.equals(want), f"partition {p} differs from pyarrow's take"
    finally:
        part.destroy()
        batch.free()


@pytest.mark.parametrize("eng", ["k5", "k4"])
def test_self_exchange_of_sliced_column(eng, monkeypatch):
    cols = sliced_cols(37, 53, "rand")
    nparts = 16
    ref = oracle_ref(("sliced", 37, 53), cols, [0], nparts)
    expect = pin_engine(monkeypatch, eng, maxlen_of(cols[1]))
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], nparts)
    comm = ex = None
    try:
        assert_info(part, expect)
        part.run()
        part.sync()
        comm = api.Comm(api.Comm.unique_id(), 0, 1)
        ex = comm.exchange(part)
        assert ex.total_rows == N
        poff = ref["part_offsets"]
        assert (ex.row_counts()[0] == np.diff(poff)).all()
        exp = ref["cols"][1]
        pref = np.zeros(N + 1, dtype=np.int64)
        pref[1:] = np.cumsum(exp["lengths"].astype(np.int64))
        bc = ex.byte_counts(1)
        assert (bc[0] == np.diff(pref[poff])).all(), f"byte counts differ: {bc[0]}"
        got = ex.col_data(1)
        assert (got["lengths"] == exp["lengths"]).all()
        assert got["data"].tobytes() == exp["data"].tobytes()
        assert (ex.col_validity(1) == exp["valid"]).all()
        assert (ex.col_data(0)["data"] == ref["cols"][0]["data"]).all()
        assert (ex.col_data(2)["data"] == ref["cols"][2]["data"]).all()
    finally:
        if ex is not None:
            ex.destroy()
        if comm is not None:
            comm.destroy()
        part.destroy()
        batch.free()
