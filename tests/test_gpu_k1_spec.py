"""K1 key signatures (marked gpu): the tile / seg / round hash-count kernels instantiated
for a compile-time key signature (Partitioner.k1_spec() != 0) against the CPU oracle, and
against the generic run-time key loop (DD_K1_SPEC=0) on the same input.

The three K1 kernels are selected by the default (k_hash_count_round), DD_PRE_LAYOUT=seg
(k_hash_count_seg) and DD_K3_PRE=0 (k_hash_count_tile). A batch shape outside the pre
path's whitelist runs the tile kernel whatever the knobs say: such a case asserts that
(info()["path"] == 1) and stops, since the tile case of the same shape covers it. Every
comparison is bit-exact; oracle results are computed once per input and shared."""

import numpy as np
import pytest

import oracle
from datafusion_distributed_amd import api
from tests.test_gpu_fuzz import random_col
from tests.test_gpu_parity import check_against_oracle, compare_to_oracle

pytestmark = pytest.mark.gpu

KNOBS = ("DD_K1_SPEC", "DD_PRE_LAYOUT", "DD_PRE_XCD", "DD_PRE_RPB", "DD_PID8", "DD_PRE_WPB",
         "DD_PRE_GMAX", "DD_PRE_SCAN_SPAN", "DD_K3_PRE", "DD_K3_HL", "DD_RHASH",
         "DD_V2_WPB", "DD_V2_GMAX", "DD_V2_BLOCKS")
# kernel -> (environment, pre_layout() it reports when the shape is on the pre path)
KERNELS = {"round": ({}, 2), "seg": ({"DD_PRE_LAYOUT": "seg"}, 1),
           "tile": ({"DD_K3_PRE": "0"}, 0)}

Q3 = ["f64", "f64", "i32"]
Q1 = ["u8", "bool", "f64", "f64", "f64", "f64", "i32"]
# signature -> (dtypes, key columns, k1_spec() code, pre(P): is the shape on the pre path)
SIGS = {
    "u8": (Q1, [0], 0x1, lambda P: P <= 128),
    "bool": (Q1, [1], 0x1, lambda P: P <= 128),
    "i16": (["i16"] + Q3, [0], 0x2, lambda P: False),
    "i32": (["i32"] + Q3, [0], 0x3, lambda P: P <= 128),
    "i64": (["i64"] + Q3, [0], 0x4, lambda P: P <= 512),
    "f32": (["f32"] + Q3, [0], 0x5, lambda P: P <= 128),
    "f64": (["f64"] + Q3, [0], 0x6, lambda P: P <= 512),
    "dict32": (["dict32"] + Q3, [0], 0x7, lambda P: P <= 128),
    "i64+i32": (["i64"] + Q3 + ["i32"], [0, 4], 0x34, lambda P: P <= 128 or 256 < P <= 512),
    "u8+bool": (Q1, [0, 1], 0x11, lambda P: P <= 128),
}
PARTS = [1, 7, 128, 257, 512]
NMAX = 3 * 4096 + 17


def row_counts(R):
    return [1, 3, 4, 5, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 17]


def head(cols, n):
    """The first n rows of a batch (dictionaries stay whole)."""
    return [{**c, "data": c["data"][:n]} for c in cols]


_DATA = {}


def sig_cols(sig, n):
    if sig not in _DATA:
        rng = np.random.default_rng(sum(map(ord, sig)))
        _DATA[sig] = [random_col(rng, NMAX, dt, 0) for dt in SIGS[sig][0]]
    return head(_DATA[sig], n)


_REFS = {}
_repartition = oracle.repartition


def reference(tag, cols, key_idx, nparts):
    """oracle.repartition, once per (tag, keys, P) — tag names the input."""
    key = (tag, tuple(key_idx), nparts)
    if key not in _REFS:
        _REFS[key] = _repartition(cols, key_idx, nparts)
    return _REFS[key]


def set_env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def oracle_check(monkeypatch, tag, cols, key_idx, nparts, env, expect=None, spec=None):
    """check_against_oracle under `env`, the oracle result shared through reference();
    returns (info(), pre_layout(), k1_spec()) of the partitioner it created, and asserts
    k1_spec() == spec when given."""
    set_env(monkeypatch, env)
    seen = []

    class Checked(api.Partitioner):
        def run(self, stream=None):
            seen.append((self.info(), self.pre_layout(), self.k1_spec()))
            super().run(stream)

    with monkeypatch.context() as m:
        m.setattr(api, "Partitioner", Checked)
        m.setattr(oracle, "repartition", lambda *args: reference(tag, *args))
        check_against_oracle(cols, key_idx, nparts, expect=expect)
    assert len(seen) == 1
    if spec is not None:
        assert seen[0][2] == spec, f"k1_spec() = {seen[0][2]:#x}, expected {spec:#x}"
    return seen[0]


def took_kernel(plan, kernel, on_pre):
    """Assert the K1 kernel a plan runs; False when the shape is not eligible for the
    kernel the case names (it then runs the tile kernel)."""
    info, layout, _ = plan
    if kernel == "tile" or not on_pre:
        assert info["path"] == 1 and layout == 0, f"expected the tile K1: {info}"
        return kernel == "tile"
    assert info["path"] == 2 and layout == KERNELS[kernel][1], \
        f"expected the {kernel} K1: {info}, pre_layout {layout}"
    return True


@pytest.mark.parametrize("nparts", PARTS)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("sig", sorted(SIGS))
def test_signature_edges(sig, kernel, nparts, monkeypatch):
    """Every instantiated signature x K1 kernel x P, on the round and row-group edges."""
    _, key_idx, code, pre = SIGS[sig]
    env = KERNELS[kernel][0]
    plan = oracle_check(monkeypatch, (sig, 1), sig_cols(sig, 1), key_idx, nparts, env,
                        spec=code)
    if not took_kernel(plan, kernel, pre(nparts)):
        return  # not eligible for this kernel: the tile case covers the shape
    R = plan[0]["round_rows"]
    assert R in (1024, 2048, 4096)
    if nparts > 256:
        assert plan[0]["pid_elem"] == 4
    for n in row_counts(R)[1:]:
        again = oracle_check(monkeypatch, (sig, n), sig_cols(sig, n), key_idx, nparts, env,
                             spec=code)
        assert took_kernel(again, kernel, pre(nparts))


def outputs(cols, key_idx, nparts):
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, key_idx, nparts)
    try:
        spec = part.k1_spec()
        part.run()
        part.sync()
        outs = [part.col_out(i)["data"].copy().view(np.uint8) for i in range(len(cols))]
        return spec, part.row_offsets().copy(), outs
    finally:
        part.destroy()
        batch.free()


@pytest.mark.parametrize("nparts", [7, 128])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("sig", sorted(SIGS))
def test_spec_equals_generic(sig, kernel, nparts, monkeypatch):
    """DD_K1_SPEC=0 and the default give the same offsets and output bytes."""
    _, key_idx, code, _ = SIGS[sig]
    cols = sig_cols(sig, NMAX)
    set_env(monkeypatch, {**KERNELS[kernel][0], "DD_K1_SPEC": "0"})
    spec0, off0, out0 = outputs(cols, key_idx, nparts)
    set_env(monkeypatch, KERNELS[kernel][0])
    spec1, off1, out1 = outputs(cols, key_idx, nparts)
    assert spec0 == 0 and spec1 == code
    assert np.array_equal(off0, off1)
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)


def nullable_key(n):
    cols = sig_cols("i64", n)
    cols[0] = {**cols[0], "valid": (np.arange(n) % 3 != 0).astype(np.uint8)}
    return cols, [0]


def utf8_key(n):
    rng = np.random.default_rng(11)
    return [random_col(rng, n, "utf8", 0)] + sig_cols("i64", n)[1:], [0]


FALLBACKS = {
    "nullable_key": nullable_key,
    "utf8_key": utf8_key,
    "three_keys": lambda n: (sig_cols("i64+i32", n), [0, 3, 4]),
    "pair_i32_i64": lambda n: (sig_cols("i64+i32", n), [4, 0]),
    "pair_i64_i64": lambda n: (sig_cols("i64", n)[:1] + sig_cols("i64+i32", n), [0, 1]),
}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_is_generic(case, kernel, monkeypatch):
    """What the whitelist leaves out reports k1_spec() == 0 and stays oracle-exact."""
    cols, key_idx = FALLBACKS[case](2 * 4096 + 5)
    oracle_check(monkeypatch, ("fb", case), cols, key_idx, 128, KERNELS[kernel][0], spec=0)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("sig", sorted(SIGS))
def test_knob_forces_generic(sig, kernel, monkeypatch):
    _, key_idx, _, _ = SIGS[sig]
    n = 4096 + 257
    oracle_check(monkeypatch, (sig, n), sig_cols(sig, n), key_idx, 128,
                 {**KERNELS[kernel][0], "DD_K1_SPEC": "0"}, spec=0)


def special_floats(dtype, n):
    """-0.0, +0.0, and quiet/signalling NaNs of both signs with different payloads,
    cycled through a column of ordinary values."""
    if dtype == "f32":
        bits = np.array([0x80000000, 0x00000000, 0x7fc00000, 0xffc00000, 0x7fc00001,
                         0x7f800001, 0xff800123, 0x7fffffff, 0x3f800000, 0xbf800000],
                        dtype=np.uint32)
        fdt = np.float32
    else:
        bits = np.array([0x8000000000000000, 0x0, 0x7ff8000000000000, 0xfff8000000000000,
                         0x7ff8000000000001, 0x7ff0000000000001, 0xfff0000000000123,
                         0x7fffffffffffffff, 0x3ff0000000000000, 0xbff0000000000000],
                        dtype=np.uint64)
        fdt = np.float64
    data = np.random.default_rng(3).normal(size=n).astype(fdt)
    idx = np.arange(0, n, 3)
    data.view(bits.dtype)[idx] = bits[np.arange(len(idx)) % len(bits)]
    return data


@pytest.mark.parametrize("nparts", [7, 128])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_float_keys(dtype, kernel, nparts, monkeypatch):
    """Signed zeros hash alike and every NaN hashes as the canonical one, as the oracle."""
    n = 4096 + 257
    cols = sig_cols(dtype, n)
    cols[0] = {**cols[0], "data": special_floats(dtype, n)}
    pid = oracle.pids(oracle.hash_cols([cols[0]], n), nparts)
    d = cols[0]["data"]
    assert len(set(pid[np.isnan(d)])) == 1 and len(set(pid[d == 0])) == 1
    plan = oracle_check(monkeypatch, ("fl", dtype), cols, [0], nparts, KERNELS[kernel][0],
                        spec=SIGS[dtype][2])
    took_kernel(plan, kernel, SIGS[dtype][3](nparts))


def dict_cols(kind, n):
    vals = [b"ab", b"", b"ab", b"xyz", b"ab", b"q", b"xyz", b"longer value 0123456789"]
    doff = np.zeros(len(vals) + 1, dtype=np.int32)
    doff[1:] = np.cumsum([len(v) for v in vals])
    idx = (np.full(n, 4) if kind == "all_equal"
           else np.random.default_rng(8).integers(0, len(vals), n)).astype(np.int32)
    cols = sig_cols("dict32", n)
    cols[0] = {"dtype": "dict32", "data": idx, "valid": None, "dict_offsets": doff,
               "dict_bytes": np.frombuffer(b"".join(vals), dtype=np.uint8).copy()}
    return cols


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("kind", ["duplicates", "all_equal"])
def test_dict32_keys(kind, kernel, monkeypatch):
    """A dictionary with duplicate values (equal bytes share a partition), and every index
    equal (all LDS adds of a wave hit one counter)."""
    n = 2 * 4096 + 17
    cols = dict_cols(kind, n)
    plan = oracle_check(monkeypatch, ("dict", kind), cols, [0], 128, KERNELS[kernel][0],
                        spec=0x7)
    took_kernel(plan, kernel, True)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("skew", ["one_key", "presorted"])
@pytest.mark.parametrize("sig,nparts", [("i64", 128), ("i64", 512), ("i64+i32", 128),
                                        ("u8+bool", 128), ("dict32", 128)])
def test_skew(sig, nparts, skew, kernel, monkeypatch):
    """one_key: every row in one partition (roundcnt = R, the last segment's
    segoff = R - SEG); presorted: input already in partition order."""
    _, key_idx, code, pre = SIGS[sig]
    n = 3 * 4096 + 17
    cols = sig_cols(sig, n)
    if skew == "presorted":
        pid = oracle.pids(oracle.hash_cols([cols[k] for k in key_idx], n), nparts)
        perm = np.argsort(pid, kind="stable")
        cols = [{**c, "data": np.ascontiguousarray(c["data"][perm])} for c in cols]
    else:
        for k in key_idx:
            cols[k] = {**cols[k], "data": np.zeros(n, dtype=cols[k]["data"].dtype)}
    plan = oracle_check(monkeypatch, ("skew", sig, skew), cols, key_idx, nparts,
                        KERNELS[kernel][0], spec=code)
    took_kernel(plan, kernel, pre(nparts))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_ranged_runs_specialised(kernel, monkeypatch):
    """pid_shift > 0 (create_ranged: 512 fine partitions in 128 contiguous buckets) goes
    through the specialised body, which applies the shift itself."""
    set_env(monkeypatch, KERNELS[kernel][0])
    total, div, n = 512, 4, 3 * 4096 + 17
    cols = sig_cols("i64", n)
    pid = (oracle.pids(oracle.hash_cols([cols[0]], n), total) // div).astype(np.uint32)
    ordr, poff = oracle.order(pid, total // div)
    ref = {"pid": pid, "part_offsets": poff,
           "cols": [{"data": oracle.gather_fixed(c["data"], ordr)} for c in cols]}
    batch = api.DeviceBatch(cols)
    part = api.Partitioner(batch, [0], None, ranged=(total, div))
    try:
        assert part.k1_spec() == 0x4
        took_kernel((part.info(), part.pre_layout(), part.k1_spec()), kernel, True)
        part.run()
        part.sync()
        compare_to_oracle(part, cols, [0], total // div, ref=ref)
    finally:
        part.destroy()
        batch.free()
