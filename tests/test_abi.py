"""C-ABI surface tests (CPU): the library loads, every symbol declared in
include/dd_shuffle.h resolves, and the no-GPU path fails loudly (no CPU fallback)."""

import ctypes
import os
import re

import numpy as np
import pytest

from datafusion_distributed_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dd_shuffle.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", src)
    # drop type names
    return sorted(set(n for n in names if not n.endswith("_t")))


def test_header_symbols_all_exported():
    L = api.lib()
    missing = []
    for name in declared_functions():
        try:
            getattr(L, name)
        except AttributeError:
            missing.append(name)
    assert not missing, f"symbols declared in dd_shuffle.h but not exported: {missing}"


def test_version_and_device_count():
    L = api.lib()
    assert b"dd_shuffle" in L.dd_version()
    assert L.dd_device_count() >= 0


@pytest.mark.skipif(api.device_count() > 0, reason="GPU present: no-device path not testable")
def test_no_gpu_fails_loudly():
    cols = [{"dtype": "i64", "data": np.arange(8, dtype=np.int64), "valid": None}]
    with pytest.raises(api.DDError) as ei:
        batch = api.DeviceBatch(cols)  # first device alloc must already fail
        api.Partitioner(batch, [0], 4)
    assert ei.value.status == 2  # DD_ERR_NO_DEVICE


def test_batch_desc_layout_matches_c():
    # struct sizes must agree with the C side (compiled into the lib? — we pin the python
    # mirror against the header's field list instead: 8 fields, pointer-aligned)
    assert ctypes.sizeof(api.ColDesc) == 8 * 8  # int32+pad, 3 ptrs, i64, 2 ptrs, i64
    assert ctypes.sizeof(api.BatchDesc) == 8 + 8 + api.DD_MAX_COLS * ctypes.sizeof(api.ColDesc)
    assert ctypes.sizeof(api.TaskKeyC) == 32


def test_null_argument_guards():
    """Null-pointer arguments return DD_ERR_INVALID with a message — never crash.
    These guards run before any device work, so they are CPU-testable."""
    L = api.lib()
    assert L.dd_comm_unique_id(None) == 1  # DD_ERR_INVALID
    out = ctypes.c_void_p()
    assert L.dd_partitioner_create(None, None, 0, 0, ctypes.byref(out)) == 1
    key = api.TaskKeyC(0, 0, 0, 0)
    assert L.dd_execute_task(ctypes.byref(key), 0, 0, None, None) == 1
    assert L.dd_set_plan(None, None, None, 0, 0) == 1
    assert b"" != L.dd_last_error()  # message was set


def test_partitioner_info_layout_matches_header():
    """api.PartitionerInfo mirrors dd_partitioner_info field for field, in order and
    width, so info() reads what dd_partitioner_get_info wrote."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct dd_partitioner_info \{(.*?)\} dd_partitioner_info;",
                     src, flags=re.S).group(1)
    declared = []
    for ctype, names in re.findall(r"\b(int32_t|int64_t)\s+([^;]+);", body):
        declared += [(n.strip(), ctype) for n in names.split(",")]
    width = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t"}
    assert declared == [(n, width[t]) for n, t in api.PartitionerInfo._fields_]
    assert ctypes.sizeof(api.PartitionerInfo) == 10 * 4 + 2 * 8
    assert api.PartitionerInfo.round_rows.offset == 40
    out = api.PartitionerInfo()
    assert api.lib().dd_partitioner_get_info(None, ctypes.byref(out)) == 1  # INVALID


def _stub_batch(monkeypatch, cols):
    """A DeviceBatch built without a device: uploads get fake addresses, and any copy
    attempted afterwards fails the test."""
    addr = iter(range(0x1000, 0x100000, 0x1000))
    monkeypatch.setattr(api.DeviceBatch, "_up", lambda self, arr: next(addr))
    batch = api.DeviceBatch(cols)

    def no_copy(*a, **k):
        raise AssertionError("refill copied before it validated")

    monkeypatch.setattr(api, "_h2d", no_copy)
    monkeypatch.setattr(api, "lib", no_copy)
    return batch


def _refill_cols():
    doff = np.array([0, 2, 2, 5], dtype=np.int32)
    return [
        {"dtype": "i64", "data": np.arange(4, dtype=np.int64), "valid": None},
        {"dtype": "f64", "data": np.zeros(4), "valid": np.ones(4, dtype=np.uint8)},
        {"dtype": "utf8", "data": np.frombuffer(b"aabbbc", dtype=np.uint8),
         "offsets": np.array([0, 2, 5, 5, 6], dtype=np.int32), "valid": None},
        {"dtype": "dict32", "data": np.array([0, 1, 2, 0], dtype=np.int32),
         "dict_bytes": np.frombuffer(b"xxyyy", dtype=np.uint8), "dict_offsets": doff,
         "valid": None},
    ]


def test_refill_accepts_same_shape(monkeypatch):
    batch = _stub_batch(monkeypatch, _refill_cols())
    new = _refill_cols()
    new[0]["data"] = new[0]["data"][::-1].copy()
    new[2]["data"] = np.frombuffer(b"cccaab", dtype=np.uint8)  # "ccc", "aa", "", "b"
    new[2]["offsets"] = np.array([0, 3, 5, 5, 6], dtype=np.int32)
    new[3]["data"] = np.array([2, 2, 1, 0], dtype=np.int32)
    plan = batch._refill_plan(new)
    # data x4, validity x1, utf8 offsets x1 — and never the dictionary
    assert len(plan) == 6
    assert [dst for dst, _ in plan] == [batch.desc.cols[0].data, batch.desc.cols[1].data,
                                        batch.desc.cols[1].validity,
                                        batch.desc.cols[2].data, batch.desc.cols[2].offsets,
                                        batch.desc.cols[3].data]


def _bad_refills():
    def edit(fn):
        cols = _refill_cols()
        fn(cols)
        return cols

    def longer_string(c):  # same 6 bytes, but one 4-byte string; create-time max is 3
        c[2]["offsets"] = np.array([0, 4, 5, 5, 6], dtype=np.int32)

    def more_bytes(c):
        c[2]["data"] = np.frombuffer(b"aabbbcc", dtype=np.uint8)
        c[2]["offsets"] = np.array([0, 2, 5, 5, 7], dtype=np.int32)

    def other_dict(c):
        c[3]["dict_bytes"] = np.frombuffer(b"xxyyz", dtype=np.uint8)

    def other_dict_offsets(c):
        c[3]["dict_offsets"] = np.array([0, 1, 2, 5], dtype=np.int32)

    return {
        "fewer_columns": edit(lambda c: c.pop()),
        "dtype": edit(lambda c: c[0].update(dtype="i32",
                                            data=np.arange(4, dtype=np.int32))),
        "n_rows": edit(lambda c: c[0].update(data=np.arange(5, dtype=np.int64))),
        "validity_added": edit(lambda c: c[0].update(valid=np.ones(4, dtype=np.uint8))),
        "validity_dropped": edit(lambda c: c[1].update(valid=None)),
        "utf8_more_bytes": edit(more_bytes),
        "utf8_offsets_short_of_data_len": edit(
            lambda c: c[2].update(offsets=np.array([0, 2, 5, 5, 5], dtype=np.int32))),
        "utf8_longer_string": edit(longer_string),
        "dict_bytes": edit(other_dict),
        "dict_offsets": edit(other_dict_offsets),
        "dict_index_out_of_range": edit(
            lambda c: c[3].update(data=np.array([0, 1, 3, 0], dtype=np.int32))),
    }


@pytest.mark.parametrize("what", sorted(_bad_refills()))
def test_refill_refuses_before_copying(what, monkeypatch):
    """DeviceBatch.refill raises ValueError for anything outside the reuse contract and
    has copied nothing when it does (the batch here has no device behind it)."""
    batch = _stub_batch(monkeypatch, _refill_cols())
    before = batch.cols
    with pytest.raises(ValueError, match="refill"):
        batch.refill(_bad_refills()[what], stream=None)
    assert batch.cols is before
