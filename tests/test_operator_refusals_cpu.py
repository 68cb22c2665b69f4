"""The refusal paths of the operators above the shuffle (final merge, hash join, outer join,
sort / top-k), checked without a device.

Every refusal these operators make happens before the device is touched, so a batch of
made-up pointers reaches all of them. Each named case below is run and its outcome (status
and the full message; for the zero-row successes the row count and the segment offsets) is
compared with tests/golden/operator_refusals.json. The golden file records what the library
answered BEFORE the host paths of these operators were consolidated; it is re-recorded only
when a message is changed on purpose:

    python tests/test_operator_refusals_cpu.py        # rewrites the golden file

The module skips itself where a device is present: there a lost check would go on to launch
kernels on the made-up pointers, whereas without a device it ends in DD_ERR_NO_DEVICE and a
failed comparison."""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datafusion_distributed_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "operator_refusals.json")


# ---------------- made-up inputs ----------------

def fake(dtypes, n_rows=8, valid=(), misaligned=(), raw_dtype=None):
    """A batch of made-up pointers. misaligned: columns whose data pointer is 8 (not 16)
    bytes aligned; raw_dtype: {col: code} written over the dtype the library is shown."""
    b = api.DeviceBatch.from_device(
        [{"dtype": dt, "data_ptr": 0x100000 * (i + 1) + (8 if i in misaligned else 0),
          "valid_ptr": 0x800000 * (i + 1) if i in valid else None,
          "offsets_ptr": 0x900000 if dt == "utf8" else None}
         for i, dt in enumerate(dtypes)], n_rows)
    for i, code in (raw_dtype or {}).items():
        b.desc.cols[i].dtype = code
    return b


def n_cols(batch, n):
    batch.desc.n_cols = n
    return batch


def lay(off, part, n_parts):
    return {"seg_offsets": off, "seg_part": part, "n_parts": n_parts}


OK2 = lay([0, 3, 8], [0, 1], 2)
BAD_LAYOUTS = {  # over 8 rows
    "short_end": lay([0, 3, 7], [0, 1], 2),
    "late_start": lay([1, 3, 8], [0, 1], 2),
    "decrease": lay([0, 9, 8], [0, 1], 2),
    "part_high": lay([0, 3, 8], [0, 2], 2),
    "part_negative": lay([0, 3, 8], [-1, 1], 2),
    "no_partition": lay([0, 8], [0], 0),
    "no_segment": lay([0], [], 2),
}
# two partitions of 2^30 and 2^30 - 1 rows: two table regions of 2^31 slots
HUGE = 2**31 - 1
HUGE_LAYOUT = lay([0, 2**30, HUGE], [0, 1], 2)
BAD_DTYPES = {"f32": "f32", "f64": "f64", "dict32": "dict32", "utf8": "utf8",
              "dec128": "dec128", "unknown": 99}


def with_dtype(dt, others=("i64",), **kw):
    """fake() whose column 0 is `dt` (a name, or a raw code the api has no name for)."""
    if isinstance(dt, str):
        return fake([dt, *others], **kw)
    return fake(["i64", *others], raw_dtype={0: dt}, **kw)


# ---------------- raw entries, for arguments the api cannot express ----------------

def _i32(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _layout_args(layout):
    off = np.ascontiguousarray(layout["seg_offsets"], dtype=np.int64)
    part = np.ascontiguousarray(layout["seg_part"], dtype=np.int32)
    return (off, part), [off.ctypes.data_as(ctypes.c_void_p),
                         part.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(len(part)),
                         ctypes.c_int32(layout["n_parts"])]


def raw_final_merge(batch, keys, states, ops, nns, layout=None, null=None):
    keep, lay_args = _layout_args(layout or lay([0, batch.n_rows], [0], 1))
    args = [ctypes.byref(batch.desc), _i32(keys), len(keys), _i32(states), _i32(ops),
            _i32(nns), len(states), *lay_args, None]
    h = ctypes.c_void_p()
    args.append(ctypes.byref(h))
    if null is not None:
        args[null] = None
    api._check(api.lib().dd_final_merge_run(*args))
    api.lib().dd_finalizer_destroy(h)


def raw_join(entry, join_type, build=None, probe=None, n_keys=1, null=None):
    build = build or fake(["i64"])
    probe = probe or fake(["i64"])
    kb, bl = _layout_args(lay([0, build.n_rows], [0], 1))
    kp, pl = _layout_args(lay([0, probe.n_rows], [0], 1))
    keys = _i32(list(range(n_keys)))
    h = ctypes.c_void_p()
    args = [ctypes.byref(build.desc), keys, ctypes.byref(probe.desc), keys,
            ctypes.c_int32(n_keys), ctypes.c_int32(join_type), *bl, *pl, _i32([0]),
            ctypes.c_int32(0), _i32([0]), ctypes.c_int32(0), None, ctypes.byref(h)]
    if null is not None:
        args[null] = None
    api._check(getattr(api.lib(), entry)(*args))
    api.lib().dd_joiner_destroy(h)


def raw_sort(batch, keys, flags, fetch=-1, null=None):
    keep, lay_args = _layout_args(lay([0, batch.n_rows], [0], 1))
    h = ctypes.c_void_p()
    args = [ctypes.byref(batch.desc), _i32(keys), _i32(flags), ctypes.c_int32(len(keys)),
            _i32([0]), ctypes.c_int32(0), *lay_args, ctypes.c_int64(fetch), None,
            ctypes.byref(h)]
    if null is not None:
        args[null] = None
    api._check(api.lib().dd_sort_run(*args))
    api.lib().dd_sorter_destroy(h)


# ---------------- the case table ----------------

CASES = {}


def case(name, fn, *args, **kw):
    assert name not in CASES, name
    CASES[name] = lambda: fn(*args, **kw)


def final_merge_cases():
    SUM = [(1, "sum_i64", 2)]
    three = ["i64", "i64", "i64"]
    for name, fm in (("final_merge", api.final_merge),
                     ("final_merge_device", api.final_merge_device)):
        c = lambda what, *a, **k: case(f"{name}/{what}", fm, *a, **k)
        for cause, bad in BAD_LAYOUTS.items():
            c(f"layout/{cause}", fake(three), [0], SUM, **bad)
        c("layout/one_entry_more", fake(three), [0], SUM, **lay([0, 8], [0, 1], 2))
        c("layout/table_past_2_32", fake(three, n_rows=HUGE), [0], SUM, **HUGE_LAYOUT)
        for cause, dt in BAD_DTYPES.items():
            if cause not in ("f32", "f64"):
                c(f"key_dtype/{cause}", with_dtype(dt, ["i64", "i64"]), [0], SUM)
        c("key_dtype/second_key", fake(["i64", "i64", "i64", "utf8"]), [0, 3], SUM)
        c("key_count/0", fake(three), [], SUM)
        c("key_count/5", fake(["i32"] * 7), [0, 1, 2, 3, 4], [(5, "sum_i64", 6)])
        c("key_index/negative", fake(three), [-1], SUM)
        c("key_index/high", fake(three), [3], SUM)
        c("n_rows/2_31", fake(three, n_rows=2**31), [0], SUM)
        c("n_rows/negative", fake(three, n_rows=-1), [0], SUM)
        c("n_cols/0", n_cols(fake(three), 0), [0], SUM)
        c("n_cols/25", n_cols(fake(three), 25), [0], SUM)
        c("aggs/0", fake(three), [0], [])
        c("aggs/9", fake(three), [0], SUM * 9)
        c("aggs/state_index_negative", fake(three), [0], [(-1, "sum_i64", 2)])
        c("aggs/state_index_high", fake(three), [0], [(3, "sum_i64", 2)])
        c("aggs/sum_dec128_state_i64", fake(three), [0], [(1, "sum_dec128", 2)])
        c("aggs/sum_dec128_misaligned", fake(["i64", "dec128", "i64"], misaligned=[1]), [0],
          [(1, "sum_dec128", 2)])
        for op in ("sum_f64", "min_f64", "max_f64"):
            c(f"aggs/{op}_state_i64", fake(three), [0], [(1, op, 2)])
        for op in ("sum_i64", "min_i64", "max_i64", "count"):
            c(f"aggs/{op}_state_f64", fake(["i64", "f64", "i64"]), [0],
              [(1, op, None if op == "count" else 2)])
        c("aggs/sum_i64_state_dec128", fake(["i64", "dec128", "i64"]), [0], SUM)
        c("aggs/nn_index_none", fake(three), [0], [(1, "sum_i64", None)])
        c("aggs/nn_index_high", fake(three), [0], [(1, "sum_i64", 3)])
        c("aggs/nn_dtype_i32", fake(["i64", "i64", "i32"]), [0], SUM)
        c("aggs/second_aggregate", fake(three), [0], [(1, "count", None), (1, "sum_f64", 2)])
        # two refusals at once: the order of the checks
        c("order/key_count_before_n_rows", fake(three, n_rows=2**31), [], SUM)
        c("order/n_rows_before_key_dtype", fake(["utf8", "i64", "i64"], n_rows=2**31), [0],
          SUM)
        c("order/key_dtype_before_aggregate", fake(["utf8", "i64", "i64"]), [0],
          [(1, "sum_f64", 2)])
        c("order/key_dtype_before_layout", fake(["utf8", "i64", "i64"]), [0], SUM,
          **BAD_LAYOUTS["decrease"])
        c("order/aggregate_before_layout", fake(three), [0], [(1, "sum_f64", 2)],
          **BAD_LAYOUTS["no_partition"])
        c("order/layout_end_before_decrease", fake(three), [0], SUM,
          **lay([0, 9, 7], [0, 1], 2))
        c("order/layout_decrease_before_part", fake(three), [0], SUM,
          **lay([0, 9, 8], [5, 1], 2))
        # successes without device work, and the call that needs the device
        c("zero_rows/one_partition", fake(three, n_rows=0), [0], SUM)
        c("zero_rows/three_partitions", fake(three, n_rows=0, valid=[0]), [0, 1],
          [(1, "count", None), (2, "max_i64", 2)], **lay([0, 0, 0, 0], [2, 0, 1], 3))
        c("needs_device", fake(three), [0], SUM)
    case("final_merge_raw/unknown_op_high", raw_final_merge, fake(three), [0], [1], [8], [2])
    case("final_merge_raw/unknown_op_negative", raw_final_merge, fake(three), [0], [1], [-1],
         [2])
    case("final_merge_raw/unknown_op_before_state_index", raw_final_merge, fake(three), [0],
         [9], [8], [2])
    for what, pos in (("batch", 0), ("key_cols", 1), ("state_cols", 3), ("agg_ops", 4),
                      ("nn_cols", 5), ("seg_offsets", 7), ("seg_part", 8), ("out", 12)):
        case(f"final_merge_raw/null_{what}", raw_final_merge, fake(three), [0], [1], [2], [2],
             null=pos)


def join_cases():
    one, two = ["i64"], ["i64", "i32"]
    entries = (("hash_join", api.hash_join, "inner"),
               ("outer_join", api.outer_join, "full"))
    for name, join, jt in entries:
        c = lambda what, *a, **k: case(f"{name}/{what}", join, *a, **k)
        for cause, bad in BAD_LAYOUTS.items():
            c(f"layout/build/{cause}", fake(one), [0], fake(one), [0], jt, build_layout=bad,
              probe_layout=OK2)
            c(f"layout/probe/{cause}", fake(one), [0], fake(one), [0], jt, build_layout=OK2,
              probe_layout=bad)
        c("layout/build/one_entry_more", fake(one), [0], fake(one), [0], jt,
          build_layout=lay([0, 8], [0, 1], 2), probe_layout=OK2)
        c("layout/probe/one_entry_more", fake(one), [0], fake(one), [0], jt,
          build_layout=OK2, probe_layout=lay([0, 8], [0, 1], 2))
        c("layout/unequal_n_parts", fake(one), [0], fake(one), [0], jt, build_layout=OK2,
          probe_layout=lay([0, 8], [0], 1))
        c("layout/unequal_n_parts_default_probe", fake(one), [0], fake(one), [0], jt,
          build_layout=OK2)
        c("layout/table_past_2_32", fake(one, n_rows=HUGE), [0], fake(one), [0], jt,
          build_layout=HUGE_LAYOUT, probe_layout=OK2)
        for cause, dt in BAD_DTYPES.items():
            c(f"key_dtype/build/{cause}", with_dtype(dt), [0], fake(two), [0], jt)
            c(f"key_dtype/probe/{cause}", fake(two), [0], with_dtype(dt), [0], jt)
            c(f"key_dtype/second_key/{cause}", with_dtype(dt), [1, 0], with_dtype(dt),
              [1, 0], jt)
        c("key_dtype/differ_pairwise", fake(two), [0], fake(two), [1], jt)
        c("key_dtype/differ_pairwise_u8_bool", fake(["u8"]), [0], fake(["bool"]), [0], jt)
        c("key_dtype/differ_pairwise_second", fake(two), [0, 1], fake(two), [0, 0], jt)
        c("key_count/0", fake(two), [], fake(two), [], jt)
        c("key_count/5", fake(["i32"] * 5), list(range(5)), fake(["i32"] * 5),
          list(range(5)), jt)
        c("key_count/unequal", fake(two), [0, 1], fake(two), [0], jt)
        c("key_index/build/high", fake(two), [2], fake(two), [0], jt)
        c("key_index/build/negative", fake(two), [-1], fake(two), [0], jt)
        c("key_index/probe/high", fake(two), [0], fake(two), [2], jt)
        c("key_index/probe/negative", fake(two), [0], fake(two), [-1], jt)
        c("n_rows/build/2_31", fake(one, n_rows=2**31), [0], fake(one), [0], jt)
        c("n_rows/probe/2_31", fake(one), [0], fake(one, n_rows=2**31), [0], jt)
        c("n_rows/build/negative", fake(one, n_rows=-1), [0], fake(one), [0], jt)
        c("n_cols/build/0", n_cols(fake(one), 0), [0], fake(one), [0], jt, build_proj=[])
        c("n_cols/probe/25", fake(one), [0], n_cols(fake(one), 25), [0], jt, probe_proj=[])
        for side in ("build", "probe"):
            def proj(what, dtypes, cols, **kw):
                bad, good = fake(dtypes, **kw), fake(two)
                b, p = (bad, good) if side == "build" else (good, bad)
                c(f"proj/{side}/{what}", b, [0], p, [0], jt, **{side + "_proj": cols})
            proj("utf8", ["i64", "utf8"], [0, 1])
            proj("dict32", ["i64", "dict32"], [1])
            proj("unknown_dtype", ["i64", "i64"], [1], raw_dtype={1: 99})
            proj("dec128_misaligned", ["i64", "dec128"], [1], misaligned=[1])
            proj("index_negative", two, [-1])
            proj("index_high", two, [0, 2])
            proj("list_of_25", two, [0] * 25)
            proj("default_includes_utf8", ["i64", "utf8"], None)
        c("proj/more_than_a_batch_holds", fake(two), [0], fake(two), [0], jt,
          build_proj=[0] * 13, probe_proj=[1] * 12)
        # two refusals at once: the order of the checks
        c("order/key_count_before_key_dtype", fake(["f32"] * 5), list(range(5)),
          fake(["f32"] * 5), list(range(5)), jt)
        c("order/build_key_before_probe_key", fake(["utf8"]), [0], fake(["f64"]), [0], jt)
        c("order/build_proj_before_probe_key", fake(["i64", "utf8"]), [0], fake(["f64"]), [0],
          jt, build_proj=[1])
        c("order/probe_key_before_build_layout", fake(one), [0], fake(["dict32"]), [0], jt,
          build_layout=BAD_LAYOUTS["decrease"], probe_layout=OK2)
        c("order/pairwise_before_layout", fake(two), [0], fake(two), [1], jt,
          build_layout=BAD_LAYOUTS["decrease"], probe_layout=OK2)
        c("order/build_layout_before_probe_layout", fake(one), [0], fake(one), [0], jt,
          build_layout=BAD_LAYOUTS["part_high"], probe_layout=BAD_LAYOUTS["short_end"])
        c("order/layout_before_unequal_n_parts", fake(one), [0], fake(one), [0], jt,
          build_layout=OK2, probe_layout=lay([0, 9, 8], [0, 0], 1))
        c("order/build_n_rows_before_build_key", fake(["f32"], n_rows=2**31), [0],
          fake(["f32"]), [0], jt)
        c("order/unequal_n_parts_before_table", fake(one, n_rows=HUGE), [0], fake(one), [0],
          jt, build_layout=HUGE_LAYOUT)
        c("join_type/unknown_name", fake(one), [0], fake(one), [0], "cross")
        c("needs_device", fake(two), [0], fake(two), [0], jt, build_layout=OK2,
          probe_layout=OK2)

    c = lambda what, *a, **k: case(f"hash_join/{what}", api.hash_join, *a, **k)
    for jt in ("left", "right", "full"):
        c(f"join_type/{jt}", fake(one), [0], fake(one), [0], jt)
    for jt, side in (("left_semi", "probe"), ("left_anti", "probe"), ("right_semi", "build"),
                     ("right_anti", "build")):
        c(f"proj/{jt}_with_{side}_list", fake(two), [0], fake(two), [0], jt,
          **{side + "_proj": [1]})
        c(f"needs_device/{jt}", fake(two), [0], fake(two), [0], jt)
    c("order/join_type_before_key_count", fake(one), [0, 0, 0, 0, 0], fake(one),
      [0, 0, 0, 0, 0], "left")
    c("order/key_count_before_semi_proj", fake(two), [], fake(two), [], "left_semi",
      probe_proj=[0])
    c("order/semi_proj_before_key_dtype", fake(["f32"]), [0], fake(["f32"]), [0],
      "right_anti", build_proj=[0])
    c("zero_rows/inner_empty_probe", fake(two), [0], fake(two, n_rows=0), [0], "inner",
      build_layout=OK2, probe_layout=lay([0, 0, 0, 0], [1, 0, 1], 2))
    c("zero_rows/inner_unprojected_utf8", fake(["i64", "utf8"]), [0], fake(one, n_rows=0),
      [0], build_proj=[0])
    c("zero_rows/right_anti_empty_probe", fake(two), [0], fake(two, n_rows=0), [0],
      "right_anti")
    c("zero_rows/left_semi_empty_build", fake(two, n_rows=0), [0], fake(two), [0],
      "left_semi", build_layout=lay([0, 0, 0], [0, 1], 2), probe_layout=OK2)
    c("needs_device/left_anti_empty_probe", fake(two), [0], fake(two, n_rows=0), [0],
      "left_anti")
    c("needs_device/inner_empty_build", fake(two, n_rows=0), [0], fake(two), [0], "inner")

    c = lambda what, *a, **k: case(f"outer_join/{what}", api.outer_join, *a, **k)
    for jt in ("inner", "left_semi", "left_anti", "right_semi", "right_anti"):
        c(f"join_type/{jt}", fake(one), [0], fake(one), [0], jt)
    for jt in ("left", "right"):
        c(f"needs_device/{jt}", fake(two), [0], fake(two), [0], jt)
    c("order/join_type_before_key_count", fake(one), [], fake(one), [], "inner")
    c("zero_rows/right_empty_probe", fake(two), [0], fake(two, n_rows=0), [0], "right",
      build_layout=OK2, probe_layout=lay([0, 0, 0, 0], [1, 0, 1], 2))
    c("zero_rows/left_both_empty", fake(two, n_rows=0, valid=[1]), [0], fake(two, n_rows=0),
      [0], "left", build_layout=lay([0, 0, 0], [0, 1], 2),
      probe_layout=lay([0, 0, 0, 0], [1, 0, 1], 2))
    c("zero_rows/full_both_empty", fake(two, n_rows=0), [0], fake(two, n_rows=0), [0],
      "full", build_proj=[1], probe_proj=[])
    c("needs_device/left_empty_probe", fake(two), [0], fake(two, n_rows=0), [0], "left")
    c("needs_device/right_empty_build", fake(two, n_rows=0), [0], fake(two), [0], "right")

    for entry in ("dd_hash_join_run", "dd_hash_join_outer_run"):
        for jt in (-1, 8):
            case(f"{entry}/join_type/{jt}", raw_join, entry, jt)
        case(f"{entry}/order/join_type_before_key_count", raw_join, entry, 8, n_keys=0)
        case(f"{entry}/order/null_before_join_type", raw_join, entry, 8, null=0)
        for what, pos in (("build", 0), ("build_keys", 1), ("probe", 2), ("probe_keys", 3),
                          ("build_seg_offsets", 6), ("build_seg_part", 7),
                          ("probe_seg_offsets", 10), ("probe_seg_part", 11), ("out", 19)):
            case(f"{entry}/null_{what}", raw_join, entry, 0 if "outer" not in entry else 7,
                 null=pos)
    # a null projection list is refused only when it is not empty: n_proj stays 0 here
    case("dd_hash_join_run/null_build_proj_of_0", raw_join, "dd_hash_join_run", 0, null=14)


def sort_cases():
    two = ["i64", "i32"]
    K = [(0, False, False)]
    c = lambda what, *a, **k: case(f"sort_topk/{what}", api.sort_topk, *a, **k)
    for cause, bad in BAD_LAYOUTS.items():
        c(f"layout/{cause}", fake(two), K, layout=bad)
    c("layout/one_entry_more", fake(two), K, layout=lay([0, 8], [0, 1], 2))
    for cause in ("dict32", "utf8", "unknown"):
        c(f"key_dtype/{cause}", with_dtype(BAD_DTYPES[cause]), K)
    c("key_dtype/dec128_misaligned", fake(["dec128", "i64"], misaligned=[0]), K)
    c("key_dtype/second_key", fake(["i64", "utf8"]), [(0, True, False), (1, False, True)],
      proj=[0])
    c("key_count/0", fake(two), [])
    c("key_count/5", fake(two), K * 5)
    c("key_index/negative", fake(two), [(-1, False, False)])
    c("key_index/high", fake(two), [(2, False, False)])
    c("keys/not_triples", fake(two), [0])
    c("fetch/minus_1", fake(two), K, fetch=-1)
    c("fetch/minus_5", fake(two), K, fetch=-5)
    c("fetch/not_an_integer", fake(two), K, fetch=1.5)
    c("n_rows/2_31", fake(two, n_rows=2**31), K)
    c("n_rows/negative", fake(two, n_rows=-1), K)
    c("n_cols/0", n_cols(fake(two), 0), K, proj=[])
    c("n_cols/25", n_cols(fake(two), 25), K, proj=[])
    c("proj/utf8", fake(["i64", "utf8"]), K, proj=[0, 1])
    c("proj/default_includes_utf8", fake(["i64", "utf8"]), K)
    c("proj/dict32", fake(["i64", "dict32"]), K, proj=[1])
    c("proj/unknown_dtype", fake(two, raw_dtype={1: 99}), K, proj=[1])
    c("proj/dec128_misaligned", fake(["i64", "dec128"], misaligned=[1]), K, proj=[1])
    c("proj/index_negative", fake(two), K, proj=[-1])
    c("proj/index_high", fake(two), K, proj=[0, 2])
    c("proj/list_of_25", fake(two), K, proj=[0] * 25)
    c("order/key_count_before_fetch", fake(two), [], fetch=-3)
    c("order/fetch_before_n_rows", fake(two, n_rows=2**31), K, fetch=-3)
    c("order/n_rows_before_key_dtype", fake(["utf8"], n_rows=2**31), K)
    c("order/key_dtype_before_proj", fake(["dict32", "utf8"]), K, proj=[1])
    c("order/proj_before_layout", fake(["i64", "utf8"]), K, proj=[1],
      layout=BAD_LAYOUTS["decrease"])
    c("order/key_dtype_before_layout", fake(["utf8"]), K, layout=BAD_LAYOUTS["no_partition"])
    c("zero_rows/no_rows", fake(two, n_rows=0), K, layout=lay([0, 0, 0, 0], [2, 0, 1], 3))
    c("zero_rows/fetch_0", fake(two), K, layout=OK2, fetch=0, proj=[1])
    c("zero_rows/dec128_key_words", fake(["dec128", "i64"], n_rows=0, valid=[0]),
      [(0, True, True), (1, False, False)], proj=[])
    c("needs_device", fake(two), K, layout=OK2, fetch=3)
    case("dd_sort_run/flag_bits_4", raw_sort, fake(two), [0], [4])
    case("dd_sort_run/flag_bits_negative", raw_sort, fake(two), [0], [-1])
    case("dd_sort_run/flag_bits_second_key", raw_sort, fake(two), [0, 1], [3, 8])
    case("dd_sort_run/order/key_index_before_flag_bits", raw_sort, fake(two), [2], [4])
    case("dd_sort_run/order/flag_bits_before_key_dtype", raw_sort, fake(["utf8"]), [0], [4])
    case("dd_sort_run/fetch_minus_2", raw_sort, fake(two), [0], [0], fetch=-2)
    for what, pos in (("batch", 0), ("key_cols", 1), ("key_flags", 2), ("seg_offsets", 6),
                      ("seg_part", 7), ("out", 12)):
        case(f"dd_sort_run/null_{what}", raw_sort, fake(two), [0], [0], null=pos)


final_merge_cases()
join_cases()
sort_cases()


# ---------------- outcomes ----------------

def describe(res):
    """What a success is held to: the row count and the segment offsets (and, per class, the
    few facts a zero-row result still carries)."""
    if isinstance(res, api.Joined):
        out = {"n_rows": res.n_rows, "out_cols": [[dt, v] for dt, v in res._out_cols],
               **{k: np.asarray(v).tolist() for k, v in res.layout().items()}}
    elif isinstance(res, api.Sorted):
        out = {"n_rows": res.n_rows, "info": res.info(), "perm": res.perm().tolist(),
               **{k: np.asarray(v).tolist() for k, v in res.layout().items()}}
    elif isinstance(res, api.Merged):
        out = {"n_groups": res.n_groups, "n_cols": res.n_cols, "dtypes": res.dtypes,
               **{k: np.asarray(v).tolist() for k, v in res.layout().items()}}
    elif isinstance(res, dict):  # final_merge
        return {k: [list(v.shape), v.tolist()] if isinstance(v, np.ndarray) else v
                for k, v in res.items()}
    else:
        return None
    res.destroy()
    return out


def outcome(name):
    try:
        res = CASES[name]()
    except api.DDError as e:
        return {"status": e.status, "message": str(e)}
    except ValueError as e:
        return {"status": "ValueError", "message": str(e)}
    return {"status": 0, "result": describe(res)}


_golden = {}
if __name__ != "__main__":
    with open(GOLDEN) as _f:
        _golden = json.load(_f)

pytestmark = pytest.mark.skipif(api.device_count() > 0,
                                reason="GPU present: a lost check would launch kernels on "
                                       "made-up pointers")


def test_golden_file_holds_exactly_these_cases():
    assert sorted(_golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outcome_is_the_recorded_one(name):
    assert outcome(name) == _golden[name]


if __name__ == "__main__":
    assert api.device_count() == 0, "record on a machine without a device"
    recorded = {name: outcome(name) for name in sorted(CASES)}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(recorded)} cases to {GOLDEN}")
