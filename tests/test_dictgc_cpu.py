"""Dictionary GC host model + ABI guard (CPU). gc_windows_ref / merge_producers_ref are the
numpy statement of DESIGN.md §14 that the GPU tests compare the kernels with; here they are
checked against pyarrow's own decode of the same DictionaryArrays."""

import ctypes

import numpy as np
import pytest

from datafusion_distributed_amd import api
from datafusion_distributed_amd.dictgc import decode, gc_windows_ref, merge_producers_ref

# 6 values: an empty string, a duplicated value (1 and 4) and a non-UTF-8 value
VALUES = [b"", b"dup", b"beta", b"\xff\xfe", b"dup", b"zeta"]


def _dict(values):
    off = np.zeros(len(values) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in values])
    return off, np.frombuffer(b"".join(values), dtype=np.uint8)


def _pa_dict_array(idx, valid, off, data):
    import pyarrow as pa

    values = pa.BinaryArray.from_buffers(
        pa.binary(), len(off) - 1, [None, pa.py_buffer(np.asarray(off, np.int32).tobytes()),
                                    pa.py_buffer(np.asarray(data, np.uint8).tobytes())])
    mask = None if valid is None else ~np.asarray(valid).astype(bool)
    return pa.DictionaryArray.from_arrays(pa.array(idx, type=pa.int32(), mask=mask), values)


def _rows():
    # 20 rows in 4 partitions of 5; index 5 ("zeta") is never used by a valid row
    idx = np.array([4, 1, 0, 3, 1, 2, 2, 0, 5, 4, 3, 3, 1, 0, 2, 4, 4, 1, 5, 0],
                   dtype=np.int32)
    valid = np.ones(20, dtype=np.uint8)
    valid[[3, 8, 12, 18]] = 0  # both rows that reference index 5 are null
    row_off = np.array([0, 5, 10, 15, 20], dtype=np.int64)
    return idx, valid, row_off


@pytest.mark.parametrize("W", [1, 4])
def test_gc_windows_ref_matches_pyarrow_decode(W):
    idx, valid, row_off = _rows()
    off, data = _dict(VALUES)
    ref = gc_windows_ref(idx, valid, row_off, off, data, W)
    original = _pa_dict_array(idx, valid, off, data).dictionary_decode()
    ppw = 4 // W
    assert (ref["indices"][valid == 0] == 0).all()  # null rows are 0
    for w in range(W):
        r0, r1 = int(row_off[w * ppw]), int(row_off[(w + 1) * ppw])
        wi, wv = idx[r0:r1], valid[r0:r1].astype(bool)
        used = ref["used"][w]
        # compacted length == number of distinct used indices; survivors ascend
        assert len(ref["offsets"][w]) - 1 == len(set(wi[wv].tolist())) == len(used)
        assert (np.diff(used) > 0).all()
        assert 5 not in used  # referenced by null rows only
        new = _pa_dict_array(ref["indices"][r0:r1], valid[r0:r1], ref["offsets"][w],
                             ref["bytes"][w])
        assert new.dictionary_decode().equals(original.slice(r0, r1 - r0))
        assert ref["val_off"][w + 1] - ref["val_off"][w] == len(used)
        assert ref["byte_off"][w + 1] - ref["byte_off"][w] == int(ref["offsets"][w][-1])
    if W == 1:
        # GC is not dedup: both "dup" entries (1 and 4) survive as two entries
        assert ref["used"][0].tolist() == [0, 1, 2, 3, 4]
        assert ref["bytes"][0].tobytes() == b"dupbeta\xff\xfedup"


def test_gc_windows_ref_edges():
    off, data = _dict(VALUES)
    # no valid rows: empty dictionary, single offsets entry 0
    ref = gc_windows_ref(np.zeros(3, np.int32), np.zeros(3, np.uint8),
                         np.array([0, 3], np.int64), off, data, 1)
    assert ref["offsets"][0].tolist() == [0] and len(ref["bytes"][0]) == 0
    assert (ref["indices"] == 0).all()
    # n_rows == 0 and dict_n == 0 are legal
    ref = gc_windows_ref(np.zeros(0, np.int32), None, np.array([0, 0, 0], np.int64),
                         np.zeros(1, np.int32), np.zeros(0, np.uint8), 2)
    assert [o.tolist() for o in ref["offsets"]] == [[0], [0]]
    # a valid out-of-range index is an error; a null one is not
    with pytest.raises(ValueError):
        gc_windows_ref(np.array([6], np.int32), None, np.array([0, 1], np.int64), off, data, 1)
    gc_windows_ref(np.array([6], np.int32), np.zeros(1, np.uint8),
                   np.array([0, 1], np.int64), off, data, 1)
    with pytest.raises(ValueError):
        gc_windows_ref(np.zeros(1, np.int32), None, np.array([0, 1, 1, 1], np.int64), off,
                       data, 2)


def test_merge_producers_ref_decodes_as_concatenation():
    import pyarrow as pa

    off_a, data_a = _dict([b"x", b"", b"\xff\xfe"])
    off_c, data_c = _dict([b"x", b"tail"])  # "x" again: duplicates across producers stay
    producers = [
        (np.array([2, 0, 0, 1], np.int32), np.array([1, 1, 0, 1], np.uint8), off_a, data_a),
        (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(1, np.int32),
         np.zeros(0, np.uint8)),  # empty dictionary, zero rows
        (np.array([1, 1, 0], np.int32), None, off_c, data_c),
    ]
    m = merge_producers_ref(producers)
    assert m["vals_per_producer"].tolist() == [3, 0, 2]
    assert m["offsets"].tolist() == [0, 1, 1, 3, 4, 8] and m["offsets"].dtype == np.int32
    assert m["bytes"].tobytes() == b"x\xff\xfextail"
    assert m["indices"].tolist() == [2, 0, 0, 1, 4, 4, 3]
    want = sum((decode(*p) for p in producers), [])
    assert decode(m["indices"], m["valid"], m["offsets"], m["bytes"]) == want
    got = _pa_dict_array(m["indices"], m["valid"], m["offsets"], m["bytes"])
    assert got.dictionary_decode().equals(pa.array(want, type=pa.binary()))


def test_dict_gc_run_null_argument_guard():
    L = api.lib()
    out = ctypes.c_void_p()
    assert L.dd_dict_gc_run(None, 0, 1, None, ctypes.byref(out)) == 1  # DD_ERR_INVALID
    assert L.dd_last_error() != b""
    assert L.dd_dict_rebase(None, 0, None, None, 0, None, None) == 1
