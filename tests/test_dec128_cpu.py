"""Decimal128 columns, host side (CPU): the column dict api.dec128_col builds
from a pyarrow Decimal128Array is pyarrow's own value buffer and validity, the dtype tables
carry the new code, the C descriptor keeps its size, and the wire writer refuses the dtype
out loud."""

import ctypes
import decimal

import numpy as np
import pyarrow as pa
import pytest

from datafusion_distributed_amd import api
from datafusion_distributed_amd.wire import IpcField


def _decimals(n, null_every):
    rng = np.random.default_rng(16)
    cents = rng.integers(-(10**13), 10**13, n)
    return [None if null_every and i % null_every == 0
            else decimal.Decimal(int(c)).scaleb(-2) for i, c in enumerate(cents)]


@pytest.mark.parametrize("null_every", [0, 3, 1], ids=["nonull", "nulls", "allnull"])
def test_dec128_col_round_trip(null_every):
    n = 1001
    typ = pa.decimal128(15, 2)
    arr = pa.array(_decimals(n, null_every), type=typ)
    col = api.dec128_col(arr)
    assert col["dtype"] == "dec128" and (col["precision"], col["scale"]) == (15, 2)
    assert col["data"].dtype == np.uint64 and col["data"].shape == (n, 2)
    assert col["data"].nbytes == 16 * n
    assert (col["valid"] is None) == (null_every == 0)
    if col["valid"] is not None:
        assert col["valid"].dtype == np.uint8 and len(col["valid"]) == n
        assert (col["valid"] != 0).tolist() == arr.is_valid().to_pylist()
    # the value words are the little-endian two's-complement halves of the unscaled value
    for i in (1, 2, n - 1):
        if arr[i].is_valid:
            unscaled = int(arr[i].as_py().scaleb(2)) % (1 << 128)
            assert int(col["data"][i, 0]) == unscaled & (2**64 - 1)
            assert int(col["data"][i, 1]) == unscaled >> 64
    # and from_buffers rebuilds the array from them, as partition_batches does
    bitmap = None
    if col["valid"] is not None:
        bitmap = pa.py_buffer(np.packbits(col["valid"], bitorder="little").tobytes())
    back = pa.Array.from_buffers(typ, n, [bitmap, pa.py_buffer(col["data"].tobytes())])
    assert back.equals(arr)


def test_dec128_col_of_a_slice_and_wrong_type():
    arr = pa.array(_decimals(100, 4), type=pa.decimal128(20, 3))
    col = api.dec128_col(arr.slice(7, 50))
    whole = api.dec128_col(arr)
    assert np.array_equal(col["data"], whole["data"][7:57])
    assert np.array_equal(col["valid"], whole["valid"][7:57])
    with pytest.raises(TypeError):
        api.dec128_col(pa.array([1, 2, 3], type=pa.int64()))


def test_fixed_host_accepts_any_16_byte_rows():
    words = np.arange(12, dtype=np.uint64).reshape(6, 2)
    for data in (words, words.view(np.int64), words.reshape(-1), words.view(np.uint8)):
        got = api.fixed_host({"dtype": "dec128", "data": data})
        assert got.dtype == np.uint64 and np.array_equal(got, words)
    with pytest.raises(ValueError):
        api.fixed_host({"dtype": "dec128", "data": np.zeros(9, dtype=np.uint8)})
    with pytest.raises(ValueError):
        api.fixed_host({"dtype": "dec128", "data": words[:, ::-1]})


def test_dtype_tables_and_descriptor_size():
    assert api.DTYPE_CODE["dec128"] == 10
    assert api.ELEM_SIZE["dec128"] == 16
    assert api.FIXED_NP["dec128"] is np.uint64
    assert ctypes.sizeof(api.ColDesc) == 64


def test_wire_writer_refuses_dec128():
    L = api.lib()
    fields = (IpcField * 2)()
    fields[0].dtype, fields[0].name, fields[0].nullable = api.DTYPE_CODE["i64"], b"k", 0
    fields[1].dtype, fields[1].name, fields[1].nullable = api.DTYPE_CODE["dec128"], b"d", 1
    w = ctypes.c_void_p()
    st = L.dd_ipc_writer_create(fields, 2, 0, ctypes.byref(w))
    assert st == 6  # DD_ERR_UNSUPPORTED
    assert b"dec128" in L.dd_last_error()
