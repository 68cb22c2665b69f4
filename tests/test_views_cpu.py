"""View columns, host side (CPU): the numpy models views.ingest_ref / views.emit_ref that the
GPU tests compare the kernels with are checked here against pyarrow's own cast of the same
view arrays, and the new exports' guards fail loudly without a device. pyarrow has no take /
filter kernel for views, so expectations are built on arr.cast(pa.string())."""

import ctypes

import numpy as np
import pyarrow as pa
import pytest

from datafusion_distributed_amd import api, arrow_boundary
from datafusion_distributed_amd.views import emit_ref, from_arrow, ingest_ref, to_arrow

LENGTHS = [0, 1, 4, 11, 12, 13, 64, 300]


def _values(rng, n, null_frac):
    vals = []
    for _ in range(n):
        ln = int(rng.choice(LENGTHS))
        vals.append(bytes(rng.integers(97, 123, ln, dtype=np.uint8)).decode())
    if null_frac >= 1.0:
        return [None] * n
    if null_frac > 0:
        for i in np.flatnonzero(rng.random(n) < null_frac):
            vals[i] = None
    return vals


def _view_array(rng, n, null_frac, n_bufs):
    """A string_view array whose long values live in exactly n_bufs data buffers (0 = all
    values inline), built by concatenating n_bufs chunks that each hold a long value."""
    if n_bufs == 0:
        vals = [None if v is None else v[:12] for v in _values(rng, n, null_frac)]
        return pa.array(vals, type=pa.string_view())
    chunks = []
    for c in np.array_split(np.arange(n), n_bufs):
        vals = _values(rng, len(c), null_frac) + ["L" * 40]  # every chunk owns a buffer
        chunks.append(pa.array(vals, type=pa.string_view()))
    arr = pa.concat_arrays(chunks)
    assert sum(b.size > 0 for b in arr.buffers()[2:]) == n_bufs
    return arr


def _cast_offsets_bytes(arr, binary=False):
    s = arr.cast(pa.binary() if binary else pa.string())
    vals = s.to_pylist()
    enc = [b"" if v is None else (v if binary else v.encode()) for v in vals]
    off = np.zeros(len(enc) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(e) for e in enc])
    return off, np.frombuffer(b"".join(enc), dtype=np.uint8)


def _one_partition(offsets, data):
    n = len(offsets) - 1
    return (np.diff(offsets).astype(np.uint32), np.array([0, n], np.int64),
            np.array([0, int(offsets[-1])], np.int64))


CASES = [(nf, nb, sl) for nf in (0.0, 0.1, 1.0) for nb in (0, 1, 2, 3)
         for sl in (False, True)]


@pytest.mark.parametrize("null_frac,n_bufs,sliced", CASES)
def test_ingest_ref_matches_cast_and_round_trips(null_frac, n_bufs, sliced):
    rng = np.random.default_rng(hash((null_frac, n_bufs, sliced)) % 2**32)
    arr = _view_array(rng, 97, null_frac, n_bufs)
    if sliced:
        arr = arr.slice(5, len(arr) - 9)
    views, valid, bufs = from_arrow(arr)
    assert views.shape == (len(arr), 16)
    assert sum(len(b) > 0 for b in bufs) == n_bufs  # pyarrow may append an empty buffer
    off, data = ingest_ref(views, valid, bufs)
    want_off, want_data = _cast_offsets_bytes(arr)
    assert off.dtype == np.int32 and np.array_equal(off, want_off)
    assert data.tobytes() == want_data.tobytes()

    # emit_ref(ingest_ref(x)) is x again, compacted
    lens, row_off, byte_off = _one_partition(off, data)
    em = emit_ref(lens, valid, data, row_off, byte_off, 1)
    back = to_arrow(em["views"], valid, em["bytes"][0])
    back.validate(full=True)
    assert back.cast(pa.string()).equals(arr.cast(pa.string()))
    ok = np.ones(len(arr), bool) if valid is None else valid.astype(bool)
    long_bytes = int(lens[ok & (lens > 12)].sum())
    assert len(em["bytes"][0]) == long_bytes == int(em["long_byte_off"][-1])
    if valid is not None:
        assert not em["views"][~ok].any()  # null rows are 16 zero bytes


def test_ingest_ref_ignores_null_garbage_and_refuses_bad_views():
    views = np.zeros((3, 16), dtype=np.uint8)
    w = views.view(np.int32).reshape(3, 4)
    w[0] = [0x7FFFFFFF, 0, 99, 5]  # garbage under a null
    w[1, 0] = 2
    views[1, 4:6] = (104, 105)
    w[2] = [20, 0, 0, 4]
    buf = np.arange(24, dtype=np.uint8)
    off, data = ingest_ref(views, np.array([0, 1, 1], np.uint8), [buf])
    assert off.tolist() == [0, 0, 2, 22]
    assert data.tobytes() == b"hi" + buf[4:24].tobytes()
    for bad in ([20, 0, 1, 4], [20, 0, 0, 5], [20, 0, 0, -1], [-1, 0, 0, 0]):
        w[2] = bad
        with pytest.raises(ValueError):
            ingest_ref(views, np.array([0, 1, 1], np.uint8), [buf])
    w[2] = [20, 0, 0, 4]
    with pytest.raises(ValueError):
        ingest_ref(views, None, [buf])  # row 0 is valid now


def test_emit_ref_windows_and_binary():
    rng = np.random.default_rng(11)
    vals = [bytes(rng.integers(0, 256, int(rng.choice(LENGTHS)), dtype=np.uint8))
            for _ in range(60)]
    vals[7] = b"\x00\xff" * 10
    arr = pa.array(vals, type=pa.binary_view())
    views, valid, bufs = from_arrow(arr)
    off, data = ingest_ref(views, valid, bufs)
    want_off, want_data = _cast_offsets_bytes(arr, binary=True)
    assert np.array_equal(off, want_off) and data.tobytes() == want_data.tobytes()
    # 4 partitions, the second one empty
    row_off = np.array([0, 15, 15, 40, 60], np.int64)
    byte_off = off[row_off].astype(np.int64)
    lens = np.diff(off).astype(np.uint32)
    for W in (1, 2, 4):
        em = emit_ref(lens, None, data, row_off, byte_off, W)
        ppw = 4 // W
        for w_ in range(W):
            r0, r1 = int(row_off[w_ * ppw]), int(row_off[(w_ + 1) * ppw])
            got = to_arrow(em["views"][r0:r1], None, em["bytes"][w_], binary=True)
            got.validate(full=True)
            assert got.cast(pa.binary()).equals(arr.cast(pa.binary()).slice(r0, r1 - r0))
            wl = lens[r0:r1]
            assert len(em["bytes"][w_]) == int(wl[wl > 12].sum())
            # any row slice of a window + the window's buffer is a valid view array
            part = to_arrow(em["views"][r0 + 3:r1], None, em["bytes"][w_], binary=True)
            part.validate(full=True)
    with pytest.raises(ValueError):
        emit_ref(lens, None, data, row_off, byte_off, 3)
    with pytest.raises(ValueError):
        emit_ref(lens, None, data, row_off, byte_off, 0)


def test_new_exports_guard_without_a_device():
    L = api.lib()
    out = ctypes.c_void_p()
    INVALID = 1
    assert L.dd_view_ingest_run(None, None, ctypes.c_int64(4), None, None, 0, None,
                                ctypes.byref(out)) == INVALID
    assert L.dd_last_error() != b""
    assert L.dd_view_ingest_run(None, None, ctypes.c_int64(0), None, None, 0, None,
                                None) == INVALID
    assert L.dd_view_ingest_run(None, None, ctypes.c_int64(-1), None, None, 0, None,
                                ctypes.byref(out)) == INVALID
    assert L.dd_view_ingest_run(None, None, ctypes.c_int64(0), None, None, 2, None,
                                ctypes.byref(out)) == INVALID
    # misaligned views
    assert L.dd_view_ingest_run(ctypes.c_void_p(0x1008), None, ctypes.c_int64(1), None,
                                None, 0, None, ctypes.byref(out)) == INVALID
    assert L.dd_view_emit_run(None, 0, 1, None, ctypes.byref(out)) == INVALID
    ms = (ctypes.c_float * 3)()
    assert L.dd_view_ingest_kernel_ms(None, ms) == INVALID
    assert L.dd_view_emit_kernel_ms(None, ms) == INVALID
    assert L.dd_view_emit_counts(None, None) == INVALID
    assert api.view_tile_rows() > 0 and api.view_tile_rows() % 64 == 0
    assert 0 < api.view_image_bytes() < 160 * 1024


def test_partition_batches_refuses_a_mismatched_view_emit():
    class Part:
        nparts = 8

    class Emit:
        n_windows = 4  # not one window per partition
        col = 0

    part = Part()
    Emit.part = part
    with pytest.raises(ValueError, match="ViewEmit"):
        next(arrow_boundary.partition_batches(part, 0, 8, views={0: Emit()}))


def test_utf8view_batch_refuses_refill(monkeypatch):
    """A batch holding a view column cannot be refilled (re-ingest is out of scope); the
    refusal comes before anything is copied."""
    addr = iter(range(0x1000, 0x100000, 0x1000))
    monkeypatch.setattr(api.DeviceBatch, "_up", lambda self, arr: next(addr))

    class FakeIngest:
        def __init__(self, *a, **k):
            self.bytes_ptr, self.offsets_ptr, self.data_len = 0x10, 0x20, 5

        def destroy(self):
            pass

    monkeypatch.setattr(api, "ViewIngest", FakeIngest)
    views, valid, bufs = from_arrow(pa.array(["ab", None, "cde"], type=pa.string_view()))
    cols = [{"dtype": "utf8view", "views": views, "bufs": bufs, "valid": valid},
            {"dtype": "i64", "data": np.arange(3, dtype=np.int64), "valid": None}]
    batch = api.DeviceBatch(cols)
    assert batch.n_rows == 3
    assert batch.desc.cols[0].dtype == api.DTYPE_CODE["utf8"] and batch.desc.cols[0].validity
    assert batch._utf8_maxlen[0] == 3
    assert ctypes.sizeof(api.ColDesc) == 64 and "utf8view" not in api.DTYPE_CODE
    with pytest.raises(ValueError, match="utf8view"):
        batch.refill(cols)
