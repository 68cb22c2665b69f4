"""api.py — ctypes binding to libdd_shuffle.so (the C ABI, include/dd_shuffle.h).

Harness layer only: uploads/downloads numpy-described Arrow columns (the column-dict
convention of oracle/pyref.py) to device memory and drives the C ABI. The compute path is
entirely inside libdd_shuffle.so; there is NO CPU fallback here — calls on a GPU-less box
raise DDError(DD_ERR_NO_DEVICE), by design.
"""

import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libdd_shuffle.so")

DD_OK = 0
STATUS_NAMES = {
    0: "DD_OK", 1: "DD_ERR_INVALID", 2: "DD_ERR_NO_DEVICE", 3: "DD_ERR_HIP",
    4: "DD_ERR_RCCL", 5: "DD_ERR_NOT_FOUND", 6: "DD_ERR_UNSUPPORTED",
}

DTYPE_CODE = {"u8": 1, "i16": 2, "i32": 3, "i64": 4, "f32": 5, "f64": 6,
              "bool": 7, "utf8": 8, "dict32": 9, "dec128": 10}
# dec128: one value is two u64 words [lo, hi]; host arrays are (n, 2)
FIXED_NP = {"u8": np.uint8, "bool": np.uint8, "i16": np.int16, "i32": np.int32,
            "f32": np.float32, "i64": np.int64, "f64": np.float64, "dict32": np.int32,
            "dec128": np.uint64}
ELEM_SIZE = {"u8": 1, "bool": 1, "i16": 2, "i32": 4, "f32": 4, "i64": 8, "f64": 8,
             "dict32": 4, "dec128": 16}

DD_MAX_COLS = 24
UNIQUE_ID_BYTES = 128


class DDError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class ColDesc(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("data", ctypes.c_void_p),
        ("validity", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("data_len", ctypes.c_int64),
        ("dict_bytes", ctypes.c_void_p),
        ("dict_offsets", ctypes.c_void_p),
        ("dict_n", ctypes.c_int64),
    ]


class BatchDesc(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("n_cols", ctypes.c_int32),
        ("cols", ColDesc * DD_MAX_COLS),
    ]


class TaskKeyC(ctypes.Structure):
    _fields_ = [
        ("query_id_hi", ctypes.c_uint64),
        ("query_id_lo", ctypes.c_uint64),
        ("stage_id", ctypes.c_uint64),
        ("task_number", ctypes.c_uint64),
    ]


class PartitionerInfo(ctypes.Structure):
    """dd_partitioner_info (include/dd_shuffle.h)."""
    _fields_ = [
        ("path", ctypes.c_int32),
        ("wpb", ctypes.c_int32),
        ("gmax", ctypes.c_int32),
        ("hl", ctypes.c_int32),
        ("rhash", ctypes.c_int32),
        ("pid_elem", ctypes.c_int32),
        ("k5", ctypes.c_int32),
        ("k5_wpb", ctypes.c_int32),
        ("k5_maxlen", ctypes.c_int32),
        ("rpb", ctypes.c_int32),
        ("round_rows", ctypes.c_int64),
        ("n_launch", ctypes.c_int64),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise FileNotFoundError(
                f"{_SO} missing — build it with __graft_entry__.build(); the product path "
                "has no fallback")
        L = ctypes.CDLL(_SO)
        L.dd_last_error.restype = ctypes.c_char_p
        L.dd_version.restype = ctypes.c_char_p
        L.dd_device_count.restype = ctypes.c_int
        L.dd_partitioner_pids.restype = ctypes.c_void_p
        L.dd_partitioner_col_data.restype = ctypes.c_void_p
        L.dd_partitioner_col_validity.restype = ctypes.c_void_p
        L.dd_partitioner_col_lengths.restype = ctypes.c_void_p
        L.dd_partitioner_var_offsets64.restype = ctypes.c_void_p
        L.dd_exchanged_col_data.restype = ctypes.c_void_p
        L.dd_exchanged_col_validity.restype = ctypes.c_void_p
        L.dd_exchanged_col_lengths.restype = ctypes.c_void_p
        L.dd_exchanged_total_rows.restype = ctypes.c_int64
        L.dd_pre_xcd_block_map.restype = None
        L.dd_pre_xcd_block_map.argtypes = [ctypes.c_int64, ctypes.c_void_p]
        L.dd_bcast_n_rows.restype = ctypes.c_int64
        L.dd_bcast_n_cols.restype = ctypes.c_int32
        L.dd_bcast_col_data.restype = ctypes.c_void_p
        L.dd_bcast_col_validity.restype = ctypes.c_void_p
        L.dd_bcast_col_offsets.restype = ctypes.c_void_p
        L.dd_reducer_n_rows.restype = ctypes.c_int64
        L.dd_reducer_kernel_ms.restype = ctypes.c_float
        L.dd_reducer_kernel.restype = ctypes.c_int32
        L.dd_reducer_waveagg.restype = ctypes.c_int32
        L.dd_finalizer_n_groups.restype = ctypes.c_int64
        L.dd_finalizer_destroy.restype = None
        L.dd_finalizer_destroy.argtypes = [ctypes.c_void_p]
        L.dd_joiner_n_rows.restype = ctypes.c_int64
        L.dd_joiner_n_rows.argtypes = [ctypes.c_void_p]
        L.dd_joiner_n_segs.restype = ctypes.c_int32
        L.dd_joiner_n_segs.argtypes = [ctypes.c_void_p]
        for fn in (L.dd_joiner_build_idx, L.dd_joiner_probe_idx):
            fn.restype = ctypes.c_void_p
            fn.argtypes = [ctypes.c_void_p]
        for fn in (L.dd_joiner_col_data, L.dd_joiner_col_validity):
            fn.restype = ctypes.c_void_p
            fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.dd_joiner_destroy.restype = None
        L.dd_joiner_destroy.argtypes = [ctypes.c_void_p]
        L.dd_finalizer_n_cols.restype = ctypes.c_int32
        L.dd_finalizer_n_cols.argtypes = [ctypes.c_void_p]
        L.dd_finalizer_col_dtype.restype = ctypes.c_int32
        L.dd_finalizer_col_dtype.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.dd_sorter_n_rows.restype = ctypes.c_int64
        L.dd_sorter_n_rows.argtypes = [ctypes.c_void_p]
        L.dd_sorter_perm.restype = ctypes.c_void_p
        L.dd_sorter_perm.argtypes = [ctypes.c_void_p]
        for fn in (L.dd_finalizer_col_data, L.dd_finalizer_col_validity,
                   L.dd_sorter_col_data, L.dd_sorter_col_validity):
            fn.restype = ctypes.c_void_p
            fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.dd_sorter_destroy.restype = None
        L.dd_sorter_destroy.argtypes = [ctypes.c_void_p]
        L.dd_dict_gc_n_windows.restype = ctypes.c_uint32
        L.dd_dict_gc_indices.restype = ctypes.c_void_p
        L.dd_dict_gc_dict_offsets.restype = ctypes.c_void_p
        L.dd_dict_gc_dict_bytes.restype = ctypes.c_void_p
        L.dd_exchanged_dict_n.restype = ctypes.c_int64
        L.dd_exchanged_dict_offsets.restype = ctypes.c_void_p
        L.dd_exchanged_dict_bytes.restype = ctypes.c_void_p
        L.dd_view_ingest_offsets.restype = ctypes.c_void_p
        L.dd_view_ingest_bytes.restype = ctypes.c_void_p
        L.dd_view_ingest_data_len.restype = ctypes.c_int64
        L.dd_view_ingest_tier.restype = ctypes.c_int32
        L.dd_view_ingest_destroy.restype = None
        L.dd_view_ingest_destroy.argtypes = [ctypes.c_void_p]
        L.dd_view_tile_rows.restype = ctypes.c_int32
        L.dd_view_image_bytes.restype = ctypes.c_int32
        L.dd_view_emit_views.restype = ctypes.c_void_p
        L.dd_view_emit_bytes.restype = ctypes.c_void_p
        L.dd_view_emit_destroy.restype = None
        L.dd_view_emit_destroy.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def _check(st):
    if st != DD_OK:
        raise DDError(st, lib().dd_last_error().decode())


def device_count():
    return lib().dd_device_count()


def _stream_arg(stream):
    """Accept None, a raw int hipStream_t, or a torch.cuda.Stream."""
    if stream is None:
        return None
    h = getattr(stream, "cuda_stream", stream)
    return ctypes.c_void_p(h)


def _dev_alloc(nbytes):
    p = ctypes.c_void_p()
    _check(lib().dd_dev_alloc(ctypes.c_int64(max(nbytes, 1)), ctypes.byref(p)))
    return p


def _h2d(dst, arr):
    arr = np.ascontiguousarray(arr)
    _check(lib().dd_memcpy_h2d(dst, arr.ctypes.data_as(ctypes.c_void_p),
                               ctypes.c_int64(arr.nbytes)))


def _d2h(src_ptr, nbytes, dtype):
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    _check(lib().dd_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p),
                               ctypes.c_void_p(src_ptr), ctypes.c_int64(nbytes)))
    return out


def fixed_host(col):
    """The host array of a fixed-width column dict in its canonical dtype and shape. A
    dec128 column may hold any C-contiguous array of n x 16 bytes; it comes back as u64
    (n, 2) = [lo, hi] without a copy."""
    if col["dtype"] == "dec128":
        data = np.asarray(col["data"])
        if data.dtype != np.uint64 or data.ndim != 2 or not data.flags.c_contiguous:
            if not data.flags.c_contiguous or data.nbytes % 16:
                raise ValueError("dec128 data must be a C-contiguous array of n x 16 bytes")
            data = data.reshape(-1).view(np.uint8).view(np.uint64)
        return data.reshape(-1, 2)
    return np.ascontiguousarray(col["data"], dtype=FIXED_NP[col["dtype"]])


def fixed_out(dtype, flat):
    """Shape a downloaded fixed-width buffer like fixed_host: dec128 -> u64 (n, 2)."""
    return flat.reshape(-1, 2) if dtype == "dec128" else flat


def dec128_col(arr):
    """Column dict of a pyarrow Decimal128Array: the value buffer as u64 (n, 2) = [lo, hi],
    the validity bitmap unpacked to u8 (None when the array has no nulls), and precision and
    scale from the type, which only the Arrow boundary reads back."""
    import pyarrow as pa

    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if not pa.types.is_decimal128(arr.type):
        raise TypeError(f"dec128_col needs a decimal128 array, got {arr.type}")
    n = len(arr)
    bitmap, values = arr.buffers()
    data = np.zeros((0, 2), dtype=np.uint64) if n == 0 else np.frombuffer(
        values, dtype=np.uint64, count=2 * n, offset=16 * arr.offset).reshape(n, 2).copy()
    valid = None
    if arr.null_count:
        bits = np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), bitorder="little")
        valid = np.ascontiguousarray(bits[arr.offset:arr.offset + n])
    return {"dtype": "dec128", "data": data, "valid": valid,
            "precision": arr.type.precision, "scale": arr.type.scale}


class DeviceBatch:
    """Device-resident batch uploaded from the column-dict convention."""

    def __init__(self, cols):
        self.cols = cols
        if cols[0]["dtype"] == "utf8":
            self.n_rows = len(cols[0]["offsets"]) - 1
        elif cols[0]["dtype"] == "utf8view":
            self.n_rows = len(np.asarray(cols[0]["views"], dtype=np.uint8).reshape(-1, 16))
        elif cols[0]["dtype"] == "dec128":
            self.n_rows = len(fixed_host(cols[0]))
        else:
            self.n_rows = len(cols[0]["data"])
        self._bufs = []
        self._host_refs = (None, None)
        self._utf8_maxlen = {}  # col -> longest string uploaded at construction
        self._ingests = {}  # col -> ViewIngest owning a utf8view column's offsets + bytes
        self.desc = BatchDesc()
        self.desc.n_rows = self.n_rows
        self.desc.n_cols = len(cols)
        for i, col in enumerate(cols):
            cd = self.desc.cols[i]
            if col["dtype"] == "utf8view":
                self._ingest_views(i, col, cd)
                continue
            cd.dtype = DTYPE_CODE[col["dtype"]]
            if col["dtype"] == "utf8":
                data = np.ascontiguousarray(col["data"], dtype=np.uint8)
                off = np.ascontiguousarray(col["offsets"], dtype=np.int32)
                b = self._up(data)
                cd.data = b
                cd.offsets = self._up(off)
                cd.data_len = int(data.nbytes)
                self._utf8_maxlen[i] = int(np.diff(off).max()) if len(off) > 1 else 0
            else:
                data = fixed_host(col)
                if col["dtype"] == "dec128" and len(data) != self.n_rows:
                    raise ValueError(f"column {i} has {len(data)} rows, batch has "
                                     f"{self.n_rows}")
                cd.data = self._up(data)
                cd.data_len = 0
            if col.get("valid") is not None:
                cd.validity = self._up(np.ascontiguousarray(col["valid"], np.uint8))
            if col["dtype"] == "dict32":
                cd.dict_bytes = self._up(np.ascontiguousarray(col["dict_bytes"], np.uint8))
                cd.dict_offsets = self._up(np.ascontiguousarray(col["dict_offsets"], np.int32))
                cd.dict_n = len(col["dict_offsets"]) - 1

    def _ingest_views(self, i, col, cd):
        """Upload a {"dtype": "utf8view", "views", "bufs", "valid"} column, run the view
        ingest on it and describe the result to C as an ordinary UTF8 column."""
        views = np.ascontiguousarray(col["views"], dtype=np.uint8).reshape(-1, 16)
        if len(views) != self.n_rows:
            raise ValueError(f"column {i} has {len(views)} views, batch has {self.n_rows} rows")
        valid = col.get("valid")
        vp = None
        lens = views.view(np.int32).reshape(-1, 4)[:, 0]
        if valid is not None:
            valid = np.ascontiguousarray(valid, np.uint8)
            vp = self._up(valid)
            lens = lens[valid != 0]
        bufs = [np.ascontiguousarray(b, dtype=np.uint8) for b in col.get("bufs", [])]
        ing = ViewIngest(self._up(views), vp, self.n_rows, [self._up(b) for b in bufs],
                         [int(b.nbytes) for b in bufs])
        self._ingests[i] = ing
        cd.dtype = DTYPE_CODE["utf8"]
        cd.data = ing.bytes_ptr
        cd.offsets = ing.offsets_ptr
        cd.data_len = ing.data_len
        if vp is not None:
            cd.validity = vp
        self._utf8_maxlen[i] = int(lens.max()) if len(lens) else 0

    @classmethod
    def from_device(cls, view_cols, n_rows):
        """Non-owning device-view batch: each col gives raw device pointers
        ({"dtype", "data_ptr", "valid_ptr", "offsets_ptr", "data_len", dict...}).
        Used by the two-level scatter to re-consume pass-A bucket slices without
        copies."""
        self = cls.__new__(cls)
        self.cols = view_cols
        self.n_rows = n_rows
        self._bufs = []
        self._host_refs = (None, None)
        self._utf8_maxlen = {}
        self._ingests = {}
        self.desc = BatchDesc()
        self.desc.n_rows = n_rows
        self.desc.n_cols = len(view_cols)
        for i, col in enumerate(view_cols):
            cd = self.desc.cols[i]
            cd.dtype = DTYPE_CODE[col["dtype"]]
            cd.data = col["data_ptr"]
            cd.data_len = int(col.get("data_len", 0))
            if col.get("valid_ptr"):
                cd.validity = col["valid_ptr"]
            if col.get("offsets_ptr"):
                cd.offsets = col["offsets_ptr"]
            if col.get("dict_bytes_ptr"):
                cd.dict_bytes = col["dict_bytes_ptr"]
                cd.dict_offsets = col["dict_offsets_ptr"]
                cd.dict_n = col["dict_n"]
        return self

    def _up(self, arr):
        p = _dev_alloc(arr.nbytes)
        _h2d(p, arr)
        self._bufs.append(p)
        return p.value

    def _refill_plan(self, cols):
        """Validate `cols` against this batch under the partitioner reuse contract
        (dd_shuffle.h, above dd_partitioner_run) and return the (device pointer, host
        array) copies a refill would make. Raises ValueError on the first mismatch;
        touches neither the device nor the library."""
        if self._ingests:
            raise ValueError(f"refill: column {min(self._ingests)} is a utf8view column "
                             "(re-ingest into a live batch is not supported)")
        if len(cols) != self.desc.n_cols:
            raise ValueError(f"refill: {len(cols)} columns, batch has {self.desc.n_cols}")
        n = self.n_rows
        plan = []
        for i, col in enumerate(cols):
            cd = self.desc.cols[i]
            old = self.cols[i]
            if DTYPE_CODE.get(col["dtype"]) != cd.dtype:
                raise ValueError(f"refill: column {i} dtype {col['dtype']} differs")
            if col["dtype"] == "utf8":
                data = np.ascontiguousarray(col["data"], dtype=np.uint8)
                off = np.ascontiguousarray(col["offsets"], dtype=np.int32)
                if len(off) != n + 1:
                    raise ValueError(f"refill: column {i} has {len(off) - 1} rows, "
                                     f"batch has {n}")
                if int(data.nbytes) != cd.data_len or int(off[-1]) != cd.data_len or \
                        int(off[0]) != 0:
                    raise ValueError(f"refill: column {i} utf8 byte total differs from "
                                     f"{cd.data_len}")
                lens = np.diff(off)
                if n and int(lens.min()) < 0:
                    raise ValueError(f"refill: column {i} offsets decrease")
                # longest string the batch has ever held == what a partitioner created
                # on it may have sized its LDS image from
                longest = self._utf8_maxlen.get(i)
                if longest is None:
                    raise ValueError(f"refill: column {i} create-time string lengths "
                                     "unknown (device-view batch)")
                if n and int(lens.max()) > longest:
                    raise ValueError(f"refill: column {i} has a string longer than "
                                     f"{longest} bytes")
                plan += [(cd.data, data), (cd.offsets, off)]
            else:
                data = fixed_host(col)
                if len(data) != n:
                    raise ValueError(f"refill: column {i} has {len(data)} rows, "
                                     f"batch has {n}")
                plan.append((cd.data, data))
            valid = col.get("valid")
            if (valid is not None) != bool(cd.validity):
                raise ValueError(f"refill: column {i} validity presence differs")
            if valid is not None:
                valid = np.ascontiguousarray(valid, dtype=np.uint8)
                if len(valid) != n:
                    raise ValueError(f"refill: column {i} validity length differs")
                plan.append((cd.validity, valid))
            if col["dtype"] == "dict32":
                same = "dict_offsets" in old and \
                    np.array_equal(np.asarray(col["dict_offsets"], dtype=np.int32),
                                   np.asarray(old["dict_offsets"], dtype=np.int32)) and \
                    np.array_equal(np.asarray(col["dict_bytes"], dtype=np.uint8),
                                   np.asarray(old["dict_bytes"], dtype=np.uint8))
                if not same:
                    raise ValueError(f"refill: column {i} dictionary differs (dict32 key "
                                     "hashes are computed at partitioner create time)")
                live = data if valid is None else data[valid != 0]
                if len(live) and (int(live.min()) < 0 or int(live.max()) >= cd.dict_n):
                    raise ValueError(f"refill: column {i} has an index outside the "
                                     "dictionary")
        return plan

    def refill(self, cols, stream=None):
        """Upload new host columns into the EXISTING device buffers, for re-running a
        partitioner created on this batch (reuse contract: dd_shuffle.h). Same dtypes,
        n_rows and validity presence; utf8: same byte total and no string longer than
        the longest this batch started with; dict32: the same dictionary. Any mismatch
        raises ValueError before anything is copied.

        stream=None copies synchronously. With a stream the copies are queued on it
        (dd_memcpy_h2d_async): they overlap other streams when the arrays are pinned host
        memory, and the caller keeps `cols` alive and unchanged until the stream has
        passed them. Ordering against the previous run (wait_phase2) is the caller's."""
        plan = self._refill_plan(cols)
        for dst, arr in plan:
            if arr.nbytes == 0:
                continue
            if stream is None:
                _h2d(ctypes.c_void_p(dst), arr)
            else:
                _check(lib().dd_memcpy_h2d_async(
                    ctypes.c_void_p(dst), arr.ctypes.data_as(ctypes.c_void_p),
                    ctypes.c_int64(arr.nbytes), _stream_arg(stream)))
        # converted temporaries of this refill and the one before stay alive
        self._host_refs = (self._host_refs[1], [arr for _, arr in plan])
        self.cols = cols

    def free(self):
        for ing in self._ingests.values():
            ing.destroy()
        self._ingests = {}
        for b in self._bufs:
            lib().dd_dev_free(b)
        self._bufs = []


class Partitioner:
    """Wraps dd_partitioner_*: the producer-head replacement."""

    def __init__(self, batch: DeviceBatch, key_idx, nparts, ranged=None):
        """ranged=(pid_total, coarse_div): coarse-bucket mode — nparts is then
        pid_total // coarse_div contiguous ranges (dd_partitioner_create_ranged)."""
        self.batch = batch
        self.key_idx = list(key_idx)
        keys = (ctypes.c_int32 * len(key_idx))(*key_idx)
        self.h = ctypes.c_void_p()
        if ranged is None:
            self.nparts = nparts
            _check(lib().dd_partitioner_create(ctypes.byref(batch.desc), keys,
                                               len(key_idx), ctypes.c_uint32(nparts),
                                               ctypes.byref(self.h)))
        else:
            total, div = ranged
            self.nparts = total // div
            _check(lib().dd_partitioner_create_ranged(
                ctypes.byref(batch.desc), keys, len(key_idx), ctypes.c_uint32(total),
                ctypes.c_uint32(div), ctypes.byref(self.h)))

    def run(self, stream=None):
        _check(lib().dd_partitioner_run(self.h, _stream_arg(stream)))

    def run_phase1(self, stream=None):
        """K1 hash+count + K2 scans (batch-pipelining split; see dd_shuffle.h)."""
        _check(lib().dd_partitioner_run_phase1(self.h, _stream_arg(stream)))

    def run_phase2(self, stream=None):
        """K3 scatter (+K4 var bytes)."""
        _check(lib().dd_partitioner_run_phase2(self.h, _stream_arg(stream)))

    def wait_phase1(self, stream):
        _check(lib().dd_partitioner_wait_phase1(self.h, _stream_arg(stream)))

    def wait_phase2(self, stream):
        _check(lib().dd_partitioner_wait_phase2(self.h, _stream_arg(stream)))

    def sync(self):
        _check(lib().dd_device_sync())

    def info(self):
        """The plan dd_partitioner_create chose, as a dict of dd_partitioner_info's
        fields (path 0 v1 / 1 staged / 2 pre, wpb, gmax, hl, rhash, pid_elem, k5, k5_wpb,
        k5_maxlen, rpb, round_rows, n_launch). Needs no run."""
        out = PartitionerInfo()
        _check(lib().dd_partitioner_get_info(self.h, ctypes.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in PartitionerInfo._fields_}

    def pre_layout(self):
        """0 not the pre path, 1 segment-granular layout precompute, 2 round-granular
        (dd_partitioner_pre_layout; DD_PRE_LAYOUT=seg|round at create time)."""
        return int(lib().dd_partitioner_pre_layout(self.h))

    def pre_wide(self):
        """1 when the pre path scatters in wide rounds (8192 rows in two column passes;
        info() then reports gmax 8 / round_rows 8192), else 0 (dd_partitioner_pre_wide;
        DD_PRE_WIDE=0|1 and DD_PRE_WIDE_MIN_ROWS at create time)."""
        return int(lib().dd_partitioner_pre_wide(self.h))

    def k1_spec(self):
        """Key-signature code of the K1 hash/count kernel: 0 = generic run-time key loop,
        else kind(key 0) | kind(key 1) << 4 (dd_partitioner_k1_spec; DD_K1_SPEC=0 at
        create time forces 0)."""
        return int(lib().dd_partitioner_k1_spec(self.h))

    def has_pid_array(self):
        """Fast null-check of the device pid pointer (no download): False when the spec
        path recomputes hashes in-kernel (rhash) and no pid array exists."""
        return bool(lib().dd_partitioner_pids(self.h))

    def pids(self):
        """Per-row partition ids (u32; widened from u8 when the precomputed-layout path
        stores byte pids), or None when the spec path recomputed hashes in-kernel (no
        pid array exists; outputs + row_offsets fully define the partitioning)."""
        p = lib().dd_partitioner_pids(self.h)
        if not p:
            return None
        if lib().dd_partitioner_pid_elem(self.h) == 1:
            return _d2h(p, self.batch.n_rows, np.uint8).astype(np.uint32)
        return _d2h(p, self.batch.n_rows * 4, np.uint32)

    def row_offsets(self):
        out = np.empty(self.nparts + 1, dtype=np.int64)
        _check(lib().dd_partitioner_row_offsets(
            self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def byte_offsets(self, col):
        out = np.empty(self.nparts + 1, dtype=np.int64)
        _check(lib().dd_partitioner_byte_offsets(
            self.h, col, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def var_offsets64(self, col):
        """Download the rebuilt Arrow offsets u64[n_rows+1] of utf8 column `col` in
        partition-major order, zero-based (dd_partitioner_var_offsets64, the K4c output), or
        None on the v1 path, which keeps lengths only (tests only)."""
        p = lib().dd_partitioner_var_offsets64(self.h, ctypes.c_int32(col))
        if not p:
            return None
        return _d2h(p, (self.batch.n_rows + 1) * 8, np.uint64)

    def kernel_ms(self):
        out = (ctypes.c_float * 3)()
        _check(lib().dd_partitioner_kernel_ms(self.h, out))
        return list(out)

    def col_out(self, i):
        """Download partitioned output of column i (tests/smoke only)."""
        col = self.batch.cols[i]
        n = self.batch.n_rows
        res = {"dtype": col["dtype"]}
        if col["dtype"] in ("utf8", "utf8view"):
            # a view column was ingested to utf8: it comes out in the usual utf8 shape
            res["dtype"] = "utf8"
            dl = (self.batch._ingests[i].data_len if col["dtype"] == "utf8view"
                  else int(np.asarray(col["data"], dtype=np.uint8).nbytes))
            res["data"] = _d2h(lib().dd_partitioner_col_data(self.h, i), dl, np.uint8)
            res["lengths"] = _d2h(lib().dd_partitioner_col_lengths(self.h, i), n * 4,
                                  np.uint32)
        else:
            npdt = FIXED_NP[col["dtype"]]
            res["data"] = fixed_out(col["dtype"],
                                    _d2h(lib().dd_partitioner_col_data(self.h, i),
                                         n * ELEM_SIZE[col["dtype"]], npdt))
        vp = lib().dd_partitioner_col_validity(self.h, i)
        if vp:
            res["valid"] = _d2h(vp, n, np.uint8)
        return res

    def destroy(self):
        if self.h:
            lib().dd_partitioner_destroy(self.h)
            self.h = None


class DictGC:
    """Per-window dictionary GC of one dict32 column of a run Partitioner (dd_dict_gc_*,
    DESIGN.md §14): window-local indices plus one compacted dictionary per window. The
    partitioner's own output is untouched and must outlive this object."""

    def __init__(self, part: Partitioner, col: int, n_windows: int, stream=None):
        self.part = part
        self.col = col
        self.n_windows = n_windows
        self.h = ctypes.c_void_p()
        _check(lib().dd_dict_gc_run(part.h, col, ctypes.c_uint32(n_windows),
                                    _stream_arg(stream), ctypes.byref(self.h)))
        self._counts = None

    def counts(self):
        """(val_off, byte_off): host prefix sums i64[n_windows+1] of values / bytes."""
        if self._counts is None:
            v = np.empty(self.n_windows + 1, dtype=np.int64)
            b = np.empty(self.n_windows + 1, dtype=np.int64)
            _check(lib().dd_dict_gc_counts(
                self.h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                b.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            self._counts = (v, b)
        return self._counts

    def indices(self):
        """Download the remapped i32[n_rows] indices (0 for null rows)."""
        return _d2h(lib().dd_dict_gc_indices(self.h), self.part.batch.n_rows * 4, np.int32)

    def window_dict(self, w):
        """Download window w's compacted dictionary: (offsets i32[nvals+1], bytes u8)."""
        v, b = self.counts()
        nv, nb = int(v[w + 1] - v[w]), int(b[w + 1] - b[w])
        off = _d2h(lib().dd_dict_gc_dict_offsets(self.h) + (int(v[w]) + w) * 4,
                   (nv + 1) * 4, np.int32)
        data = (_d2h(lib().dd_dict_gc_dict_bytes(self.h) + int(b[w]), nb, np.uint8)
                if nb else np.zeros(0, dtype=np.uint8))
        return off, data

    def kernel_ms(self):
        """[mark, rank, compact, remap] hipEvent durations of the run, in ms."""
        out = (ctypes.c_float * 4)()
        _check(lib().dd_dict_gc_kernel_ms(self.h, out))
        return list(out)

    def destroy(self):
        if self.h:
            lib().dd_dict_gc_destroy(self.h)
            self.h = None


class ViewIngest:
    """dd_view_ingest_*: Arrow views + their data buffers -> a dense utf8 column (i32
    offsets + bytes) on the device. Takes raw device pointers; from_host
    uploads numpy arrays first and owns those uploads."""

    def __init__(self, views_ptr, valid_ptr, n_rows, buf_ptrs, buf_lens, stream=None):
        nb = len(buf_ptrs)
        ptrs = (ctypes.c_void_p * max(nb, 1))(*buf_ptrs)
        lens = (ctypes.c_int64 * max(nb, 1))(*buf_lens)
        self.n_rows = n_rows
        self._owned = []
        self.h = ctypes.c_void_p()
        _check(lib().dd_view_ingest_run(
            ctypes.c_void_p(views_ptr), ctypes.c_void_p(valid_ptr), ctypes.c_int64(n_rows),
            ptrs, lens, ctypes.c_int32(nb), _stream_arg(stream), ctypes.byref(self.h)))
        self.data_len = int(lib().dd_view_ingest_data_len(self.h))
        self.offsets_ptr = lib().dd_view_ingest_offsets(self.h)
        self.bytes_ptr = lib().dd_view_ingest_bytes(self.h)

    @classmethod
    def from_host(cls, views, valid, bufs, buf_lens=None, stream=None):
        """Upload views u8[n,16], valid u8[n] or None and the data buffers, then ingest.
        buf_lens overrides the lengths stated to the library (default: the arrays')."""
        owned = []

        def up(arr):
            arr = np.ascontiguousarray(arr, dtype=np.uint8)
            p = _dev_alloc(arr.nbytes)
            if arr.nbytes:
                _h2d(p, arr)
            owned.append(p)
            return p.value

        try:
            views = np.ascontiguousarray(views, dtype=np.uint8).reshape(-1, 16)
            vp = up(views)
            validp = up(valid) if valid is not None else None
            ptrs = [up(b) for b in bufs]
            if buf_lens is None:
                buf_lens = [int(np.asarray(b).nbytes) for b in bufs]
            self = cls(vp, validp, len(views), ptrs, buf_lens, stream)
        except Exception:
            for p in owned:
                lib().dd_dev_free(p)
            raise
        self._owned = owned
        return self

    def tier(self):
        """1 = LDS-staged copy (DD_VIEW_LDS=1), 0 = direct (the default, or every tile
        outgrew the image)."""
        return int(lib().dd_view_ingest_tier(self.h))

    def offsets(self):
        return _d2h(self.offsets_ptr, (self.n_rows + 1) * 4, np.int32)

    def bytes(self):
        return (_d2h(self.bytes_ptr, self.data_len, np.uint8) if self.data_len
                else np.zeros(0, dtype=np.uint8))

    def kernel_ms(self):
        """[length pass, scan, copy] hipEvent durations of the run, in ms."""
        out = (ctypes.c_float * 3)()
        _check(lib().dd_view_ingest_kernel_ms(self.h, out))
        return list(out)

    def destroy(self):
        if self.h:
            lib().dd_view_ingest_destroy(self.h)
            self.h = None
        for p in self._owned:
            lib().dd_dev_free(p)
        self._owned = []


def view_tile_rows():
    """Rows per copy tile of the view kernels (dd_view_tile_rows; needs no device)."""
    return int(lib().dd_view_tile_rows())


def view_image_bytes():
    """Bytes of the LDS image of the staged copy tier (dd_view_image_bytes)."""
    return int(lib().dd_view_image_bytes())


class ViewEmit:
    """dd_view_emit_*: one utf8 column of a run Partitioner as compact per-window Arrow
    view arrays: 16-byte views, partition-major, plus one data buffer per
    window holding only the long values. The partitioner's own output is untouched and
    must outlive this object."""

    def __init__(self, part: Partitioner, col: int, n_windows: int, stream=None):
        self.part = part
        self.col = col
        self.n_windows = n_windows
        self.h = ctypes.c_void_p()
        _check(lib().dd_view_emit_run(part.h, col, ctypes.c_uint32(n_windows),
                                      _stream_arg(stream), ctypes.byref(self.h)))
        self._counts = None

    def counts(self):
        """long_byte_off: host prefix sums i64[n_windows+1] of the windows' buffers."""
        if self._counts is None:
            b = np.empty(self.n_windows + 1, dtype=np.int64)
            _check(lib().dd_view_emit_counts(
                self.h, b.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            self._counts = b
        return self._counts

    def views(self):
        """Download the u8[n_rows, 16] views."""
        n = self.part.batch.n_rows
        if n == 0:
            return np.zeros((0, 16), dtype=np.uint8)
        return _d2h(lib().dd_view_emit_views(self.h), n * 16, np.uint8).reshape(n, 16)

    def window_bytes(self, w):
        """Download window w's data buffer."""
        b = self.counts()
        nb = int(b[w + 1] - b[w])
        if nb == 0:
            return np.zeros(0, dtype=np.uint8)
        return _d2h(lib().dd_view_emit_bytes(self.h) + int(b[w]), nb, np.uint8)

    def kernel_ms(self):
        """[scan, build, copy] hipEvent durations of the run, in ms."""
        out = (ctypes.c_float * 3)()
        _check(lib().dd_view_emit_kernel_ms(self.h, out))
        return list(out)

    def destroy(self):
        if self.h:
            lib().dd_view_emit_destroy(self.h)
            self.h = None


class Comm:
    """RCCL communicator (dd_comm_*)."""

    def __init__(self, unique_id: bytes, rank: int, nranks: int):
        assert len(unique_id) == UNIQUE_ID_BYTES
        self.rank, self.nranks = rank, nranks
        self.h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        _check(lib().dd_comm_init(buf, rank, nranks, ctypes.byref(self.h)))

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(lib().dd_comm_unique_id(buf))
        return buf.raw

    def exchange(self, part: Partitioner, stream=None, gc=None):
        """gc: a list of DictGC (n_windows == nranks) routes to dd_exchange_run_gc — those
        columns cross with their compacted dictionaries (Exchanged.col_dict)."""
        h = ctypes.c_void_p()
        if gc is None:
            _check(lib().dd_exchange_run(self.h, part.h, _stream_arg(stream),
                                         ctypes.byref(h)))
        else:
            gcs = (ctypes.c_void_p * max(len(gc), 1))(*[g.h.value for g in gc])
            _check(lib().dd_exchange_run_gc(self.h, part.h, gcs, len(gc),
                                            _stream_arg(stream), ctypes.byref(h)))
        return Exchanged(h, part, self)

    def coalesce(self, part: Partitioner, consumer_tasks: int, stream=None):
        """NetworkCoalesceExec data plane (dd_coalesce_run): this consumer rank receives
        the whole partitioned output of every producer rank in its contiguous group."""
        h = ctypes.c_void_p()
        _check(lib().dd_coalesce_run(self.h, part.h, consumer_tasks,
                                     _stream_arg(stream), ctypes.byref(h)))
        ex = Exchanged(h, part, self)
        return ex

    def broadcast(self, batch, root=0, stream=None):
        """Replicate the root's device batch on every rank (dd_broadcast_run: the
        BroadcastExec/NetworkBroadcastExec data plane)."""
        h = ctypes.c_void_p()
        desc = ctypes.byref(batch.desc) if batch is not None else None
        _check(lib().dd_broadcast_run(self.h, desc, root, _stream_arg(stream),
                                      ctypes.byref(h)))
        return Broadcasted(h)

    def destroy(self):
        if self.h:
            lib().dd_comm_destroy(self.h)
            self.h = None


class Broadcasted:
    def __init__(self, h):
        self.h = h

    @property
    def n_rows(self):
        return lib().dd_bcast_n_rows(self.h)

    @property
    def n_cols(self):
        return lib().dd_bcast_n_cols(self.h)

    def col(self, i):
        dtype = ctypes.c_int32()
        dlen = ctypes.c_int64()
        _check(lib().dd_bcast_col_meta(self.h, i, ctypes.byref(dtype),
                                       ctypes.byref(dlen)))
        name = {v: k for k, v in DTYPE_CODE.items()}[dtype.value]
        n = self.n_rows
        out = {"dtype": name}
        if name == "utf8":
            out["data"] = _d2h(lib().dd_bcast_col_data(self.h, i), int(dlen.value), np.uint8)
            out["offsets"] = _d2h(lib().dd_bcast_col_offsets(self.h, i), (n + 1) * 4,
                                  np.int32)
        else:
            out["data"] = fixed_out(name, _d2h(lib().dd_bcast_col_data(self.h, i),
                                               int(dlen.value), FIXED_NP[name]))
        vp = lib().dd_bcast_col_validity(self.h, i)
        if vp:
            out["valid"] = _d2h(vp, n, np.uint8)
        return out

    def destroy(self):
        if self.h:
            lib().dd_bcast_destroy(self.h)
            self.h = None


class Exchanged:
    def __init__(self, h, part, comm):
        self.h = h
        self.part = part
        self.comm = comm

    @property
    def total_rows(self):
        return lib().dd_exchanged_total_rows(self.h)

    def row_counts(self, producers=None, parts=None):
        """Per-(producer, partition) row counts. Defaults fit dd_exchange_run's window
        shape; pass producers/parts explicitly for dd_coalesce_run results (group size,
        full P)."""
        producers = self.comm.nranks if producers is None else producers
        parts = (self.part.nparts // self.comm.nranks) if parts is None else parts
        out = np.empty(max(producers * parts, 1), dtype=np.int64)
        _check(lib().dd_exchanged_row_counts(
            self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out.reshape(max(producers, 1), -1)

    def byte_counts(self, col):
        out = np.empty(self.comm.nranks * (self.part.nparts // self.comm.nranks),
                       dtype=np.int64)
        _check(lib().dd_exchanged_byte_counts(
            self.h, col, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out.reshape(self.comm.nranks, -1)

    def col_data(self, i):
        col = self.part.batch.cols[i]
        n = self.total_rows
        if col["dtype"] in ("utf8", "utf8view"):
            total_b = int(self.byte_counts(i).sum())
            data = _d2h(lib().dd_exchanged_col_data(self.h, i), total_b, np.uint8)
            lens = _d2h(lib().dd_exchanged_col_lengths(self.h, i), n * 4, np.uint32)
            return {"dtype": "utf8", "data": data, "lengths": lens}
        npdt = FIXED_NP[col["dtype"]]
        return {"dtype": col["dtype"],
                "data": fixed_out(col["dtype"],
                                  _d2h(lib().dd_exchanged_col_data(self.h, i),
                                       n * ELEM_SIZE[col["dtype"]], npdt))}

    def col_validity(self, i):
        vp = lib().dd_exchanged_col_validity(self.h, i)
        return _d2h(vp, self.total_rows, np.uint8) if vp else None

    def col_dict(self, i):
        """Received dictionary of a GC'd dict32 column (its col_data holds the rebased
        indices): {"offsets": i32[dict_n+1], "bytes": u8, "vals_per_producer": i64}."""
        vpp = np.empty(self.comm.nranks, dtype=np.int64)
        _check(lib().dd_exchanged_dict_counts(
            self.h, i, vpp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        dn = int(lib().dd_exchanged_dict_n(self.h, i))
        off = _d2h(lib().dd_exchanged_dict_offsets(self.h, i), (dn + 1) * 4, np.int32)
        nb = int(off[-1])
        data = (_d2h(lib().dd_exchanged_dict_bytes(self.h, i), nb, np.uint8)
                if nb else np.zeros(0, dtype=np.uint8))
        return {"offsets": off, "bytes": data, "vals_per_producer": vpp}

    def stats(self):
        ms = ctypes.c_float()
        eg = ctypes.c_int64()
        _check(lib().dd_exchanged_stats(self.h, ctypes.byref(ms), ctypes.byref(eg)))
        return float(ms.value), int(eg.value)

    def destroy(self):
        if self.h:
            lib().dd_exchanged_destroy(self.h)
            self.h = None


AGG_OPS = {"sum_f64": 0, "count": 1, "sum_i64": 2, "min_f64": 3, "max_f64": 4,
           "min_i64": 5, "max_i64": 6, "sum_dec128": 7}


def partial_reduce_geometry(n_rows):
    """Launch geometry partial_reduce uses for an n_rows batch whose plan has at most 4
    aggregates and no sum_dec128 (no device needed):
    {"table_slots", "probe_limit", "nblocks", "chunk_rows"}."""
    slots = ctypes.c_int32()
    probe = ctypes.c_int32()
    nblocks = ctypes.c_int64()
    chunk = ctypes.c_int64()
    _check(lib().dd_partial_reduce_geometry(
        ctypes.c_int64(n_rows), ctypes.byref(slots), ctypes.byref(probe),
        ctypes.byref(nblocks), ctypes.byref(chunk)))
    return {"table_slots": int(slots.value), "probe_limit": int(probe.value),
            "nblocks": int(nblocks.value), "chunk_rows": int(chunk.value)}


def partial_reduce_plan_geometry(n_rows, n_keys, ops):
    """Launch geometry partial_reduce uses for an n_rows batch under any plan (no device
    needed). ops: the 1..8 op names of the plan. Returns {"kernel": 0 (at most 4 aggregates,
    no sum_dec128: the numbers of partial_reduce_geometry) or 1 (the wide kernel),
    "table_slots", "probe_limit", "block_threads", "lds_bytes", "nblocks", "chunk_rows"}."""
    na = len(ops)
    opsc = (ctypes.c_int32 * max(na, 1))(*[AGG_OPS[o] for o in ops])
    i32 = [ctypes.c_int32() for _ in range(5)]
    nblocks = ctypes.c_int64()
    chunk = ctypes.c_int64()
    _check(lib().dd_partial_reduce_plan_geometry(
        ctypes.c_int64(n_rows), ctypes.c_int32(n_keys), opsc, ctypes.c_int32(na),
        *[ctypes.byref(v) for v in i32], ctypes.byref(nblocks), ctypes.byref(chunk)))
    names = ("kernel", "table_slots", "probe_limit", "block_threads", "lds_bytes")
    geo = {k: int(v.value) for k, v in zip(names, i32)}
    geo["nblocks"] = int(nblocks.value)
    geo["chunk_rows"] = int(chunk.value)
    return geo


def partial_reduce(batch: DeviceBatch, key_idx, aggs):
    """GPU partial aggregation below the shuffle (dd_partial_reduce_run).

    key_idx: 1..4 key columns, fixed-width or dict32 (grouped by dictionary index).
    aggs: 1..8 of (col_index_or_None, op) with op in AGG_OPS: "count" (every row, column
    ignored), "sum_f64", "sum_i64" (wraps mod 2^64), "min_f64"/"max_f64" (IEEE totalOrder
    on the bit pattern: sign-set NaN < -inf < -0.0 < +0.0 < +inf < sign-clear NaN),
    "min_i64"/"max_i64", "sum_dec128" (exact sum of a dec128 column, wraps mod 2^128).
    Every op but count skips NULL inputs.
    Returns {"keys": u64[n, nk] canonical bits (0 for a NULL key component), "keynull":
    u32[n] per-key null bitmask, "aggs": f64[n, na], "nn": u64[n, na] non-null input
    counts, "aggs_hi": u64[n, na], "kernel": 0 or 1, "waveagg": 0 or 1} — integer
    aggregates (count / sum_i64 / min_i64 / max_i64) are bit-cast in the f64 slots (view
    with .view(np.int64)); a sum_dec128 has its low 64 bits there (.view(np.uint64)) and
    its high 64 bits in "aggs_hi", which is 0 for every other op. "kernel" says which
    kernel ran (partial_reduce_plan_geometry) and "waveagg" the wave-aggregation setting
    the wide kernel ran with (DD_REDUCE_WAVEAGG; always 0 for kernel 0). May contain
    duplicate groups (partial semantics). The final merge sums "nn" per group, skips the
    value of a partial whose nn is 0 (it holds the op identity; (0, 0) for sum_dec128), and
    emits NULL for an aggregate whose total non-null count is 0 (DataFusion semantics).
    """
    nk = len(key_idx)
    na = len(aggs)
    keysc = (ctypes.c_int32 * nk)(*key_idx)
    aggc = (ctypes.c_int32 * na)(*[c if c is not None else 0 for c, _ in aggs])
    opsc = (ctypes.c_int32 * na)(*[AGG_OPS[o] for _, o in aggs])
    h = ctypes.c_void_p()
    _check(lib().dd_partial_reduce_run(ctypes.byref(batch.desc), keysc, nk, aggc, opsc,
                                       na, None, ctypes.byref(h)))
    try:
        kernel_ms = float(lib().dd_reducer_kernel_ms(h))
        n = lib().dd_reducer_n_rows(h)
        keys = np.empty((n, nk), dtype=np.uint64)
        keynull = np.empty(n, dtype=np.uint32)
        vals = np.empty((n, na), dtype=np.float64)
        nn = np.zeros((n, na), dtype=np.uint64)
        hi = np.zeros((n, na), dtype=np.uint64)
        if n:
            _check(lib().dd_reducer_fetch(
                h, keys.ctypes.data_as(ctypes.c_void_p),
                keynull.ctypes.data_as(ctypes.c_void_p),
                vals.ctypes.data_as(ctypes.c_void_p)))
            _check(lib().dd_reducer_fetch_nn(h, nn.ctypes.data_as(ctypes.c_void_p)))
            _check(lib().dd_reducer_fetch_hi(h, hi.ctypes.data_as(ctypes.c_void_p)))
        return {"keys": keys, "keynull": keynull, "aggs": vals, "nn": nn,
                "aggs_hi": hi, "kernel": int(lib().dd_reducer_kernel(h)),
                "waveagg": int(lib().dd_reducer_waveagg(h)), "kernel_ms": kernel_ms}
    finally:
        lib().dd_reducer_destroy(h)


def reduce_dec128_col(res, g, precision, scale):
    """The column dict that carries decimal sum `g` of a partial_reduce result into the
    shuffle: {"dtype": "dec128", "data": u64[n, 2] = [lo, hi], "valid": (nn > 0) as u8, or
    None when every partial has a non-null input, "precision": min(38, precision + 10)
    (DataFusion's sum type), "scale": scale}."""
    lo = np.ascontiguousarray(res["aggs"][:, g]).view(np.uint64)
    data = np.ascontiguousarray(np.stack([lo, res["aggs_hi"][:, g]], axis=1))
    ok = res["nn"][:, g] > 0
    return {"dtype": "dec128", "data": data,
            "valid": None if ok.all() else ok.astype(np.uint8),
            "precision": min(38, precision + 10), "scale": scale}


def final_merge(batch: DeviceBatch, key_idx, aggs, seg_offsets=None, seg_part=None, n_parts=1):
    """GPU final aggregation above the shuffle (dd_final_merge_run): merge the
    partial states in `batch` to one row per (partition, group).

    key_idx: 1..4 fixed-width key columns (u8, bool, i16, i32, i64, f32, f64), nullable.
    aggs: 1..8 of (state_col, op, nn_col) with op in AGG_OPS read as a merge op; nn_col is
    the i64 column of non-null input counts, None (or -1) for "count", whose state column
    holds the partial counts and whose nn is the merged count. A partial with nn == 0 is
    skipped; a total nn of 0 means SQL NULL (value slot unspecified).
    seg_offsets i64[S + 1], seg_part i32[S], n_parts: the segment layout; rows of all
    segments with one partition id form a partition and groups are formed within it.
    Default: one segment, one partition (a global group-by). exchanged_batch and
    partitioned_batch return (batch, layout) with layout a dict of these three, so
    final_merge(batch, key_idx, aggs, **layout) merges a shuffle's output in place.
    Returns {"keys": u64[n, nk], "keynull": u32[n], "aggs": f64[n, na] (integers bit-cast,
    min / max as value bits, a sum_dec128's low half), "aggs_hi": u64[n, na], "nn":
    u64[n, na], "group_offsets": i64[n_parts + 1] (partition p's groups are rows
    [off[p], off[p + 1]); their order inside a partition is unspecified), "kernel_ms":
    [claim, scan, merge]}."""
    h, _, n_parts = _run_final_merge("final_merge", batch, key_idx, aggs, seg_offsets, seg_part,
                                     n_parts)
    try:
        return _fetch_merged(h, len(key_idx), len(aggs), n_parts)
    finally:
        lib().dd_finalizer_destroy(h)


def _layout(who, layout, n_rows):
    """(seg_offsets i64[S + 1], seg_part i32[S], n_parts) of a {"seg_offsets", "seg_part",
    "n_parts"} layout, None being one segment and one partition over n_rows rows. `who`
    names the caller in the ValueError."""
    if layout is None:
        layout = {"seg_offsets": [0, n_rows], "seg_part": [0], "n_parts": 1}
    off = np.ascontiguousarray(layout["seg_offsets"], dtype=np.int64)
    part = np.ascontiguousarray(layout["seg_part"], dtype=np.int32)
    if len(off) != len(part) + 1:
        raise ValueError(f"{who}: seg_offsets must have one entry more than seg_part")
    return off, part, int(layout["n_parts"])


def _i32s(vals):
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def _layout_args(off, part, n_parts):
    return (off.ctypes.data_as(ctypes.c_void_p), part.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_int32(len(part)), ctypes.c_int32(n_parts))


def _run_final_merge(who, batch, key_idx, aggs, seg_offsets, seg_part, n_parts):
    """Marshal final_merge's arguments and run dd_final_merge_run: (handle, ops as a C array,
    n_parts of the layout used)."""
    layout = None if seg_offsets is None else {"seg_offsets": seg_offsets,
                                               "seg_part": seg_part, "n_parts": n_parts}
    off, part, n_parts = _layout(who, layout, batch.n_rows)
    opsc = _i32s([AGG_OPS[o] for _, o, _ in aggs])
    h = ctypes.c_void_p()
    _check(lib().dd_final_merge_run(
        ctypes.byref(batch.desc), _i32s(key_idx), len(key_idx),
        _i32s([c for c, _, _ in aggs]), opsc, _i32s([-1 if c is None else c for _, _, c in aggs]),
        len(aggs), *_layout_args(off, part, n_parts), None, ctypes.byref(h)))
    return h, opsc, n_parts


def _fetch_merged(h, nk, na, n_parts):
    """final_merge's result dict: host copies of a finalizer's interleaved state."""
    n = int(lib().dd_finalizer_n_groups(h))
    keys = np.zeros((n, nk), dtype=np.uint64)
    keynull = np.zeros(n, dtype=np.uint32)
    vals = np.zeros((n, na), dtype=np.float64)
    nn = np.zeros((n, na), dtype=np.uint64)
    hi = np.zeros((n, na), dtype=np.uint64)
    goff = np.zeros(n_parts + 1, dtype=np.int64)
    ms = (ctypes.c_float * 3)()
    _check(lib().dd_finalizer_group_offsets(h, goff.ctypes.data_as(ctypes.c_void_p)))
    _check(lib().dd_finalizer_kernel_ms(h, ms))
    if n:
        _check(lib().dd_finalizer_fetch(
            h, keys.ctypes.data_as(ctypes.c_void_p), keynull.ctypes.data_as(ctypes.c_void_p),
            vals.ctypes.data_as(ctypes.c_void_p)))
        _check(lib().dd_finalizer_fetch_nn(h, nn.ctypes.data_as(ctypes.c_void_p)))
        _check(lib().dd_finalizer_fetch_hi(h, hi.ctypes.data_as(ctypes.c_void_p)))
    return {"keys": keys, "keynull": keynull, "aggs": vals, "aggs_hi": hi, "nn": nn,
            "group_offsets": goff, "kernel_ms": list(ms)}


class _DeviceColumns:
    """What Joined, Sorted and Merged share: typed output columns on the device, owned by a
    library handle. A subclass names its accessor and destroy symbols; _out_cols holds
    (dtype, has validity) per column."""

    _COL_DATA = _COL_VALIDITY = _DESTROY = None

    def __init__(self, h, out_cols, n_rows):
        self.h = h
        self._out_cols = out_cols
        self.n_rows = n_rows

    def _views(self):
        """The columns as DeviceBatch.from_device takes them; nothing is copied."""
        data, valid = getattr(lib(), self._COL_DATA), getattr(lib(), self._COL_VALIDITY)
        return [{"dtype": dt, "data_ptr": data(self.h, i), "valid_ptr": valid(self.h, i)}
                for i, (dt, _) in enumerate(self._out_cols)]

    def col(self, i):
        """Host copy of output column i in Partitioner.col_out's shape (tests)."""
        dt, has_valid = self._out_cols[i]
        n = self.n_rows
        res = {"dtype": dt, "data": fixed_out(dt, np.zeros(0, dtype=FIXED_NP[dt]))}
        if n:
            res["data"] = fixed_out(dt, _d2h(getattr(lib(), self._COL_DATA)(self.h, i),
                                             n * ELEM_SIZE[dt], FIXED_NP[dt]))
        if has_valid:
            res["valid"] = (_d2h(getattr(lib(), self._COL_VALIDITY)(self.h, i), n, np.uint8)
                            if n else np.zeros(0, dtype=np.uint8))
        return res

    def destroy(self):
        if self.h:
            getattr(lib(), self._DESTROY)(self.h)
            self.h = None


def _output_view(src, col_data, col_validity, n_rows):
    """Non-owning DeviceBatch over the fixed-width output columns of a run Partitioner or
    an Exchanged (whose buffers must outlive it)."""
    view_cols = []
    for i, col in enumerate(src.cols):
        if col["dtype"] not in ELEM_SIZE:
            raise ValueError(f"column {i}: a {col['dtype']} column has no fixed-width device "
                             "view (final_merge takes fixed-width columns)")
        view_cols.append({"dtype": col["dtype"], "data_ptr": col_data(i),
                          "valid_ptr": col_validity(i)})
    return DeviceBatch.from_device(view_cols, n_rows)


def partitioned_batch(part: Partitioner):
    """(batch, layout) of a run Partitioner's output: a non-owning device view
    (DeviceBatch.from_device) plus {"seg_offsets", "seg_part", "n_parts"}, one segment per
    partition. Nothing is copied; `part` must outlive the view."""
    L = lib()
    batch = _output_view(part.batch, lambda i: L.dd_partitioner_col_data(part.h, i),
                         lambda i: L.dd_partitioner_col_validity(part.h, i),
                         part.batch.n_rows)
    return batch, {"seg_offsets": part.row_offsets(),
                   "seg_part": np.arange(part.nparts, dtype=np.int32),
                   "n_parts": part.nparts}


def exchanged_batch(ex: Exchanged):
    """(batch, layout) of an Exchanged window: a non-owning device view over its buffers
    plus {"seg_offsets", "seg_part", "n_parts"} derived from row_counts(): producer-major, then
    partition-major per producer, so segment s holds partition s % parts. Nothing is
    copied; `ex` must outlive the view."""
    L = lib()
    counts = ex.row_counts()
    n_prod, n_parts = counts.shape
    seg_offsets = np.zeros(n_prod * n_parts + 1, dtype=np.int64)
    np.cumsum(counts.reshape(-1)[:n_prod * n_parts], out=seg_offsets[1:])
    seg_part = (np.arange(n_prod * n_parts) % n_parts).astype(np.int32)
    batch = _output_view(ex.part.batch, lambda i: L.dd_exchanged_col_data(ex.h, i),
                         lambda i: L.dd_exchanged_col_validity(ex.h, i), int(ex.total_rows))
    return batch, {"seg_offsets": seg_offsets, "seg_part": seg_part, "n_parts": int(n_parts)}


JOIN_TYPES = {"inner": 0, "left_semi": 1, "left_anti": 2, "right_semi": 3, "right_anti": 4,
              "left": 5, "right": 6, "full": 7}


class Joined(_DeviceColumns):
    """Output of hash_join (dd_joiner_*): pair indices and the projected columns, all on
    the device, plus the emitting side's segment layout with new offsets."""

    _COL_DATA, _COL_VALIDITY = "dd_joiner_col_data", "dd_joiner_col_validity"
    _DESTROY = "dd_joiner_destroy"

    def __init__(self, h, join_type, out_cols, seg_part, n_parts):
        super().__init__(h, out_cols, int(lib().dd_joiner_n_rows(h)))
        self.join_type = join_type
        self._seg_part = seg_part
        self._n_parts = n_parts

    def seg_offsets(self):
        """Host i64[S + 1] over the output rows; S and seg_part are the emitting side's."""
        out = np.zeros(len(self._seg_part) + 1, dtype=np.int64)
        _check(lib().dd_joiner_seg_offsets(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def layout(self):
        return {"seg_offsets": self.seg_offsets(), "seg_part": self._seg_part.copy(),
                "n_parts": self._n_parts}

    def pairs_ptr(self):
        """(build_idx, probe_idx) device pointers to u32[n_rows]; None for the side a semi /
        anti join does not emit, and for both when the emitting side had no rows."""
        return lib().dd_joiner_build_idx(self.h), lib().dd_joiner_probe_idx(self.h)

    def pairs(self):
        """(build_idx, probe_idx) as host u32[n_rows] copies (tests); None for the side a
        semi / anti join does not emit."""
        emitted = (not self.join_type.startswith("right_"),
                   not self.join_type.startswith("left_"))
        return tuple(None if not e else
                     _d2h(p, self.n_rows * 4, np.uint32) if self.n_rows else
                     np.zeros(0, dtype=np.uint32)
                     for e, p in zip(emitted, self.pairs_ptr()))

    def batch(self):
        """(view, layout): a non-owning DeviceBatch over the output columns (build_proj
        first) plus {"seg_offsets", "seg_part", "n_parts"}, ready for final_merge,
        partial_reduce or Partitioner. Nothing is copied; this Joined must outlive it."""
        if not self._out_cols:
            raise ValueError("hash_join: no projected columns, so there is no batch (pairs only)")
        return DeviceBatch.from_device(self._views(), self.n_rows), self.layout()

    def kernel_ms(self):
        """[build, count, scan, emit, gather] hipEvent times in ms."""
        out = (ctypes.c_float * 5)()
        _check(lib().dd_joiner_kernel_ms(self.h, out))
        return list(out)


def _run_join(entry, build, build_keys, probe, probe_keys, join_type, build_layout,
              probe_layout, build_proj, probe_proj):
    """Marshal a join's arguments and run `entry` (dd_hash_join_run or its outer twin):
    (handle, build seg_part, probe seg_part, n_parts)."""
    boff, bpart, bparts = _layout("hash_join", build_layout, build.n_rows)
    poff, ppart, pparts = _layout("hash_join", probe_layout, probe.n_rows)
    h = ctypes.c_void_p()
    _check(getattr(lib(), entry)(
        ctypes.byref(build.desc), _i32s(build_keys), ctypes.byref(probe.desc),
        _i32s(probe_keys), ctypes.c_int32(len(build_keys)),
        ctypes.c_int32(JOIN_TYPES[join_type]), *_layout_args(boff, bpart, bparts),
        *_layout_args(poff, ppart, pparts), _i32s(build_proj), ctypes.c_int32(len(build_proj)),
        _i32s(probe_proj), ctypes.c_int32(len(probe_proj)), None, ctypes.byref(h)))
    return h, bpart, ppart, bparts


def hash_join(build: DeviceBatch, build_keys, probe: DeviceBatch, probe_keys,
              join_type="inner", build_layout=None, probe_layout=None, build_proj=None,
              probe_proj=None):
    """GPU partitioned hash join above two co-partitioned shuffles (dd_hash_join_run;
    DESIGN.md §19): HashJoinExec mode=Partitioned with `build` as its left side.

    build_keys / probe_keys: 1..4 key columns per side, pairwise of one dtype out of u8,
    bool, i16, i32, i64; a row with a NULL in any key component matches nothing.
    join_type: "inner", "left_semi", "left_anti" (build rows), "right_semi", "right_anti"
    (probe rows).
    build_layout / probe_layout: {"seg_offsets", "seg_part", "n_parts"} as exchanged_batch
    and partitioned_batch return them; partition p joins partition p only, and n_parts must
    be equal. Default: one segment, one partition (a plain hash join).
    build_proj / probe_proj: output column indices, build columns first; default: all
    columns of the side(s) the join type emits. Fixed-width dtypes only.
    Returns a Joined. Output rows follow the emitting side's row order (probe for inner and
    right_*, build for left_*) and keep its segments."""
    if join_type not in JOIN_TYPES:
        raise ValueError(f"hash_join: unknown join type {join_type!r}")
    if len(build_keys) != len(probe_keys):
        raise ValueError("hash_join: the two sides need the same number of key columns")
    emits_build = not join_type.startswith("right_")
    emits_probe = not join_type.startswith("left_")
    if build_proj is None:
        build_proj = list(range(build.desc.n_cols)) if emits_build else []
    if probe_proj is None:
        probe_proj = list(range(probe.desc.n_cols)) if emits_probe else []
    h, bpart, ppart, bparts = _run_join("dd_hash_join_run", build, build_keys, probe,
                                        probe_keys, join_type, build_layout, probe_layout,
                                        build_proj, probe_proj)
    out_cols = [(b.cols[i]["dtype"], bool(b.desc.cols[i].validity))
                for b, proj in ((build, build_proj), (probe, probe_proj)) for i in proj]
    return Joined(h, join_type, out_cols, ppart if emits_probe else bpart, bparts)


OUTER_JOIN_TYPES = ("left", "right", "full")
JOIN_NONE = 0xFFFFFFFF  # DD_JOIN_NONE: the absent side of an outer join's output row


def outer_join(build: DeviceBatch, build_keys, probe: DeviceBatch, probe_keys, join_type,
               build_layout=None, probe_layout=None, build_proj=None, probe_proj=None):
    """GPU partitioned outer hash join (dd_hash_join_outer_run): hash_join's
    arguments, keys, layouts and refusals, for join_type "left", "right" or "full" (`build`
    is HashJoinExec's left side).

    "right": every inner pair plus one row per probe row without a match, build side NULL;
    "left": every inner pair plus one row per build row no probe row matched, probe side
    NULL; "full": both. A NULL-key row is a row without a match.
    Returns a Joined whose segments come in two sections: the probe side's segments (rows in
    probe row order; an unmatched probe row in its place under right / full), then for left
    and full the build side's segments holding its unmatched rows in row order. seg_part is
    the concatenation, n_parts unchanged. pairs() returns both arrays, JOIN_NONE marking the
    absent side. Every column of a NULL-extended side (probe for left, build for right, both
    for full) has validity: 0 and zero value bytes on a JOIN_NONE row.
    build_proj / probe_proj: default all columns of both sides."""
    if join_type not in JOIN_TYPES:
        raise ValueError(f"outer_join: unknown join type {join_type!r}")
    if len(build_keys) != len(probe_keys):
        raise ValueError("outer_join: the two sides need the same number of key columns")
    if build_proj is None:
        build_proj = list(range(build.desc.n_cols))
    if probe_proj is None:
        probe_proj = list(range(probe.desc.n_cols))
    # the five other types reach the library too: it refuses them and names hash_join's entry
    h, bpart, ppart, bparts = _run_join("dd_hash_join_outer_run", build, build_keys, probe,
                                        probe_keys, join_type, build_layout, probe_layout,
                                        build_proj, probe_proj)
    null_ext = {"left": (False, True), "right": (True, False), "full": (True, True)}[join_type]
    out_cols = [(b.cols[i]["dtype"], ext or bool(b.desc.cols[i].validity))
                for b, proj, ext in ((build, build_proj, null_ext[0]),
                                     (probe, probe_proj, null_ext[1])) for i in proj]
    seg_part = ppart if join_type == "right" else np.concatenate([ppart, bpart])
    joined = Joined(h, join_type, out_cols, seg_part, bparts)
    assert int(lib().dd_joiner_n_segs(h)) == len(seg_part)
    return joined


class Merged(_DeviceColumns):
    """Output of final_merge_device (dd_finalizer_*): the merged rows kept on the device as
    typed columns, for a further operator."""

    _COL_DATA, _COL_VALIDITY = "dd_finalizer_col_data", "dd_finalizer_col_validity"
    _DESTROY = "dd_finalizer_destroy"

    def __init__(self, h, key_dtypes, ops, n_parts, with_nn):
        self.key_dtypes = list(key_dtypes)
        self.ops = list(ops)
        self.n_parts = n_parts
        self.with_nn = with_nn
        self.n_groups = int(lib().dd_finalizer_n_groups(h))
        self.n_cols = int(lib().dd_finalizer_n_cols(h))
        inv = {v: k for k, v in DTYPE_CODE.items()}
        self.dtypes = [inv[int(lib().dd_finalizer_col_dtype(h, i))] for i in range(self.n_cols)]
        # keys are nullable, every aggregate but count is, the nn columns are not
        has_valid = [True] * len(self.key_dtypes) + [o != "count" for o in self.ops]
        has_valid += [False] * (self.n_cols - len(has_valid))
        super().__init__(h, list(zip(self.dtypes, has_valid)), self.n_groups)

    def group_offsets(self):
        """Host i64[n_parts + 1]: partition p's groups are rows [off[p], off[p + 1])."""
        out = np.zeros(self.n_parts + 1, dtype=np.int64)
        _check(lib().dd_finalizer_group_offsets(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def layout(self):
        return {"seg_offsets": self.group_offsets(),
                "seg_part": np.arange(self.n_parts, dtype=np.int32), "n_parts": self.n_parts}

    def batch(self):
        """(view, layout): a non-owning DeviceBatch over the typed columns (keys, one column
        per aggregate, then the nn columns if asked for) plus the layout with seg_offsets =
        group_offsets and identity seg_part, ready for sort_topk, Partitioner, partial_reduce,
        final_merge or a join. Nothing is copied; this Merged must outlive it."""
        return DeviceBatch.from_device(self._views(), self.n_groups), self.layout()

    def fetch(self):
        """The dict final_merge returns for the same input (host copies of the interleaved
        state), so a test can hold the columns to it."""
        return _fetch_merged(self.h, len(self.key_dtypes), len(self.ops), self.n_parts)


def final_merge_device(batch: DeviceBatch, key_idx, aggs, seg_offsets=None, seg_part=None,
                       n_parts=1, with_nn=False):
    """final_merge that keeps its result on the device: the same arguments,
    kernels and refusals (dd_final_merge_run), then dd_finalizer_columns turns the interleaved
    state into typed device columns. Returns a Merged.

    Columns: each key in its input dtype with validity from keynull (a float key comes out
    canonicalised, +0.0 for -0.0 and one quiet NaN, because the group identity is); one
    column per aggregate, i64 for count / sum_i64 / min_i64 / max_i64, f64 for sum_f64 /
    min_f64 / max_f64, dec128 for sum_dec128, with validity nn != 0 (a total nn of 0 is SQL
    NULL; count has no validity buffer and is never NULL); with_nn adds one i64 nn column per
    aggregate after the value columns."""
    h, opsc, n_parts = _run_final_merge("final_merge_device", batch, key_idx, aggs, seg_offsets,
                                        seg_part, n_parts)
    try:
        key_dtypes = [batch.cols[k]["dtype"] for k in key_idx]
        _check(lib().dd_finalizer_columns(
            h, _i32s([DTYPE_CODE[d] for d in key_dtypes]), ctypes.c_int32(len(key_idx)), opsc,
            ctypes.c_int32(len(aggs)), ctypes.c_int32(int(with_nn)), None))
    except Exception:
        lib().dd_finalizer_destroy(h)
        raise
    return Merged(h, key_dtypes, [o for _, o, _ in aggs], n_parts, bool(with_nn))


SORT_DESC = 1         # DD_SORT_DESC
SORT_NULLS_FIRST = 2  # DD_SORT_NULLS_FIRST


class Sorted(_DeviceColumns):
    """Output of sort_topk (dd_sorter_*): perm, the gathered columns and the new segment
    offsets, all on the device; one segment per partition."""

    _COL_DATA, _COL_VALIDITY = "dd_sorter_col_data", "dd_sorter_col_validity"
    _DESTROY = "dd_sorter_destroy"

    def __init__(self, h, out_cols, n_parts):
        super().__init__(h, out_cols, int(lib().dd_sorter_n_rows(h)))
        self._n_parts = n_parts

    def seg_offsets(self):
        """Host i64[n_parts + 1]: partition p's rows are [off[p], off[p + 1])."""
        out = np.zeros(self._n_parts + 1, dtype=np.int64)
        _check(lib().dd_sorter_seg_offsets(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def layout(self):
        return {"seg_offsets": self.seg_offsets(),
                "seg_part": np.arange(self._n_parts, dtype=np.int32), "n_parts": self._n_parts}

    def perm_ptr(self):
        """Device pointer to u32[n_rows], the input row of each output row (None at zero
        rows)."""
        return lib().dd_sorter_perm(self.h)

    def perm(self):
        """perm as a host u32[n_rows] copy (tests)."""
        if not self.n_rows:
            return np.zeros(0, dtype=np.uint32)
        return _d2h(self.perm_ptr(), self.n_rows * 4, np.uint32)

    def batch(self):
        """(view, layout): a non-owning DeviceBatch over the projected columns plus
        {"seg_offsets", "seg_part", "n_parts"}, ready for Partitioner, partial_reduce,
        final_merge, a join or another sort_topk. Nothing is copied; this Sorted must outlive
        it."""
        if not self._out_cols:
            raise ValueError("sort_topk: no projected columns, so there is no batch (perm only)")
        return DeviceBatch.from_device(self._views(), self.n_rows), self.layout()

    def info(self):
        """{"passes_planned": radix passes the key dtypes and the layout call for,
        "passes_run": those left after the census dropped every constant digit (all of them
        under DD_SORT_SKIP=0), "tile_rows": rows per scatter tile, "words": 64-bit words per
        row}. Zero passes when the result is empty (no device work)."""
        out = (ctypes.c_int32 * 4)()
        _check(lib().dd_sorter_info(self.h, out))
        return dict(zip(("passes_planned", "passes_run", "tile_rows", "words"),
                        (int(v) for v in out)))

    def kernel_ms(self):
        """[encode + census, passes, segment output, gather] hipEvent times in ms."""
        out = (ctypes.c_float * 4)()
        _check(lib().dd_sorter_kernel_ms(self.h, out))
        return list(out)


def sort_topk(batch: DeviceBatch, keys, layout=None, fetch=None, proj=None):
    """GPU SortExec / TopK per partition above the shuffle (dd_sort_run; DESIGN.md §22;
    sortref.sort_ref is the same rules in numpy).

    keys: 1..4 of (col, descending, nulls_first), the two flags independent (DataFusion
    prints `x DESC` for DESC NULLS FIRST and `x ASC NULLS LAST` for the other default);
    dtypes u8, bool, i16, i32, i64, f32, f64 (totalOrder on the raw bits), dec128.
    layout: {"seg_offsets", "seg_part", "n_parts"} as exchanged_batch, partitioned_batch,
    Joined.batch, Merged.batch and Sorted.batch return it; default one segment, one partition.
    fetch: None keeps every row, k >= 0 the first min(k, rows) of each partition.
    proj: columns to gather on the device, default all; fixed-width dtypes only.
    Returns a Sorted: one segment per partition, rows in key order, ties in input order
    (stable). sort_topk over Sorted.batch() with sortref.collapsed_layout and the same fetch
    is the SortPreservingMergeExec(fetch) at the top of the plan."""
    try:
        keys = [(int(c), bool(d), bool(nf)) for c, d, nf in keys]
    except (TypeError, ValueError):
        raise ValueError("sort_topk: keys are (col, descending, nulls_first) triples") from None
    if fetch is not None and int(fetch) != fetch:
        raise ValueError("sort_topk: fetch must be None or an integer")
    if proj is None:
        proj = list(range(batch.desc.n_cols))
    proj = [int(c) for c in proj]
    off, part, n_parts = _layout("sort_topk", layout, batch.n_rows)
    # None is the library's -1; a negative fetch reaches it as one it refuses
    fetch_c = -1 if fetch is None else int(fetch) if fetch >= 0 else min(int(fetch), -2)
    kf = [(SORT_DESC if d else 0) | (SORT_NULLS_FIRST if nf else 0) for _, d, nf in keys]
    h = ctypes.c_void_p()
    _check(lib().dd_sort_run(
        ctypes.byref(batch.desc), _i32s([c for c, _, _ in keys]), _i32s(kf),
        ctypes.c_int32(len(keys)), _i32s(proj), ctypes.c_int32(len(proj)),
        *_layout_args(off, part, n_parts), ctypes.c_int64(fetch_c), None, ctypes.byref(h)))
    out_cols = [(batch.cols[i]["dtype"], bool(batch.desc.cols[i].validity)) for i in proj]
    return Sorted(h, out_cols, n_parts)
