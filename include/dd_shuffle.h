/* include/dd_shuffle.h — C ABI of the MI355X-native shuffle/exchange path.
 *
 * This is the drop-in boundary: the exports mirror, 1:1, the reference's
 * transport/operator seam for the hash-shuffle hot path so that a one-file Rust shim
 * implementing `WorkerChannel` (reference: src/protocol/worker_channel.rs:19-46, resolved via
 * src/protocol/channel_resolver.rs:27-41) can delegate to these functions wherever cargo
 * exists. The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * No torch types anywhere; plain pointers and sizes. All device pointers are HIP device
 * memory on the current device. All entry points return dd_status; dd_last_error() gives a
 * human-readable message (mirrors the reference's DataFusionError <-> tonic Status mapping,
 * src/protocol/grpc/errors/).
 */

#ifndef DD_SHUFFLE_H
#define DD_SHUFFLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- status / errors ---------------- */

typedef enum dd_status {
    DD_OK = 0,
    DD_ERR_INVALID = 1,     /* bad arguments / unsupported shape */
    DD_ERR_NO_DEVICE = 2,   /* no HIP device — the product path FAILS here, no CPU fallback */
    DD_ERR_HIP = 3,         /* HIP runtime error */
    DD_ERR_RCCL = 4,        /* RCCL error */
    DD_ERR_NOT_FOUND = 5,   /* unknown TaskKey (mirrors worker "plan not found" timeout,
                               src/worker/impl_execute_task.rs:29-34) */
    DD_ERR_UNSUPPORTED = 6  /* dtype/partition-count combination outside round-1 coverage */
} dd_status;

const char *dd_last_error(void);
int dd_device_count(void); /* number of visible HIP devices (0 on a GPU-less box) */
const char *dd_version(void);

/* ---------------- data model ----------------
 * Device-resident Arrow-layout columns. Validity is UNPACKED u8 (1=valid).
 * dtype codes shared with oracle/dd_oracle.c. */

typedef enum dd_dtype {
    DD_DT_U8 = 1,
    DD_DT_I16 = 2,
    DD_DT_I32 = 3,
    DD_DT_I64 = 4,
    DD_DT_F32 = 5,
    DD_DT_F64 = 6,
    DD_DT_BOOL = 7,  /* unpacked u8 0/1 */
    DD_DT_UTF8 = 8,  /* i32 offsets[n+1] + byte buffer */
    DD_DT_DICT32 = 9, /* i32 indices; dictionary values as utf8 (offsets+bytes) */
    /* Opaque 16-byte value in the Arrow Decimal128 value-buffer layout: little-endian
     * two's complement, lo = bytes 0..7, hi = bytes 8..15. `data` must be 16-byte aligned
     * (dd_partitioner_create: DD_ERR_INVALID otherwise). Precision and scale are schema,
     * not device data: the shim keeps them beside the column. Hashes as the two i64 keys
     * (lo, hi), DESIGN.md §16. Seam: the Decimal128 columns DataFusion gives the TPC-H
     * money/quantity fields that RepartitionExec(Hash) routes (tests/tpch_plans_test.rs);
     * arrow's create_hashes over the i128 value buffer is the reference operation.
     * Interval(MonthDayNano) and FixedSizeBinary(16) share the layout. */
    DD_DT_DEC128 = 10
} dd_dtype;

#define DD_MAX_COLS 24
#define DD_MAX_KEYS 8
#define DD_MAX_PARTITIONS 2048u /* round-1 cap (LDS budget), DESIGN.md §5 */

typedef struct dd_col_desc {
    int32_t dtype;            /* dd_dtype */
    const void *data;         /* device: values (DEC128: 16-byte aligned), or utf8 bytes */
    const uint8_t *validity;  /* device, unpacked u8, NULL => all valid */
    const int32_t *offsets;   /* device, UTF8 only: offsets[n_rows+1] */
    int64_t data_len;         /* UTF8: byte length of `data`; else 0 */
    const void *dict_bytes;   /* DICT32: device value bytes */
    const int32_t *dict_offsets; /* DICT32: device offsets[dict_n+1] */
    int64_t dict_n;           /* DICT32: number of dictionary values */
} dd_col_desc;
/* UTF8 input to dd_partitioner_create may be an Arrow slice: offsets[0] may be non-zero and
 * `data` may hold bytes before offsets[0] and after offsets[n_rows]; the one requirement is
 * data_len >= offsets[n_rows] (all of `data` stays readable). Row i's bytes are
 * data[offsets[i] .. offsets[i+1]). Outputs are zero-based whatever the input's base: the
 * column's output buffer has data_len bytes, of which the first offsets[n_rows] - offsets[0]
 * are defined (the strings in partition-major order) and the rest unspecified;
 * dd_partitioner_byte_offsets[P] and dd_partitioner_var_offsets64[n_rows] equal that byte
 * total, not data_len. The reuse contract below is narrower: a refilled column is zero-based
 * and exactly sized. */

typedef struct dd_batch_desc {
    int64_t n_rows;
    int32_t n_cols;
    dd_col_desc cols[DD_MAX_COLS];
} dd_batch_desc;

/* ---------------- hash-repartition (the producer head) ----------------
 * Replaces the `RepartitionExec(Hash(keys, P_total))` head the reference inserts on the
 * producer: ProducerHead::insert (src/distributed_planner/network_boundary.rs:86-106),
 * required input shape at src/execution_plans/network_shuffle.rs:121-127, lazily re-created
 * per task at src/worker/task_data.rs:104-116. Semantics: DESIGN.md §3 (normative; stable).
 *
 * Two-phase (prepare/execute) so repeated executions reuse workspace + output buffers —
 * mirroring the worker's lazy plan-head caching. All output buffers are partition-major
 * contiguous. */

typedef struct dd_partitioner dd_partitioner; /* opaque */

dd_status dd_partitioner_create(const dd_batch_desc *batch, const int32_t *key_cols,
                                int32_t n_keys, uint32_t n_partitions,
                                dd_partitioner **out);
/* Reuse contract. A partitioner may be run any number of times; every run recomputes the
 * whole result from the input buffers named at create time, and no workspace state
 * carries over from the run before. Between runs the caller may overwrite IN PLACE, with
 * n_rows unchanged, the contents of:
 *   - fixed-width data (key or payload), bool and dict32 indices included;
 *   - validity bytes (a column keeps having, or not having, a validity buffer);
 *   - utf8 bytes and offsets, provided offsets[n_rows] stays equal to data_len and no
 *     string is longer than the longest one at create time (the LDS-staged byte scatter
 *     sizes its image from that length).
 * The dictionary bytes and offsets of a dict32 KEY column must not change: their hashes
 * are computed once, at create time. Pointers, dtypes, data_len and dict_n are fixed.
 * Each overwrite must be ordered after dd_partitioner_wait_phase2 of the previous run
 * (or a device sync), and the next run after the overwrite. Anything else is undefined
 * and may fault the device.
 *
 * Runs K1 (hash+count), K2 (scan), K3 (stable scatter) on `stream` (a hipStream_t, or NULL
 * for the default stream). Asynchronous; results valid after stream sync. */
dd_status dd_partitioner_run(dd_partitioner *p, void *stream);
/* coarse-bucket variant: pid = (h % pid_total) / coarse_div — pid_total/coarse_div
 * CONTIGUOUS ranges of the final partition space (pass A of the two-level var scatter,
 * DESIGN.md §11; both arguments must be powers of two) */
dd_status dd_partitioner_create_ranged(const dd_batch_desc *batch, const int32_t *key_cols,
                                       int32_t n_keys, uint32_t pid_total,
                                       uint32_t coarse_div, dd_partitioner **out);
/* Phase split for batch pipelining (the reference streams batches through
 * RepartitionExec continuously; overlapping batch s+1's hash/count with batch s's
 * scatter mirrors that): phase1 = K1+K2 (+byte scans), phase2 = K3 (+K4). phase2 must be
 * ordered after phase1 of the SAME partitioner (same stream, or an event). */
dd_status dd_partitioner_run_phase1(dd_partitioner *p, void *stream);
dd_status dd_partitioner_run_phase2(dd_partitioner *p, void *stream);
/* make `stream` wait for this partitioner's last phase1 / phase2 completion (for
 * cross-stream batch pipelining) */
dd_status dd_partitioner_wait_phase1(dd_partitioner *p, void *stream);
dd_status dd_partitioner_wait_phase2(dd_partitioner *p, void *stream);
void dd_partitioner_destroy(dd_partitioner *p);

/* Read-only view of the plan dd_partitioner_create chose (which scatter tier, which block
 * shape), so tests and benchmarks can assert the tier they mean to measure instead of
 * mirroring the gates. Needs no run. */
typedef struct dd_partitioner_info {
    int32_t path;      /* 0 = v1 (k_scatter), 1 = staged, 2 = pre (K3-P) */
    int32_t wpb, gmax; /* staged/pre block shape; 0 on v1 */
    int32_t hl;        /* 0 none, 1 k_scatter_hl, 2 k_scatter_hlg */
    int32_t rhash;     /* 1: K3 recomputes hashes, no pid array */
    int32_t pid_elem;  /* 4, or 1 for byte pids */
    int32_t k5;        /* 1: LDS-staged var-byte scatter, 0: K4 gather (or no var col) */
    int32_t k5_wpb;    /* K5 waves per block; 0 when k5 == 0 */
    int32_t k5_maxlen; /* longest string at create time; 0 when k5 == 0 */
    int32_t rpb;       /* pre: rounds per block; 0 otherwise */
    int64_t round_rows; /* gmax*wpb*64 on staged/pre, else 0 */
    int64_t n_launch;   /* nchunks (v1/staged) or nrounds (pre) */
} dd_partitioner_info;
dd_status dd_partitioner_get_info(const dd_partitioner *p, dd_partitioner_info *out);
/* how the pre path precomputes its scatter layout: 0 = not the pre path, 1 = per wave
 * segment (k_hash_count_seg + segment-granular scan), 2 = per round (k_hash_count_round +
 * round-granular scan). Kept out of dd_partitioner_info, whose size is part of the ABI. */
int32_t dd_partitioner_pre_layout(const dd_partitioner *p);
/* 1 when the pre path scatters in wide rounds (8192 rows per round staged in two column
 * passes, k_scatter_pre_wide; dd_partitioner_info then reports gmax 8 and round_rows 8192),
 * else 0. Eligible: round layout, P <= 128, no validity, element sizes (8,8,8,4),
 * (4,8,8,4) or (8,8,8,4,4). DD_PRE_WIDE=1 forces it on an eligible shape and 0 forbids it;
 * unset, it is taken from 8,000,000 rows up (DD_PRE_WIDE_MIN_ROWS overrides the
 * threshold) and below 2^29 rows. Results do not depend on it. */
int32_t dd_partitioner_pre_wide(const dd_partitioner *p);
/* the compile-time key signature the K1 hash/count kernel runs with: 0 = the generic
 * run-time key loop; otherwise kind(key 0) | kind(key 1) << 4 with kinds 1 u8/bool, 2 i16,
 * 3 i32, 4 i64, 5 f32, 6 f64, 7 dict32. Chosen at create time for one non-nullable key of
 * those kinds and the pairs i64+i32 and u8/bool+u8/bool on the staged and pre paths
 * (ranged partitioners included); DD_K1_SPEC=0 forces 0. Results do not depend on it. */
int32_t dd_partitioner_k1_spec(const dd_partitioner *p);
/* out[b] = logical block of hardware block b in a grid of `nblocks` under DD_PRE_XCD=1
 * (hardware blocks with equal b mod 8 get one contiguous run of logical blocks); runs on
 * the host, so the map can be checked without a device */
void dd_pre_xcd_block_map(int64_t nblocks, int64_t *out);

/* result accessors (pointers are device memory owned by the partitioner) */
/* u32[n_rows] of per-row partition ids. NULL ONLY when the opt-in DD_RHASH=1 recompute
 * path is active (all-fixed no-validity batches with integer keys, measured slower and
 * OFF by default — DESIGN.md §9): shim authors must handle NULL for robustness but will
 * not see it under default configuration; partition membership is always fully defined
 * by col_data + row_offsets either way. */
const uint32_t *dd_partitioner_pids(const dd_partitioner *p);
/* element size of the pid array: 4 (u32) normally, 1 (u8) when the precomputed-layout
 * path stores byte pids (n_partitions <= 256) — cast the pids pointer accordingly */
int32_t dd_partitioner_pid_elem(const dd_partitioner *p);
const void *dd_partitioner_col_data(const dd_partitioner *p, int32_t col); /* partition-major */
const uint8_t *dd_partitioner_col_validity(const dd_partitioner *p, int32_t col);
const uint32_t *dd_partitioner_col_lengths(const dd_partitioner *p, int32_t col); /* utf8 */
/* copies part_row_offsets[P+1] (rows) to host */
dd_status dd_partitioner_row_offsets(const dd_partitioner *p, int64_t *host_out);
/* staged-var path only: device pointer to the rebuilt 64-bit Arrow offsets [n_rows+1]
 * of a var column (K4c output); NULL on the v1 path */
const uint64_t *dd_partitioner_var_offsets64(const dd_partitioner *p, int32_t col);
/* out32[i] = (int32)(off64[lo_row + i] - off64[lo_row]) for i in [0, n]; device buffers;
 * lets a bucket/chunk of a var column be re-consumed as an Arrow batch view */
dd_status dd_make_offsets32(const uint64_t *off64, int64_t lo_row, int64_t n,
                            int32_t *out32, void *stream);
/* copies per-var-col part_byte_offsets[P+1] to host */
dd_status dd_partitioner_byte_offsets(const dd_partitioner *p, int32_t col, int64_t *host_out);
/* per-kernel last-run durations in ms, measured with hipEvents on the run stream:
 * [0]=K1 hash+count, [1]=K2 scan, [2]=K3 scatter. Valid after a synced run. */
dd_status dd_partitioner_kernel_ms(const dd_partitioner *p, float out_ms[3]);

/* ---------------- exchange (the transport data plane) ----------------
 * Replaces the Arrow-Flight-over-gRPC data plane (client demux src/protocol/grpc/
 * worker_client.rs:89-320; server encode+tagging src/protocol/grpc/worker_service.rs:133-184,
 * 363-433) with an RCCL all-to-all-v over xGMI: one rank per GPU, rank = task
 * (TaskKey.task_number, src/stage.rs:134-139). Consumer rank r owns partition window
 * [P*r, P*(r+1)) of P_total = P*nranks (src/execution_plans/network_shuffle.rs:232-244,
 * scale_partitioning src/execution_plans/common.rs:18-30). Received data is concatenated
 * in producer-rank order (deterministic refinement of the reference's select_all merge). */

typedef struct dd_comm dd_comm; /* opaque: RCCL communicator + streams */

#define DD_UNIQUE_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */
dd_status dd_comm_unique_id(void *bytes128); /* rank 0 calls; share out-of-band */
dd_status dd_comm_init(const void *bytes128, int rank, int nranks, dd_comm **out);
void dd_comm_destroy(dd_comm *c);

typedef struct dd_exchanged dd_exchanged; /* opaque: received window buffers */

/* Exchange the partitioned result: every rank sends partition window [P*j, P*(j+1)) of its
 * local result to rank j and receives its own window from every rank. P (= partitions per
 * consumer) is inferred: partitioner P_total must equal P*nranks. Synchronous on `stream`. */
dd_status dd_exchange_run(dd_comm *c, const dd_partitioner *p, void *stream,
                          dd_exchanged **out);
void dd_exchanged_destroy(dd_exchanged *e);

/* accessors: my window, producer-major then partition-major per producer */
int64_t dd_exchanged_total_rows(const dd_exchanged *e);
const void *dd_exchanged_col_data(const dd_exchanged *e, int32_t col);
const uint8_t *dd_exchanged_col_validity(const dd_exchanged *e, int32_t col);
const uint32_t *dd_exchanged_col_lengths(const dd_exchanged *e, int32_t col);
/* row counts per (producer, local partition): host_out[nranks*P] */
dd_status dd_exchanged_row_counts(const dd_exchanged *e, int64_t *host_out);
/* bytes per (producer, local partition) for a var col: host_out[nranks*P] */
dd_status dd_exchanged_byte_counts(const dd_exchanged *e, int32_t col, int64_t *host_out);
/* last exchange wall time (ms, hipEvent on the exchange stream) and payload bytes sent by
 * this rank to OTHER ranks (xGMI egress) */
dd_status dd_exchanged_stats(const dd_exchanged *e, float *ms, int64_t *egress_bytes);

/* ---------------- dictionary GC (compact + resend dictionaries) ----------------
 * The reference compacts every dictionary column to the values a batch references before
 * it goes on the wire and resends the compacted dictionary with the batch
 * (garbage_collect_arrays + DictionaryHandling::Resend,
 * src/protocol/grpc/worker_service.rs:363-433). Here the unit is a WINDOW: the P_total
 * partitions are cut into n_windows contiguous ranges and each window gets its own
 * compacted dictionary and window-local indices (normative). n_windows =
 * nranks gives one dictionary per consumer (dd_exchange_run_gc); n_windows = P_total gives
 * one per partition (the Arrow boundary, the reference's per-batch granularity). */

typedef struct dd_dict_gc dd_dict_gc; /* opaque: bitmaps, remapped indices, dictionaries */

/* Runs mark/rank/compact/remap for dict32 column `col` of a run partitioner. Synchronous
 * (one host sync to size the dictionaries); `stream` must be ordered after the
 * partitioner's run. The partitioner's own output is not modified
 * and must outlive the GC object. A valid row whose index is outside [0, dict_n) is never
 * dereferenced: DD_ERR_INVALID (worker_service.rs:363-433 is the seam). */
dd_status dd_dict_gc_run(const dd_partitioner *p, int32_t col, uint32_t n_windows,
                         void *stream, dd_dict_gc **out);
/* worker_service.rs:363-433: releases the GC'd dictionaries and indices */
void dd_dict_gc_destroy(dd_dict_gc *g);
/* worker_service.rs:363-433: which column / how many windows this GC covers */
int32_t dd_dict_gc_col(const dd_dict_gc *g);
uint32_t dd_dict_gc_n_windows(const dd_dict_gc *g);
/* device i32[n_rows]: window-local indices, partition-major like the partitioner's output
 * (0 for null rows; the validity buffer stays the partitioner's) —
 * worker_service.rs:363-433 ships these as the batch's dictionary keys */
const int32_t *dd_dict_gc_indices(const dd_dict_gc *g);
/* host prefix sums, [n_windows+1] each: values and bytes per window
 * (worker_service.rs:363-433: the size of each resent dictionary) */
dd_status dd_dict_gc_counts(const dd_dict_gc *g, int64_t *val_off, int64_t *byte_off);
/* device: window w's zero-based offsets array (nvals_w+1 entries) starts at element
 * val_off[w] + w; its bytes start at byte_off[w] — each window is a ready Arrow utf8 array
 * and one contiguous send slice (worker_service.rs:363-433: the resent dictionary) */
const int32_t *dd_dict_gc_dict_offsets(const dd_dict_gc *g);
const uint8_t *dd_dict_gc_dict_bytes(const dd_dict_gc *g);
/* hipEvent durations of the last run in ms: mark, rank, compact, remap (the device cost
 * of the worker_service.rs:363-433 GC step) */
dd_status dd_dict_gc_kernel_ms(const dd_dict_gc *g, float out_ms[4]);

/* dd_exchange_run that also carries dictionaries (worker_service.rs:363-433, Resend):
 * every GC in gcs[] must belong to `p` and have n_windows == nranks. A GC'd column's
 * indices are sent from the GC's buffer, and window j's compacted dictionary goes to rank
 * j in the same grouped send/recv. On the consumer the nranks received dictionaries are
 * concatenated in producer-rank order and the indices rebased, so the column is one
 * decodable dictionary array. n_gcs == 0 is dd_exchange_run; a dict32 column without a GC
 * crosses as plain i32 indices, as before. */
dd_status dd_exchange_run_gc(dd_comm *c, const dd_partitioner *p, dd_dict_gc *const *gcs,
                             int32_t n_gcs, void *stream, dd_exchanged **out);
/* received dictionary of a GC'd column (worker_service.rs:363-433 on the consumer side):
 * number of values (-1 when the column crossed without a GC), device i32[dict_n+1]
 * zero-based offsets, device value bytes, and host values-per-producer [nranks] */
int64_t dd_exchanged_dict_n(const dd_exchanged *e, int32_t col);
const int32_t *dd_exchanged_dict_offsets(const dd_exchanged *e, int32_t col);
const void *dd_exchanged_dict_bytes(const dd_exchanged *e, int32_t col);
dd_status dd_exchanged_dict_counts(const dd_exchanged *e, int32_t col,
                                   int64_t *vals_per_producer);

/* device helper, also used internally after the collective (worker_service.rs:363-433's
 * consumer half): out[i] = in[i] + bases[s] for seg_off[s] <= i < seg_off[s+1];
 * seg_off[0] == 0, seg_off[n_seg] == n. in == out is allowed. Synchronous. */
dd_status dd_dict_rebase(const int32_t *in, int64_t n, const int64_t *host_seg_off,
                         const int32_t *host_bases, int32_t n_seg, int32_t *out,
                         void *stream);

/* ---------------- view columns (Utf8View / BinaryView around the shuffle) ----------------
 * Besides dictionaries, the reference's pre-wire GC calls .gc() on StringViewArray and
 * BinaryViewArray so that their buffers hold only referenced bytes (garbage_collect_arrays,
 * src/protocol/grpc/worker_service.rs:408-433). The device's var-width form (dense offsets +
 * bytes) is that form already, so view columns get two steps around the unchanged
 * partitioner and exchange (normative): INGEST turns views + N data buffers
 * into an ordinary DD_DT_UTF8 column, EMIT turns a partition-major utf8 column into compact
 * per-window view arrays. Arrow view layout, little-endian, 16 bytes per row: i32 length;
 * length <= 12: the value, zero-padded; else a 4-byte prefix, i32 buffer_index, i32 offset. */

typedef struct dd_view_ingest dd_view_ingest; /* opaque, owns offsets + bytes */

/* worker_service.rs:408-433 (gc() of a view array, device side). views: device, 16-byte
 * aligned, 16 B x n_rows; validity: device unpacked u8 or NULL; data_bufs / data_buf_lens:
 * HOST arrays of n_bufs device pointers / byte lengths. Row i has len = view.length if
 * valid, else 0 (a null row's view is never interpreted); offsets = exclusive prefix sum of
 * len; bytes = the values in row order. Views may alias, overlap, repeat, and come in any
 * order. n_bufs == 0 (every valid row inline) and n_rows == 0 are legal. A valid row with
 * length < 0, or a long row with buffer_index outside [0, n_bufs), offset < 0 or offset +
 * length > data_buf_lens[buffer_index], is never dereferenced: DD_ERR_INVALID. Value bytes
 * above INT32_MAX: DD_ERR_UNSUPPORTED before any copy (chunk the rows). Synchronous: one
 * host sync reads the flag and the total and sizes the bytes. The result is an ordinary
 * DD_DT_UTF8 column: data = bytes, offsets, data_len. */
dd_status dd_view_ingest_run(const void *views, const uint8_t *validity, int64_t n_rows,
                             const void *const *data_bufs, const int64_t *data_buf_lens,
                             int32_t n_bufs, void *stream, dd_view_ingest **out);
/* worker_service.rs:408-433: device i32[n_rows+1], zero-based */
const int32_t *dd_view_ingest_offsets(const dd_view_ingest *g);
/* worker_service.rs:408-433: device value bytes, data_len of them */
const uint8_t *dd_view_ingest_bytes(const dd_view_ingest *g);
int64_t dd_view_ingest_data_len(const dd_view_ingest *g);
/* copy tier of the run: 1 = LDS-staged (DD_VIEW_LDS=1, read per call; a tile whose bytes
 * outgrow the image still copies directly), 0 = direct (the default: DD_VIEW_LDS unset or
 * 0, or every tile outgrew the image) */
int32_t dd_view_ingest_tier(const dd_view_ingest *g);
/* hipEvent durations of the run in ms: length pass, scan, copy */
dd_status dd_view_ingest_kernel_ms(const dd_view_ingest *g, float out_ms[3]);
void dd_view_ingest_destroy(dd_view_ingest *g);
/* rows per copy tile and bytes of the LDS image (tests size their edge cases from these) */
int32_t dd_view_tile_rows(void);
int32_t dd_view_image_bytes(void);

typedef struct dd_view_emit dd_view_emit; /* opaque: views + per-window data buffers */

/* worker_service.rs:408-433 (the arrays gc() would produce, per window). `col` is a UTF8
 * column of a run partitioner; windows as for the dictionary GC (n_windows divides P_total,
 * each window a contiguous partition range), anything else DD_ERR_INVALID. Window w's data
 * buffer is the concatenation, in row order, of its valid rows' values longer than 12
 * bytes. A null row emits 16 zero bytes; a valid short row its length and value; a valid
 * long row its length, 4-byte prefix, buffer_index 0 and offset = the long bytes of earlier
 * rows of the window. Any row slice of a window plus the window's buffer is a valid Arrow
 * view array. A window with more than INT32_MAX long bytes: DD_ERR_UNSUPPORTED.
 * Synchronous; `stream` must be ordered after the partitioner's run. The partitioner's own
 * output is not modified and must outlive the emit object. */
dd_status dd_view_emit_run(const dd_partitioner *p, int32_t col, uint32_t n_windows,
                           void *stream, dd_view_emit **out);
/* worker_service.rs:408-433: device 16 B x n_rows, partition-major */
const void *dd_view_emit_views(const dd_view_emit *g);
/* host prefix sums [n_windows+1] of the windows' data buffer sizes */
dd_status dd_view_emit_counts(const dd_view_emit *g, int64_t *long_byte_off);
/* device: window w's data buffer starts at long_byte_off[w] */
const uint8_t *dd_view_emit_bytes(const dd_view_emit *g);
/* hipEvent durations of the run in ms: scan, build, copy */
dd_status dd_view_emit_kernel_ms(const dd_view_emit *g, float out_ms[3]);
void dd_view_emit_destroy(dd_view_emit *g);

/* ---------------- coalesce (N->M task coalesce, no repartition) ----------------
 * Data plane for NetworkCoalesceExec (src/execution_plans/network_coalesce.rs:24-70):
 * consumer rank t receives the WHOLE partitioned output of every producer rank in its
 * contiguous group (task_group, :376-400; groups = ceil-split of nranks over
 * consumer_tasks). No repartition head (ProducerHead::None, :209-212). Reuses the
 * dd_exchanged result shape: producer-major concatenation, per-(producer, partition)
 * row counts. Ranks outside any group's producer set still participate (empty sends). */
dd_status dd_coalesce_run(dd_comm *c, const dd_partitioner *p, int32_t consumer_tasks,
                          void *stream, dd_exchanged **out);

/* ---------------- broadcast (build side of CollectLeft joins) ----------------
 * Replaces BroadcastExec's cache + NetworkBroadcastExec's per-consumer fetch
 * (src/execution_plans/broadcast.rs:24-28,163; network_broadcast.rs:245-266) with one
 * RCCL ncclBroadcast over xGMI: the root rank's device batch is replicated on every rank.
 * A size header is broadcast first so non-root ranks can allocate. */

typedef struct dd_bcast dd_bcast; /* opaque: replicated batch */

/* batch: the root's device batch (ignored on other ranks, may be NULL there) */
dd_status dd_broadcast_run(dd_comm *c, const dd_batch_desc *batch, int root, void *stream,
                           dd_bcast **out);
void dd_bcast_destroy(dd_bcast *b);
int64_t dd_bcast_n_rows(const dd_bcast *b);
int32_t dd_bcast_n_cols(const dd_bcast *b);
const void *dd_bcast_col_data(const dd_bcast *b, int32_t col);
const uint8_t *dd_bcast_col_validity(const dd_bcast *b, int32_t col);
const int32_t *dd_bcast_col_offsets(const dd_bcast *b, int32_t col);
dd_status dd_bcast_col_meta(const dd_bcast *b, int32_t col, int32_t *dtype,
                            int64_t *data_len);

/* ---------------- task cache (worker execute path) ----------------
 * Mirrors SetPlanRequest / ExecuteTaskRequest (src/protocol/worker_channel.rs:74-93,163-176)
 * and the worker's TaskData cache (src/worker/task_data.rs:16-29,104-116;
 * src/worker/worker_service.rs:12,31 — the moka TTI cache becomes an explicit
 * set/execute/drop lifecycle). The "plan" payload here is the shuffle-path plan descriptor:
 * a device batch + key columns + partitioning, i.e. exactly the producer head the reference
 * ships for this path. */

typedef struct dd_task_key {
    uint64_t query_id_hi, query_id_lo; /* Uuid (src/protocol/worker_channel.rs:57-65) */
    uint64_t stage_id;
    uint64_t task_number;
} dd_task_key;

dd_status dd_set_plan(const dd_task_key *key, const dd_batch_desc *batch,
                      const int32_t *key_cols, int32_t n_keys, uint32_t n_partitions);
/* Executes (or reuses) the cached task's partitioner and returns it; partition range
 * [part_lo, part_hi) mirrors ExecuteTaskRequest.target_partition_start/end. The returned
 * partitioner is owned by the cache; do not destroy. Lifetime: concurrent
 * set_plan/execute/drop calls on the same key are safe (entries are refcounted and an
 * in-flight execute pins its entry), but the pointer *out refers to the cache entry as
 * of this call — it is invalidated by a later dd_drop_task or dd_set_plan on the same
 * key, so callers must not use it past either (the reference's worker has the same
 * contract: task state lives until the TTI cache evicts it, task_data.rs:16-29). */
dd_status dd_execute_task(const dd_task_key *key, uint32_t part_lo, uint32_t part_hi,
                          void *stream, dd_partitioner **out);
dd_status dd_drop_task(const dd_task_key *key); /* task cleanup (stateful_data_cleanup) */

/* ---------------- protobuf plan/stage wire payload (dd_proto.cpp) ----------------
 * The reference's own wire shapes at this boundary (field numbers cited in
 * dd_proto.cpp): SetPlanRequest / ExecuteTaskRequest / TaskKey
 * (src/protocol/grpc/worker.proto:84-110,134-155,171-179) with the producer_head's
 * RepartitionExecHead carrying a datafusion-proto `Partitioning` message
 * (worker.proto:167-170; datafusion-proto 55.0.0, Cargo.lock pin). A Rust shim passes
 * the prost-encoded request bytes straight through — no re-encoding. */

enum { DD_HEAD_NONE = 0, DD_HEAD_BROADCAST = 1, DD_HEAD_REPARTITION = 2 };

/* decode a datafusion-proto Partitioning (hash exprs must be columns) */
dd_status dd_decode_partitioning(const uint8_t *buf, int64_t len, int32_t *key_cols,
                                 int32_t max_keys, int32_t *n_keys,
                                 uint32_t *n_partitions);
/* decode an ExecuteTaskRequest: task key, partition range, producer head (repartition
 * heads also fill key_cols/n_keys/n_partitions; broadcast fills n_partitions) */
dd_status dd_decode_execute_task(const uint8_t *buf, int64_t len, dd_task_key *key,
                                 uint64_t *part_start, uint64_t *part_end,
                                 int32_t *head_kind, int32_t *key_cols, int32_t max_keys,
                                 int32_t *n_keys, uint32_t *n_partitions);
/* decode a SetPlanRequest; *plan_proto is a borrowed view into buf */
dd_status dd_decode_set_plan(const uint8_t *buf, int64_t len, dd_task_key *key,
                             uint64_t *task_count, const uint8_t **plan_proto,
                             int64_t *plan_len);
/* register a plan under the TaskKey decoded from a prost-encoded SetPlanRequest; the
 * device batch is what the subplan below the network boundary produces (the shim
 * materializes it — the plan_proto subplan itself stays host-side per the tier) */
dd_status dd_set_plan_proto(const uint8_t *set_plan_pb, int64_t len,
                            const dd_batch_desc *batch);
/* execute from a prost-encoded ExecuteTaskRequest: decodes the RepartitionExecHead,
 * lazily inserts the head (TaskData::plan / ProducerHead::insert semantics) and runs
 * the partition kernels; same returned-pointer lifetime as dd_execute_task */
dd_status dd_execute_task_proto(const uint8_t *execute_task_pb, int64_t len, void *stream,
                                dd_partitioner **out);
dd_status dd_drop_task_proto(const uint8_t *task_key_pb, int64_t len);

/* ---------------- Arrow IPC + lz4 wire format (dd_wire.cpp) ----------------
 * The on-wire batch encoding for cross-node (non-xGMI) hops, reimplementing the
 * reference's Flight encode/decode (src/protocol/grpc/worker_service.rs:363-433 /
 * worker_client.rs:302): Apache Arrow IPC STREAMING format, MetadataVersion V5, with
 * per-buffer lz4-frame BodyCompression (the reference's default,
 * distributed_config.rs:36-38). Zero-column batches (row count, no fields) round-trip —
 * the edge case the reference wire-tests pin (tests/empty_columns_between_workers.rs).
 * Validity and bool data are unpacked u8 at this ABI (packed to Arrow bitmaps on the
 * wire). Host memory only; this is the serialization layer, not the device path. */

typedef struct dd_ipc_field {
    int32_t dtype;    /* dd_dtype (DICT32 unsupported on the wire: indices + values
                         cross via arrow_boundary materialization) */
    const char *name; /* optional */
    int32_t nullable;
} dd_ipc_field;

typedef struct dd_ipc_array {
    const void *data;        /* fixed: values (bool: unpacked u8); utf8: byte buffer */
    int64_t data_len;        /* utf8: byte length; reader fills for fixed too */
    const uint8_t *validity; /* unpacked u8, NULL = all valid */
    int64_t null_count;
    const int32_t *offsets;  /* utf8: [n_rows+1] */
} dd_ipc_array;

typedef struct dd_ipc_writer dd_ipc_writer;
typedef struct dd_ipc_reader dd_ipc_reader;

/* DD_DT_DEC128 fields: DD_ERR_UNSUPPORTED (dd_ipc_field carries no precision and scale;
 * decimals on the cross-node wire are out of scope). */
dd_status dd_ipc_writer_create(const dd_ipc_field *fields, int32_t n_fields,
                               int32_t use_lz4, dd_ipc_writer **out);
dd_status dd_ipc_writer_batch(dd_ipc_writer *w, int64_t n_rows, const dd_ipc_array *cols);
/* appends the EOS marker (idempotent) and exposes the stream; owned by the writer */
dd_status dd_ipc_writer_finish(dd_ipc_writer *w, const uint8_t **data, int64_t *len);
void dd_ipc_writer_destroy(dd_ipc_writer *w);

dd_status dd_ipc_reader_create(const uint8_t *data, int64_t len, dd_ipc_reader **out);
int32_t dd_ipc_reader_n_fields(const dd_ipc_reader *r);
int32_t dd_ipc_reader_n_batches(const dd_ipc_reader *r);
int32_t dd_ipc_reader_field_dtype(const dd_ipc_reader *r, int32_t i);
const char *dd_ipc_reader_field_name(const dd_ipc_reader *r, int32_t i);
int64_t dd_ipc_reader_batch_rows(const dd_ipc_reader *r, int32_t b);
/* pointers into reader-owned memory (decompressed; validity/bool unpacked to u8) */
dd_status dd_ipc_reader_batch_col(const dd_ipc_reader *r, int32_t b, int32_t c,
                                  dd_ipc_array *out);
void dd_ipc_reader_destroy(dd_ipc_reader *r);

/* ---------------- partial aggregation (below the shuffle) ----------------
 * Mirrors the partial-reduce pass (src/distributed_planner/
 * partial_reduce_below_network_shuffles.rs; `distributed.partial_reduce`,
 * distributed_config.rs:50-54): a mode=Partial aggregate run before dd_partition so the
 * exchange moves per-group partials. May emit duplicate groups (one per block); the
 * downstream final aggregate merges them. Up to 4 key columns: fixed-width (u8, i16,
 * i32, i64, f32, f64, bool) or dict32 grouped BY INDEX (utf8 keys are unsupported). Float
 * keys are canonicalised like the row hash (-0.0 -> +0.0, every NaN -> one quiet NaN).
 * Duplicate dictionary values under different indices yield separate partial groups,
 * which the final aggregate merges by value. Up to 8 aggregates, ops below.
 *
 * Aggregate contract (every op but COUNT skips NULL inputs):
 *  - Each output row carries, per aggregate, the NON-NULL INPUT COUNT `nn`
 *    (dd_reducer_fetch_nn). The final merge sums nn per group; a total of 0 means the
 *    merged aggregate is SQL NULL. The value slot of a partial with nn == 0 holds the op
 *    identity and must be skipped by a min/max merge.
 *  - SUM_I64 wraps modulo 2^64 (two's complement), like the u64 atomic add behind it.
 *  - MIN_F64 / MAX_F64 order by IEEE-754 totalOrder on the bit pattern:
 *    -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN. A sign-set NaN (e.g. the
 *    0xfff8... that x86 produces for inf - inf) therefore sorts BELOW -inf; only a
 *    sign-clear NaN sorts above +inf. NaN payloads and the sign of zero are preserved.
 *  - SUM_F64 adds in an unspecified order (floating-point atomics).
 *  - SUM_DEC128 sums a DD_DT_DEC128 column exactly: the state is a 128-bit
 *    two's-complement sum that wraps modulo 2^128, low half in the value slot (bit-cast,
 *    like the integer ops), high half from dd_reducer_fetch_hi. A partial with nn == 0
 *    holds (0, 0). Precision and scale are schema: the result type
 *    Decimal128(min(38, p + 10), s) is the caller's business. avg(dec128) is this op plus
 *    its nn; there is no separate avg op.
 *  - Not offered: min / max of a dec128 column. gfx950 has no 128-bit LDS atomic, and a
 *    per-slot lock is a hang risk on hardware without independent thread scheduling (the
 *    reason the probe loop never spins). dec128 keys are not offered either. */

typedef struct dd_reducer dd_reducer;

#define DD_AGG_SUM_F64 0 /* sum of an f64 column */
#define DD_AGG_COUNT 1   /* count(*): every row, agg_col ignored; nn == count, never NULL */
#define DD_AGG_SUM_I64 2 /* wrapping sum of an i64 column */
#define DD_AGG_MIN_F64 3 /* totalOrder min / max of an f64 column */
#define DD_AGG_MAX_F64 4
#define DD_AGG_MIN_I64 5 /* signed min / max of an i64 column */
#define DD_AGG_MAX_I64 6
#define DD_AGG_SUM_DEC128 7 /* exact wrapping 128-bit sum of a dec128 column */

/* Launch geometry dd_partial_reduce_run uses for an n_rows batch whose plan has at most 4
 * aggregates and no SUM_DEC128: LDS table slots per block, probe limit before a row
 * spills as a singleton group, block count and rows per block (the last block may be
 * ragged or empty). Needs no device. */
dd_status dd_partial_reduce_geometry(int64_t n_rows, int32_t *table_slots,
                                     int32_t *probe_limit, int64_t *nblocks,
                                     int64_t *chunk_rows);

/* The same for any plan (n_keys 1..4, agg_ops[n_aggs] with n_aggs 1..8). kernel: 0 = the
 * 4-aggregate kernel (at most 4 aggregates, none of them SUM_DEC128; the numbers are those
 * of dd_partial_reduce_geometry), 1 = the wide kernel, whose table is sized for the plan:
 * table_slots is a power of two in [512, 1024] and lds_bytes <= 163840. The home slot of
 * a row is max(row hash, 1) % table_slots in both. Needs no device. */
dd_status dd_partial_reduce_plan_geometry(int64_t n_rows, int32_t n_keys,
                                          const int32_t *agg_ops, int32_t n_aggs,
                                          int32_t *kernel, int32_t *table_slots,
                                          int32_t *probe_limit, int32_t *block_threads,
                                          int32_t *lds_bytes, int64_t *nblocks,
                                          int64_t *chunk_rows);

/* 1..8 aggregates. DD_ERR_UNSUPPORTED, with a message that names the cause, for: a
 * DD_DT_DEC128 key; any op but SUM_DEC128 on a DD_DT_DEC128 column; SUM_DEC128 on any
 * other column; more than 8 aggregates. The wide kernel's wave aggregation is chosen by
 * DD_REDUCE_WAVEAGG=0/1, read per call. */
dd_status dd_partial_reduce_run(const dd_batch_desc *batch, const int32_t *key_cols,
                                int32_t n_keys, const int32_t *agg_cols,
                                const int32_t *agg_ops, int32_t n_aggs, void *stream,
                                dd_reducer **out);
int64_t dd_reducer_n_rows(const dd_reducer *r);
float dd_reducer_kernel_ms(const dd_reducer *r); /* reduce-kernel time of the last run */
/* host_keys[n][n_keys] canonical 64-bit key bits; host_keynull[n] per-key null bitmask;
 * host_aggs[n][n_aggs] (i64 sums / counts bit-cast into the double slot) */
dd_status dd_reducer_fetch(const dd_reducer *r, uint64_t *host_keys, uint32_t *host_keynull,
                           double *host_aggs);
/* host_nn[n][n_aggs] non-null input counts per aggregate: the final merge sums them and
 * emits NULL when the total is 0 (DataFusion: SUM/MIN/MAX over an all-null group is NULL,
 * not the op identity; COUNT counts rows and is never NULL) */
dd_status dd_reducer_fetch_nn(const dd_reducer *r, uint64_t *host_nn);
/* host_hi[n][n_aggs]: the high 64 bits of each SUM_DEC128 slot (host_aggs holds the low
 * 64), 0 for every other op */
dd_status dd_reducer_fetch_hi(const dd_reducer *r, uint64_t *host_hi);
/* which kernel ran (as dd_partial_reduce_plan_geometry names them) and the wave-aggregation
 * setting it ran with (0 or 1; always 0 for kernel 0) */
int32_t dd_reducer_kernel(const dd_reducer *r);
int32_t dd_reducer_waveagg(const dd_reducer *r);
void dd_reducer_destroy(dd_reducer *r);

/* ---------------- final aggregation (above the shuffle) ----------------
 * The other half of the two-phase aggregate: the AggregateExec mode=FinalPartitioned that
 * sits on RepartitionExec Hash([l_returnflag, l_linestatus], 6) in the q1 plan of
 * tests/tpch_plans_test.rs. Input: a device batch of PARTIAL STATES (what
 * dd_partial_reduce_run produced and the shuffle carried) plus a segment layout; output:
 * exactly one row per (partition, group), partition-major. DESIGN.md §18 is normative.
 *
 * Segment layout (host arrays): seg_offsets[n_segs + 1] non-decreasing row offsets from 0
 * to n_rows; seg_part[n_segs] the partition of each segment, in [0, n_parts). The rows of
 * all segments with one partition id form that partition. A dd_partitioner output is
 * n_segs = P, seg_part = identity; a dd_exchanged window (producer-major, then
 * partition-major per producer) is n_segs = producers * parts, seg_part[s] = s % parts;
 * n_segs = n_parts = 1 is a plain global group-by.
 *
 * Groups are formed WITHIN a partition (one key in two partitions gives two groups) by the
 * identity dd_reducer_fetch reports: canonical u64 key bits plus the key-null mask; a NULL
 * component has bits 0 and its mask bit set. Keys: 1..4 of u8, bool, i16, i32, i64, f32, f64.
 *
 * Aggregates: 1..8 of (state_col, op, nn_col), DD_AGG_* read as merge ops. COUNT adds an i64
 * column of partial counts (nn_col ignored, pass -1; nn is the merged count); SUM_I64 wraps
 * modulo 2^64; SUM_F64 adds in an unspecified order; MIN / MAX as in the partial aggregate
 * (signed; totalOrder on the bit pattern, payloads preserved); SUM_DEC128 adds (lo, hi)
 * modulo 2^128. nn_col is an i64 column of non-null input counts: a partial with nn == 0 is
 * skipped, nn is summed per group, and a total of 0 means SQL NULL (value unspecified).
 * Validity buffers of state and nn columns are ignored, as are columns the plan does not
 * name. The order of groups inside a partition is unspecified.
 *
 * DD_ERR_UNSUPPORTED, with a message that names the cause: a dict32 (rebased indices after
 * a GC'd exchange must be merged by value), utf8 or dec128 key; a state or nn column of the
 * wrong dtype for its op; more than 8 aggregates or 4 keys. DD_ERR_INVALID: a malformed
 * segment layout, a column index out of range, n_rows >= 2^31. n_rows == 0 succeeds with
 * zero groups. Synchronous on `stream`. */

typedef struct dd_finalizer dd_finalizer;

/* seam: the final aggregate above RepartitionExec in the q1 plan (tests/tpch_plans_test.rs) */
dd_status dd_final_merge_run(const dd_batch_desc *batch, const int32_t *key_cols,
                             int32_t n_keys, const int32_t *state_cols,
                             const int32_t *agg_ops, const int32_t *nn_cols, int32_t n_aggs,
                             const int64_t *seg_offsets, const int32_t *seg_part,
                             int32_t n_segs, int32_t n_parts, void *stream,
                             dd_finalizer **out);
/* same seam: output rows of the final aggregate, one per (partition, group) */
int64_t dd_finalizer_n_groups(const dd_finalizer *f);
/* same seam: host_out[n_parts + 1], partition p's groups are rows [out[p], out[p + 1]) --
 * the output partitioning the FinalPartitioned aggregate keeps from RepartitionExec */
dd_status dd_finalizer_group_offsets(const dd_finalizer *f, int64_t *host_out);
/* same seam: the merged rows in the shapes of dd_reducer_fetch: host_keys[n][n_keys],
 * host_keynull[n], host_aggs[n][n_aggs] (integers bit-cast; min / max as value bits) */
dd_status dd_finalizer_fetch(const dd_finalizer *f, uint64_t *host_keys,
                             uint32_t *host_keynull, double *host_aggs);
/* same seam: host_nn[n][n_aggs] summed non-null counts; 0 = the aggregate is SQL NULL */
dd_status dd_finalizer_fetch_nn(const dd_finalizer *f, uint64_t *host_nn);
/* same seam: host_hi[n][n_aggs] high 64 bits of each SUM_DEC128, 0 for every other op */
dd_status dd_finalizer_fetch_hi(const dd_finalizer *f, uint64_t *host_hi);
/* same seam: hipEvent times of the run in ms: out3 = [claim, scan, merge] */
dd_status dd_finalizer_kernel_ms(const dd_finalizer *f, float *out3);
/* same seam: the merged rows as typed DEVICE columns, for a further operator on the device
 * (DESIGN.md §18.6). Column order: n_keys key columns, each in its input dtype from the
 * canonical key bits (so a float key comes out canonicalised: +0.0 for -0.0, one quiet NaN)
 * with a validity buffer from keynull; n_aggs aggregate columns (COUNT, SUM_I64, MIN_I64,
 * MAX_I64: i64; SUM_F64, MIN_F64, MAX_F64: f64; SUM_DEC128: dec128 = (lo, hi)) with a
 * validity buffer nn != 0, none for COUNT; then, when with_nn, n_aggs i64 nn columns without
 * validity. key_dtypes / agg_ops are the run's (the finalizer keeps no plan); counts that
 * differ from the run's are DD_ERR_INVALID. Rows are the groups in dd_finalizer_fetch's
 * order, partition-major by dd_finalizer_group_offsets. A second call replaces the columns.
 * Synchronous on `stream`. */
dd_status dd_finalizer_columns(dd_finalizer *f, const int32_t *key_dtypes, int32_t n_keys,
                               const int32_t *agg_ops, int32_t n_aggs, int32_t with_nn,
                               void *stream);
/* same seam: columns built by dd_finalizer_columns (0 before it ran) */
int32_t dd_finalizer_n_cols(const dd_finalizer *f);
/* same seam: dd_dtype of column i */
int32_t dd_finalizer_col_dtype(const dd_finalizer *f, int32_t i);
/* same seam: device values of column i, owned by the finalizer; NULL at zero groups */
const void *dd_finalizer_col_data(const dd_finalizer *f, int32_t i);
/* same seam: device validity bytes of column i, NULL when it has none */
const uint8_t *dd_finalizer_col_validity(const dd_finalizer *f, int32_t i);
/* same seam: frees the merged rows and their columns */
void dd_finalizer_destroy(dd_finalizer *f);

/* ---------------- partitioned hash join (above two co-partitioned shuffles) ----------------
 * HashJoinExec mode=Partitioned on two RepartitionExec Hash(keys, P) inputs that share P:
 * tests/join.rs:116,197,279, tests/tpch_plans_test.rs:59,239,867 (Inner, LeftSemi, Left) and
 * tests/multi_task_collect_join_repros.rs:68 (LeftSemi). DESIGN.md §19 is normative.
 *
 * Two device batches, each with a segment layout in the final aggregation's form (above);
 * n_segs may differ, n_parts must be equal. "Left" is the BUILD side, as in HashJoinExec.
 * Partition p of the build side joins partition p of the probe side and nothing else;
 * co-partitioning is the caller's contract and is not verified.
 *
 * Keys: 1..4 columns per side, pairwise of one dtype out of u8, bool, i16, i32, i64, nullable;
 * equality on the raw value; a row with a NULL in any key component matches nothing.
 * INNER emits one row per matching (build row, probe row) pair; LEFT_SEMI / LEFT_ANTI the
 * build rows with / without a match, RIGHT_SEMI / RIGHT_ANTI the probe rows (a NULL-key row
 * is without a match). Output rows follow the row order of the EMITTING side (probe for
 * INNER and RIGHT_*, build for LEFT_*) and keep its segments: the same seg_part, new
 * seg_offsets. The matches of one probe row are adjacent, in an unspecified order.
 *
 * Output columns: build_proj then probe_proj (column indices; the plan's projection=[...]),
 * fixed-width dtypes of element size 1, 2, 4, 8 or 16; an output column has a validity
 * buffer exactly when its source has one; values and validity bytes are copied bit-exactly.
 * A semi / anti join takes the emitting side's list only.
 *
 * DD_ERR_UNSUPPORTED, with a message that names the cause: f32 / f64 keys (Arrow compares
 * float join keys by total order, the key bits here canonicalise -0.0 and NaN), dict32, utf8
 * or dec128 keys; a var-width or dict32 column in a projection; more than 4 keys; LEFT, RIGHT
 * and FULL; and, after the count pass, an output of 2^31 rows or more (chunk the probe
 * side; nothing is emitted). DD_ERR_INVALID: key dtypes that differ pairwise, unequal
 * n_parts, a malformed layout, a column index out of range, the other side's list on a semi
 * / anti join, n_rows >= 2^31 on either side. An empty side or an empty result succeeds with
 * zero rows and a valid layout. Synchronous on `stream`. */

#define DD_JOIN_INNER 0
#define DD_JOIN_LEFT_SEMI 1
#define DD_JOIN_LEFT_ANTI 2
#define DD_JOIN_RIGHT_SEMI 3
#define DD_JOIN_RIGHT_ANTI 4
#define DD_JOIN_LEFT 5  /* the outer joins: refused here by name, dd_hash_join_outer_run's */
#define DD_JOIN_RIGHT 6
#define DD_JOIN_FULL 7

typedef struct dd_joiner dd_joiner; /* opaque: pair indices and gathered columns */

/* seam: HashJoinExec mode=Partitioned above two RepartitionExec Hash(keys, P)
 * (tests/join.rs:116, tests/tpch_plans_test.rs:59) */
dd_status dd_hash_join_run(const dd_batch_desc *build, const int32_t *build_keys,
                           const dd_batch_desc *probe, const int32_t *probe_keys,
                           int32_t n_keys, int32_t join_type,
                           const int64_t *build_seg_offsets, const int32_t *build_seg_part,
                           int32_t build_n_segs, int32_t build_n_parts,
                           const int64_t *probe_seg_offsets, const int32_t *probe_seg_part,
                           int32_t probe_n_segs, int32_t probe_n_parts,
                           const int32_t *build_proj, int32_t n_build_proj,
                           const int32_t *probe_proj, int32_t n_probe_proj, void *stream,
                           dd_joiner **out);
/* The outer joins: LEFT, RIGHT and FULL. dd_hash_join_run's parameters, its
 * keys, layouts, projections and refusals; the five other types are refused here with
 * DD_ERR_INVALID (they are dd_hash_join_run's), as is a type outside 0..7.
 *
 * RIGHT: every inner pair, plus one row per probe row without a match with the build side
 * NULL. LEFT: every inner pair, plus one row per build row no probe row matched with the
 * probe side NULL. FULL: both. A NULL-key row is a row without a match.
 *
 * The output has TWO SECTIONS of segments. First the probe side's probe_n_segs segments with
 * its seg_part: rows in probe row order, the matches of one probe row adjacent in an
 * unspecified order; under RIGHT / FULL a probe row without a match stands there once as
 * (DD_JOIN_NONE, row), under LEFT it contributes nothing. Then, for LEFT and FULL only, the
 * build side's build_n_segs segments with its seg_part: segment probe_n_segs + s holds the
 * unmatched rows of build segment s in build row order as (row, DD_JOIN_NONE) -- where
 * HashJoinExec emits them, after the partition's probe stream is exhausted. dd_joiner_n_segs
 * is probe_n_segs (RIGHT) or probe_n_segs + build_n_segs; n_parts is unchanged.
 *
 * build_idx and probe_idx are both always present. Every output column of a NULL-extended
 * side (probe for LEFT, build for RIGHT, both for FULL) has a validity buffer: the source's
 * byte on a real row (1 if the source has none), 0 on a DD_JOIN_NONE row, whose value bytes
 * are all zero. Columns of the other side have validity exactly when their source has.
 * The total over both sections is range-checked after the count pass as above. RIGHT with
 * an empty probe side and any type with both sides empty succeed with zero rows. */

#define DD_JOIN_NONE 0xffffffffu /* build_idx / probe_idx: this side of the row is absent */

/* seam: HashJoinExec mode=Partitioned, join_type=Left above two NetworkShuffleExec (TPC-H
 * q13, tests/tpch_plans_test.rs:867); Right / Full in tests/tpcds_plans_test.rs */
dd_status dd_hash_join_outer_run(const dd_batch_desc *build, const int32_t *build_keys,
                                 const dd_batch_desc *probe, const int32_t *probe_keys,
                                 int32_t n_keys, int32_t join_type,
                                 const int64_t *build_seg_offsets,
                                 const int32_t *build_seg_part, int32_t build_n_segs,
                                 int32_t build_n_parts, const int64_t *probe_seg_offsets,
                                 const int32_t *probe_seg_part, int32_t probe_n_segs,
                                 int32_t probe_n_parts, const int32_t *build_proj,
                                 int32_t n_build_proj, const int32_t *probe_proj,
                                 int32_t n_probe_proj, void *stream, dd_joiner **out);
/* same seam: output segments: dd_joiner_seg_offsets copies this many + 1 entries */
int32_t dd_joiner_n_segs(const dd_joiner *j);
/* same seam: output rows of the HashJoinExec */
int64_t dd_joiner_n_rows(const dd_joiner *j);
/* same seam: host_out[n_segs + 1] of the emitting side: output segment s is rows
 * [out[s], out[s + 1]) -- the partitioning the join keeps from its RepartitionExec inputs */
dd_status dd_joiner_seg_offsets(const dd_joiner *j, int64_t *host_out);
/* same seam: device u32[n_rows] build row of each output row (the join's left indices);
 * NULL for RIGHT_SEMI / RIGHT_ANTI */
const uint32_t *dd_joiner_build_idx(const dd_joiner *j);
/* same seam: device u32[n_rows] probe row of each output row (the join's right indices);
 * NULL for LEFT_SEMI / LEFT_ANTI */
const uint32_t *dd_joiner_probe_idx(const dd_joiner *j);
/* same seam: device values of output column i (build_proj first, then probe_proj): the
 * HashJoinExec's projected output batch, columnar on the device for the next operator */
const void *dd_joiner_col_data(const dd_joiner *j, int32_t i);
/* same seam: device validity bytes of output column i, NULL when its source has none */
const uint8_t *dd_joiner_col_validity(const dd_joiner *j, int32_t i);
/* same seam: hipEvent times of the run in ms: out5 = [build, count, scan, emit, gather] */
dd_status dd_joiner_kernel_ms(const dd_joiner *j, float *out5);
/* same seam: frees the join's output */
void dd_joiner_destroy(dd_joiner *j);

/* ---------------- sort / top-k per partition (above the shuffle) ----------------
 * The SortExec: expr=[...], preserve_partitioning=[true] (TopK(fetch=k) under a LIMIT) that
 * closes every task of the TPC-H plans: tests/tpch_plans_test.rs:30 (q1), :180 (q3), :853
 * (q13), :1113 (q18), above AggregateExec mode=FinalPartitioned. DESIGN.md §22 is normative;
 * datafusion_distributed_amd/sortref.py states the same rules in Python.
 *
 * Input: a device batch plus a segment layout in the final aggregation's form (above). A
 * row's INPUT RANK is its row index. Keys: 1..4 of (column, flags), flags = DD_SORT_DESC |
 * DD_SORT_NULLS_FIRST, the two independent; dtypes u8, bool, i16, i32, i64, f32, f64, dec128.
 * Order of values: u8 / bool unsigned; integers signed; f32 / f64 IEEE-754 totalOrder on the
 * RAW bit pattern (-0.0 < +0.0, a sign-clear NaN above +inf, a sign-set NaN below -inf, NaN
 * payloads by their bits: arrow-rs total_cmp; nothing is canonicalised); dec128 signed 128-bit.
 * NULLs are equal to each other and their value bytes are never read. DESC reverses the
 * values only; NULLS_FIRST alone places the NULLs.
 *
 * Output: one segment per partition (n_parts segments, seg_part = identity), partition-major;
 * partition p holds its rows in key order, ties in input rank (the sort is STABLE, so every
 * bit of the output is determined). fetch = k >= 0 keeps the first min(k, rows) rows of each
 * partition, fetch = -1 all; fetch = 0 is a valid empty result. The result holds perm (the
 * source row of each output row), the proj columns gathered on the device (fixed-width dtypes
 * of 1, 2, 4, 8 or 16 byte elements; validity exactly when the source has it) and the new
 * seg_offsets. The SortPreservingMergeExec(fetch=k) on top of the plan is this entry again
 * over the result with the one-partition layout ([0, n_out], [0], 1): its stable tie order is
 * partition order, the order a merge takes ties in.
 *
 * Every check runs before any device work. DD_ERR_UNSUPPORTED: a dict32 key (dictionary
 * index order is not value order), a utf8 / utf8view key, a utf8 / dict32 column in proj.
 * DD_ERR_INVALID: 0 keys or more than 4, a column index out of range, unknown flag bits,
 * fetch < -1, a malformed layout (dd_final_merge_run's checks), n_rows >= 2^31 (perm holds
 * 32-bit row ids). n_rows == 0 succeeds with empty segments. DD_SORT_SKIP=0 (environment,
 * read per call) runs every planned radix pass instead of dropping those whose digit is the
 * same in all rows; results are bit-identical. Synchronous on `stream`. */

#define DD_SORT_DESC 1
#define DD_SORT_NULLS_FIRST 2

typedef struct dd_sorter dd_sorter; /* opaque: perm, gathered columns, segment offsets */

/* seam: SortExec preserve_partitioning=[true] above AggregateExec mode=FinalPartitioned
 * (tests/tpch_plans_test.rs:180, :1113); with the one-partition layout, the
 * SortPreservingMergeExec above it (:175, :1109) */
dd_status dd_sort_run(const dd_batch_desc *batch, const int32_t *key_cols,
                      const int32_t *key_flags, int32_t n_keys, const int32_t *proj_cols,
                      int32_t n_proj, const int64_t *seg_offsets, const int32_t *seg_part,
                      int32_t n_segs, int32_t n_parts, int64_t fetch, void *stream,
                      dd_sorter **out);
/* same seam: output rows of the SortExec, after fetch */
int64_t dd_sorter_n_rows(const dd_sorter *s);
/* same seam: host_out[n_parts + 1]: partition p's rows are [out[p], out[p + 1]) */
dd_status dd_sorter_seg_offsets(const dd_sorter *s, int64_t *host_out);
/* same seam: device u32[n_rows], the input row of each output row; NULL at zero rows */
const uint32_t *dd_sorter_perm(const dd_sorter *s);
/* same seam: device values of projected column i, in output order; NULL at zero rows */
const void *dd_sorter_col_data(const dd_sorter *s, int32_t i);
/* same seam: device validity bytes of projected column i, NULL when its source has none */
const uint8_t *dd_sorter_col_validity(const dd_sorter *s, int32_t i);
/* same seam: out4 = [radix passes planned from the key dtypes and the layout, passes run
 * after the census dropped the constant digits, rows per scatter tile, 64-bit words per row
 * (ordered key words + the partition / null-rank word)] */
dd_status dd_sorter_info(const dd_sorter *s, int32_t *out4);
/* same seam: hipEvent times in ms: out4 = [encode + census, passes, segment output, gather] */
dd_status dd_sorter_kernel_ms(const dd_sorter *s, float *out4);
/* same seam: frees the sort's output */
void dd_sorter_destroy(dd_sorter *s);

/* ---------------- device helpers (harness convenience; not part of the seam) ------- */
dd_status dd_dev_alloc(int64_t bytes, void **out);
dd_status dd_dev_free(void *p);
dd_status dd_memcpy_h2d(void *dst, const void *src, int64_t bytes);
/* asynchronous on `stream`; truly overlapped only when `src` is pinned host memory, and
 * `src` must stay valid and unchanged until the stream has passed the copy */
dd_status dd_memcpy_h2d_async(void *dst, const void *src, int64_t bytes, void *stream);
dd_status dd_memcpy_d2h(void *dst, const void *src, int64_t bytes);
dd_status dd_memcpy_d2d(void *dst, const void *src, int64_t bytes);
dd_status dd_device_sync(void);

#ifdef __cplusplus
}
#endif

#endif /* DD_SHUFFLE_H */
