/* dd_internal.h — shared between dd_kernels.hip and dd_host.cpp (not part of the ABI). */

#ifndef DD_INTERNAL_H
#define DD_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define DD_MAX_P 2048
#define WAVES_PER_BLOCK_H 4 /* must match WAVES_PER_BLOCK in dd_kernels.hip */
#define DD_KMAX_COLS 24
#define DD_KMAX_KEYS 8
#define DD_KMAX_VAR 4
#define DD_SCAN_RANGES 64
#define DD_STAGE_MAXC 8 /* staged-path column cap (register prefetch arrays) */

/* partial-reduce geometry (dd_reduce.hip kernel + dd_host.cpp launch/allocation; reported
 * by dd_partial_reduce_geometry so tests never mirror these literals) */
#define DD_R_CAP 1024        /* LDS table slots per block */
#define DD_R_PROBE 64        /* bounded linear probe; then spill */
#define DD_R_BLOCK_ROWS 16384 /* target rows per block */
#define DD_R_MIN_BLOCKS 8
#define DD_R_MAX_BLOCKS 1024

/* wide partial reduce (k_partial_reduce_wide): up to DD_RW_MAX_AGGS
 * aggregates, exact dec128 sums; the table lives in dynamic LDS sized per plan and is
 * reported by dd_partial_reduce_plan_geometry */
#define DD_R_NARROW_AGGS 4    /* k_partial_reduce's aggregate cap */
#define DD_RW_MAX_AGGS 8
#define DD_RW_THREADS 1024    /* one table serves 16 waves */
#define DD_RW_MAX_SLOTS 1024  /* table slots: a power of two in [MIN, MAX] */
#define DD_RW_MIN_SLOTS 512
#define DD_RW_PROBE 64
#define DD_RW_LDS_LIMIT 163840 /* LDS one workgroup may hold on gfx950 */
#define DD_RW_BLOCK_ROWS 8192  /* target rows per block: 8 per thread */
#define DD_RW_MIN_BLOCKS 8
#define DD_RW_MAX_BLOCKS 2048
#define DD_RW_PEEL_MIN 8       /* wave aggregation: smallest lane group worth a reduce */

/* final merge above the shuffle (dd_final.hip) */
#define DD_F_MAX_AGGS 8
#define DD_F_THREADS 256
#define DD_F_BLOCK_ROWS 2048  /* claim: rows per block, so the staged segment offsets are
                                 read once per 2048 rows */
#define DD_F_LDS_SEGS 1024    /* claim: segment offsets staged in LDS up to this many */
#define DD_F_MIN_SLOTS 64     /* smallest claim-table region of a partition */
#define DD_F_SCAN_TILE 1024   /* scan: table entries per block, 4 per thread */
#define DD_F_EMPTY 0xffffffffu

/* hash join above two shuffles (dd_join.hip); the table, the segment search
 * and the block geometry are the final merge's (DD_F_*) */
#define DD_J_SCAN_TILE 1024    /* scan: counts per block, 4 per thread */
#define DD_J_SUMS_THREADS 1024 /* scan: tile sums per round of the one-block middle pass */

/* sort / top-k above the shuffle (dd_sort.hip); the segment search and its
 * LDS staging are the final merge's (DD_F_LDS_SEGS) */
#define DD_S_MAX_KEYS 4
#define DD_S_MAX_WORDS 9       /* four dec128 keys give 8 value words; + the meta word */
#define DD_S_THREADS 256
#define DD_S_TILE 2048         /* hist / scatter: rows per tile = 4 waves x 8 steps x 64 */
#define DD_S_ENC_ROWS 16384    /* encode: rows per block, so a block's census flush of at
                                  most 2048 bins per word is spread over 16384 rows */
#define DD_S_SCAN_TILE 1024    /* scan: histogram entries per block, 4 per thread */
#define DD_S_SUMS_THREADS 1024 /* scan: tile sums per round of the one-block middle pass */

/* dtype codes mirror dd_dtype in include/dd_shuffle.h */
enum {
    DD_KDT_U8 = 1,
    DD_KDT_I16 = 2,
    DD_KDT_I32 = 3,
    DD_KDT_I64 = 4,
    DD_KDT_F32 = 5,
    DD_KDT_F64 = 6,
    DD_KDT_BOOL = 7,
    DD_KDT_UTF8 = 8,
    DD_KDT_DICT32 = 9,
    DD_KDT_DEC128 = 10, /* 16-byte value: hashes as two u64 halves (lo, hi), DESIGN.md §16 */
    DD_KDT_VARLEN = 100, /* synthetic (staged-var): data = var col's offsets; value = len */
    DD_KDT_ROWID = 101,  /* synthetic (staged-var): value = input row index */
};

/* K1 key kinds: what a compile-time key signature (dd_hash_device.h) says about one
 * non-nullable key column */
enum {
    DD_KK_NONE = 0,
    DD_KK_B1 = 1, /* u8 / bool */
    DD_KK_B2 = 2, /* i16 */
    DD_KK_B4 = 3, /* i32 */
    DD_KK_B8 = 4, /* i64 */
    DD_KK_F32 = 5,
    DD_KK_F64 = 6,
    DD_KK_DICT32 = 7,
};
/* signature code: first key's kind | second key's kind << 4 (0 = generic body) */
#define DD_K1_CODE(K0, K1) ((K0) | ((K1) << 4))

struct dd_kcol {
    int32_t dtype;
    int32_t elem;               /* fixed elem size (1/2/4/8/16); 0 for var (utf8) data */
    const void *data;           /* input values / utf8 bytes */
    const uint8_t *valid;       /* unpacked u8, or null */
    const int32_t *offsets;     /* utf8 input offsets[n+1] */
    const uint64_t *dict_hashes;/* dict32: per-value hash */
    void *out_data;             /* partition-major output values / bytes */
    uint8_t *out_valid;         /* partition-major output validity (if valid != null) */
    uint32_t *out_lengths;      /* utf8: partition-major per-row byte lengths */
};

struct dd_kargs {
    int64_t n_rows;
    int32_t n_cols;
    int32_t n_keys;
    int32_t n_var;
    uint32_t pid_total; /* pid = (h % pid_total) >> pid_shift; nparts = pid_total >> shift */
    int32_t pid_shift;  /* 0 for plain partitioning; >0 = contiguous coarse buckets */
    int32_t rhash;      /* staged spec path recomputes the row hash from preloaded
                           registers in K3 (no pid array: K1 skips its store, K3 its
                           load). Host gates: all-fixed no-validity batch, integer/bool
                           keys, wpb==16 (DD_RHASH=0 disables). */
    int32_t nt;         /* pre path: non-temporal flush stores (default on) */
    int32_t pid8;       /* pre path, P <= 256: pid array is u8 (saves 3 B/row of HBM
                           write in K1 + read in K3); dd_partitioner_pid_elem reports */
    int32_t hl;         /* hidden-load scatter (default on for its shape; DD_K3_HL=0
                           reverts): preload loads in inline asm + hand-counted
                           s_waitcnt so flush stores never drain mid-loop. gmax 4,
                           wpb 16, 4 fixed cols, no validity, elems in {4,8};
                           mutually exclusive with rhash. */
    int32_t key_idx[DD_KMAX_KEYS];
    int32_t var_idx[DD_KMAX_VAR];
    dd_kcol cols[DD_KMAX_COLS];
};

/* the plan of a final merge, passed by value so every field is wave-uniform */
struct dd_final_plan {
    int32_t n_aggs;
    int32_t ops[DD_F_MAX_AGGS];        /* DD_AGG_* read as merge ops */
    int32_t state_cols[DD_F_MAX_AGGS]; /* partial state column per aggregate */
    int32_t nn_cols[DD_F_MAX_AGGS];    /* i64 non-null-count column; unused for COUNT */
};

/* the projected columns of one side of a hash join, passed by value to k_join_gather */
struct dd_join_gather {
    int32_t n_cols;
    int32_t elem[DD_KMAX_COLS];               /* 1 / 2 / 4 / 8 / 16 */
    const void *src[DD_KMAX_COLS];
    const uint8_t *src_valid[DD_KMAX_COLS];   /* null: the column has no validity */
    void *dst[DD_KMAX_COLS];
    uint8_t *dst_valid[DD_KMAX_COLS];
};

/* the keys of a sort, passed by value to k_sort_encode. Word w of a row is the ordered
 * value word wpart[w] (0: the only or high word, 1: a dec128's low word) of key wkey[w];
 * the last word (n_words - 1) is the meta word: partition id << 32 | null rank of key j in
 * byte j */
struct dd_sort_keys {
    int32_t n_keys;
    int32_t n_words;
    int32_t dtype[DD_S_MAX_KEYS];
    int32_t flags[DD_S_MAX_KEYS]; /* DD_SORT_DESC | DD_SORT_NULLS_FIRST */
    int32_t wkey[DD_S_MAX_WORDS];
    int32_t wpart[DD_S_MAX_WORDS];
    const void *data[DD_S_MAX_KEYS];
    const uint8_t *valid[DD_S_MAX_KEYS]; /* null: the key has no validity */
};

/* the typed columns k_final_columns writes from a final merge's interleaved state */
struct dd_final_cols {
    int32_t n_keys;
    int32_t n_aggs;
    int32_t key_dtype[4];
    int32_t ops[DD_F_MAX_AGGS];
    void *key_data[4];
    uint8_t *key_valid[4];
    void *agg_data[DD_F_MAX_AGGS];
    uint8_t *agg_valid[DD_F_MAX_AGGS]; /* null for COUNT, which is never NULL */
    int64_t *nn_data[DD_F_MAX_AGGS];   /* null unless the nn columns were asked for */
};

/* dictionary GC (dd_dictgc.hip): one workgroup per row tile; a tile never straddles a
 * window boundary */
struct dd_gc_tile {
    int64_t row_lo, row_hi; /* partition-major output rows [row_lo, row_hi) */
    uint32_t window;
    uint32_t pad;
};
#define DD_GC_LDS_THREADS 1024 /* LDS tier: 16 waves share one staged bitmap */
#define DD_GC_GLB_THREADS 256
#define DD_GC_LDS_MAX_WORDS 16384u /* 64 KiB bitmap = dict_n <= 524288 */

/* view columns (dd_views.hip): a block of DD_VW_THREADS owns a tile of
 * DD_VW_TILE_ROWS rows and stages up to DD_VW_IMAGE_BYTES of its output in LDS */
#define DD_VW_THREADS 512
#define DD_VW_TILE_ROWS 512
#define DD_VW_IMAGE_BYTES 40960
/* emit tile: never straddles a partition (hence never a window) */
struct dd_vw_tile {
    int64_t row_lo, row_hi; /* partition-major output rows [row_lo, row_hi) */
    uint32_t part;          /* partition of the rows */
    uint32_t part_first;    /* first tile of that partition */
    uint32_t win_first;     /* first tile of the rows' window */
    uint32_t pad;
};

#include "dd_shuffle.h" /* dd_status for dd_set_error */

/* DD_PRE_XCD=1 block map of k_scatter_pre. Workgroups are dealt round-robin over
 * DD_NXCD dies with private L2s, so hardware blocks b, b+8, b+16, ... share one; this
 * hands those the contiguous logical run [start(x), start(x) + count(x)), x = b % 8,
 * count(x) = floor(nblocks/8) + (x < nblocks % 8). A bijection onto [0, nblocks) for
 * every nblocks (tests/test_xcd_map.py). */
#define DD_NXCD 8
__host__ __device__ inline int64_t dd_xcd_block_map(int64_t b, int64_t nblocks) {
    const int64_t q = nblocks / DD_NXCD, rem = nblocks % DD_NXCD;
    const int64_t x = b % DD_NXCD;
    return x * q + (x < rem ? x : rem) + b / DD_NXCD;
}

extern "C" {
hipError_t dd_launch_gc_mark(const dd_gc_tile *tiles, int64_t n_tiles, const int32_t *idx,
                             const uint8_t *valid, uint32_t dict_n, uint32_t nw, int lds,
                             uint32_t *bits, uint32_t *flag, hipStream_t s);
hipError_t dd_launch_gc_rank(const uint32_t *bits, uint32_t n_windows, uint32_t nw,
                             const int32_t *dict_offsets, uint32_t *prefix, uint32_t *nvals,
                             uint64_t *nbytes, hipStream_t s);
hipError_t dd_launch_gc_compact(const uint32_t *bits, const uint32_t *prefix,
                                uint32_t n_windows, uint32_t nw, const int32_t *dict_offsets,
                                const uint8_t *dict_bytes, const int64_t *val_off,
                                const int64_t *byte_off, int32_t *offs, uint8_t *out_bytes,
                                hipStream_t s);
hipError_t dd_launch_gc_remap(const dd_gc_tile *tiles, int64_t n_tiles, const int32_t *idx,
                              const uint8_t *valid, uint32_t dict_n, uint32_t nw, int lds,
                              const uint32_t *bits, const uint32_t *prefix, int32_t *out,
                              hipStream_t s);
hipError_t dd_launch_gc_rebase(const int32_t *in, int64_t n, const int64_t *seg_off,
                               const int32_t *bases, int32_t n_seg, int32_t skew,
                               int32_t *out, hipStream_t s);
hipError_t dd_launch_vw_len(const void *views, const uint8_t *valid, int64_t n_rows,
                            const int64_t *buf_lens, int32_t n_bufs, int32_t *lens,
                            uint64_t *tsum, uint32_t *flag, hipStream_t s);
hipError_t dd_launch_vw_scan(const uint64_t *in, int64_t n, int32_t nc, uint64_t *out,
                             uint64_t *meta, int32_t *off_end, hipStream_t s);
hipError_t dd_launch_vw_add(int32_t *offs, int64_t n_tiles, const uint64_t *tbase,
                            hipStream_t s);
hipError_t dd_launch_vw_copy(const void *views, int64_t n_rows, const uint8_t *const *bufs,
                             const int32_t *offs, uint8_t *out, int lds, hipStream_t s);
hipError_t dd_launch_ve_sums(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                             const uint8_t *valid, uint64_t *tsum, hipStream_t s);
hipError_t dd_launch_ve_build(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                              const uint8_t *valid, const uint8_t *bytes,
                              const uint64_t *part_boff, const uint64_t *S, void *views,
                              hipStream_t s);
hipError_t dd_launch_ve_copy(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                             const uint8_t *valid, const uint8_t *bytes,
                             const uint64_t *part_boff, const uint64_t *S, uint8_t *out,
                             int lds, hipStream_t s);
dd_status dd_set_error(dd_status s, const char *msg); /* thread-local dd_last_error */
hipError_t dd_launch_dict_hashes(const uint8_t *bytes, const int32_t *offsets, int64_t n,
                                 uint64_t *out, hipStream_t s);
hipError_t dd_launch_k5_maxlen(const int32_t *offsets, int64_t n, uint32_t *out_max,
                               hipStream_t s);
hipError_t dd_launch_k5_count(int64_t n, uint32_t nparts, const uint32_t *pid,
                              const int32_t *offsets, uint16_t *bcounts,
                              uint32_t *partials, int nranges, int64_t nseg5,
                              size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_k5_roff(const uint32_t *bcounts, const uint64_t *part_boffsets,
                             int64_t nrounds, int wpb, uint32_t nparts, uint32_t *roffB,
                             hipStream_t s);
hipError_t dd_launch_k5_scatter(int64_t n, uint32_t nparts, int nbits, const uint32_t *pid,
                                const int32_t *offsets, const uint8_t *in_bytes,
                                const uint32_t *gbaseB, const uint32_t *roffB,
                                int64_t nrounds, uint8_t *out_bytes, int wpb5,
                                size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_hash_count(const dd_kargs *a, int64_t nchunks, int64_t chunk_rows,
                                uint32_t nparts, int nbits, uint32_t *pid_out,
                                uint32_t *counts, uint32_t *bcounts, size_t lds_bytes,
                                hipStream_t s);
hipError_t dd_launch_scan(uint32_t *counts, int64_t nchunks, uint32_t nparts, int nranges,
                          uint32_t *partials, uint64_t *part_offsets, int fold_global,
                          hipStream_t s);
hipError_t dd_launch_scan_deep(uint16_t *counts16, int64_t nchunks, uint32_t nparts,
                               int nr1, int nr2, uint32_t *partials, uint32_t *partials2,
                               uint64_t *part_offsets, uint32_t *gbase, hipStream_t s);
/* k1_spec: the K1 key-signature code chosen at create time (dd_hash_device.h; 0 = generic) */
hipError_t dd_launch_hash_count_seg(const dd_kargs *a, int k1_spec, int64_t nseg,
                                    int64_t seg_rows, uint32_t nparts, int nbits,
                                    uint32_t *pid_out, uint16_t *counts, uint32_t *partials,
                                    int nranges, size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_round_layout(const uint32_t *counts, const uint64_t *part_offsets,
                                  int64_t nrounds, int wpb, uint32_t nparts, uint32_t sP2,
                                  uint16_t *imgb, hipStream_t s);
hipError_t dd_launch_scatter_pre(const dd_kargs *a, int64_t nblocks, int64_t nrounds,
                                 int rpb, uint32_t nparts, int nbits,
                                 const uint32_t *pid_in, const uint32_t *gbase,
                                 const uint16_t *imgb, uint32_t sP2, const uint16_t *segoff,
                                 const uint32_t *rbase, int layout, int xcd, int gmax,
                                 int wpb, size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_scatter_pre_wide(const dd_kargs *a, int64_t nblocks, int64_t nrounds,
                                      int rpb, uint32_t nparts, int nbits,
                                      const uint32_t *pid_in, const uint16_t *rofftab,
                                      uint32_t sP2, const uint16_t *segoff,
                                      const uint32_t *rbase, int xcd, size_t lds_bytes,
                                      hipStream_t s);
hipError_t dd_launch_hash_count_round(const dd_kargs *a, int k1_spec, int64_t nrounds,
                                      int64_t seg_rows, int wpb, uint32_t nparts,
                                      uint32_t sP2, uint32_t *pid_out, uint16_t *segoff,
                                      uint32_t *roundcnt, uint16_t *rofftab,
                                      hipStream_t s);
hipError_t dd_launch_scan_round(const uint32_t *roundcnt, int64_t nrounds, uint32_t nparts,
                                uint32_t sP2, int nr1, int nr2, uint32_t *partials,
                                uint32_t *partials2, uint32_t *totals,
                                uint64_t *part_offsets, uint32_t *rbase, hipStream_t s);
hipError_t dd_launch_hash_count_tile(const dd_kargs *a, int k1_spec, int64_t nblocks,
                                     int64_t tile_rows, uint32_t nparts, int nbits,
                                     uint32_t *pid_out, uint32_t *counts, size_t lds_bytes,
                                     hipStream_t s);
hipError_t dd_launch_scatter_staged(const dd_kargs *a, int64_t nblocks, int64_t tile_rows,
                                    uint32_t nparts, int nbits, const uint32_t *pid_in,
                                    const uint32_t *tile_off, const uint64_t *part_offsets,
                                    int gmax, int wpb, size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_scatter(const dd_kargs *a, int64_t nchunks, int64_t chunk_rows,
                             uint32_t nparts, int nbits, const uint32_t *pid_in,
                             const uint32_t *chunk_off, const uint64_t *part_offsets,
                             const uint32_t *chunk_boff, const uint64_t *part_boffsets,
                             size_t lds_bytes, hipStream_t s);
hipError_t dd_launch_off64_to_off32(const uint64_t *off64, int64_t lo, int64_t n,
                                    int32_t *out32, hipStream_t s);
hipError_t dd_launch_var_bytes(const uint32_t *lens, const uint32_t *src_row,
                               const int32_t *in_offsets, const uint8_t *in_bytes,
                               int64_t n, uint64_t *partials,
                               uint64_t *out_off, uint8_t *out_bytes,
                               const uint64_t *part_offsets, uint32_t nparts,
                               uint64_t *part_boffsets, uint32_t *k4w_meta,
                               uint32_t *k4w_order, int skip_copy, hipStream_t s);
hipError_t dd_launch_partial_reduce(const dd_kargs *a, int64_t nblocks, int64_t chunk_rows,
                                    int n_aggs, const int32_t *agg_cols,
                                    const int32_t *agg_ops, uint64_t *out_keys,
                                    uint32_t *out_keynull, double *out_aggs,
                                    uint64_t *out_nn, uint64_t *out_n, hipStream_t s);
/* agg_cols / agg_ops: DD_RW_MAX_AGGS device ints each; lds_bytes as the plan geometry
 * reports it (sets the kernel's dynamic-LDS attribute when past 64 KiB) */
hipError_t dd_launch_partial_reduce_wide(const dd_kargs *a, int waveagg, int64_t nblocks,
                                         int64_t chunk_rows, int n_aggs, int table_slots,
                                         int probe_limit, size_t lds_bytes,
                                         const int32_t *agg_cols, const int32_t *agg_ops,
                                         uint64_t *out_keys, uint32_t *out_keynull,
                                         uint64_t *out_aggs, uint64_t *out_hi,
                                         uint64_t *out_nn, uint64_t *out_n, hipStream_t s);
/* final merge (dd_final.hip). table / slot_gid: n_slots u32 entries, n_slots a multiple
 * of 4; part_base / part_log2: region base and log2(region slots) per partition */
hipError_t dd_launch_final_claim(const dd_kargs *a, const int64_t *seg_offsets,
                                 const int32_t *seg_part, int32_t n_segs,
                                 const uint32_t *part_base, const uint32_t *part_log2,
                                 uint32_t *table, uint32_t *row_slot, uint32_t *err,
                                 hipStream_t s);
/* block_sums: n_slots / DD_F_SCAN_TILE (rounded up) + 1 entries; group_offsets: device
 * int64[n_parts + 1] */
hipError_t dd_launch_final_scan(const uint32_t *table, uint64_t n_slots,
                                uint32_t *block_sums, uint32_t *slot_gid,
                                const uint32_t *part_base, int32_t n_parts,
                                int64_t *group_offsets, hipStream_t s);
hipError_t dd_launch_final_merge(const dd_kargs *a, const dd_final_plan *plan,
                                 const uint32_t *table, const uint32_t *row_slot,
                                 const uint32_t *slot_gid, int64_t n_groups,
                                 uint64_t *out_keys, uint32_t *out_keynull,
                                 uint64_t *out_aggs, uint64_t *out_hi, uint64_t *out_nn,
                                 hipStream_t s);
/* typed device columns of a finished final merge (k_final_columns, dd_final.hip) */
hipError_t dd_launch_final_columns(const dd_final_cols *c, int64_t n_groups,
                                   const uint64_t *keys, const uint32_t *keynull,
                                   const uint64_t *aggs, const uint64_t *hi,
                                   const uint64_t *nn, hipStream_t s);
/* sort (dd_sort.hip). words: u64[n_words][n]; census: u32[n_words][8][256], zeroed */
hipError_t dd_launch_sort_encode(const dd_sort_keys *k, int64_t n, const int64_t *seg_offsets,
                                 const int32_t *seg_part, int32_t n_segs, uint64_t *words,
                                 uint32_t *perm, uint32_t *census, hipStream_t s);
/* one stable pass on the digit (word >> shift) & 255. hist: u32[256 * tiles], tiles = n /
 * DD_S_TILE rounded up; sums: u32[256 * tiles / DD_S_SCAN_TILE rounded up] */
hipError_t dd_launch_sort_pass(const uint64_t *win, const uint32_t *pin, int64_t n, int shift,
                               uint32_t *hist, uint32_t *sums, uint64_t *wout, uint32_t *pout,
                               hipStream_t s);
hipError_t dd_launch_sort_gather_word(const uint64_t *src, const uint32_t *perm, int64_t n,
                                      uint64_t *out, hipStream_t s);
/* in_off / out_off: device int64[n_parts + 1], sorted rows and kept rows before partition p */
hipError_t dd_launch_sort_seg_out(const uint32_t *sorted, const int64_t *in_off,
                                  const int64_t *out_off, int32_t n_parts, int64_t n_out,
                                  uint32_t *perm_out, hipStream_t s);
/* hash join (dd_join.hip). table: the build side's regions as in the final merge; next:
 * u32[build rows] preset to DD_F_EMPTY; the layout passed to build is the build side's, to
 * count / emit_probe the probe side's */
hipError_t dd_launch_join_build(const dd_kargs *b, const int64_t *seg_offsets,
                                const int32_t *seg_part, int32_t n_segs,
                                const uint32_t *part_base, const uint32_t *part_log2,
                                uint32_t *table, uint32_t *next, uint32_t *err, hipStream_t s);
hipError_t dd_launch_join_count(const dd_kargs *b, const dd_kargs *p,
                                const int64_t *seg_offsets, const int32_t *seg_part,
                                int32_t n_segs, const uint32_t *part_base,
                                const uint32_t *part_log2, const uint32_t *table,
                                const uint32_t *next, int32_t join_type, uint32_t *cnt,
                                uint8_t *matched, hipStream_t s);
hipError_t dd_launch_join_left_cnt(const uint8_t *matched, int64_t n, int anti, uint32_t *cnt,
                                   hipStream_t s);
/* cnt: n rounded up to a multiple of 4 entries, the pad zero; scanned in place. sums:
 * tiles + 1 u64; seg_out: device int64[n_segs + 2], the last entry the exact total */
hipError_t dd_launch_join_scan(uint32_t *cnt, int64_t n, uint64_t *sums,
                               const int64_t *seg_offsets, int32_t n_segs, int64_t *seg_out,
                               hipStream_t s);
hipError_t dd_launch_join_emit_probe(const dd_kargs *b, const dd_kargs *p,
                                     const int64_t *seg_offsets, const int32_t *seg_part,
                                     int32_t n_segs, const uint32_t *part_base,
                                     const uint32_t *part_log2, const uint32_t *table,
                                     const uint32_t *next, int32_t join_type,
                                     const uint32_t *off, uint32_t n_out, uint32_t *build_idx,
                                     uint32_t *probe_idx, hipStream_t s);
hipError_t dd_launch_join_emit_build(const uint8_t *matched, int64_t n, int anti,
                                     const uint32_t *off, uint32_t n_out, uint32_t *build_idx,
                                     hipStream_t s);
hipError_t dd_launch_join_gather(const dd_join_gather *g, const uint32_t *idx, int64_t n_out,
                                 hipStream_t s);
/* outer joins. cnt: u32[n_probe + n_build] (right: [n_probe]), padded to 4
 * as for the scan; head: u32[probe rows]; matched: u8[build rows] zeroed, null for right.
 * emit: n_tail = build rows for left / full, 0 for right; off is the scanned cnt */
hipError_t dd_launch_join_count_outer(const dd_kargs *b, const dd_kargs *p,
                                      const int64_t *seg_offsets, const int32_t *seg_part,
                                      int32_t n_segs, const uint32_t *part_base,
                                      const uint32_t *part_log2, const uint32_t *table,
                                      const uint32_t *next, int keep_probe, uint32_t *head,
                                      uint32_t *cnt, uint8_t *matched, hipStream_t s);
hipError_t dd_launch_join_build_cnt_outer(const uint8_t *matched, int64_t n_build,
                                          int64_t n_probe, uint32_t *cnt, hipStream_t s);
hipError_t dd_launch_join_emit_outer(const uint32_t *head, const uint32_t *next,
                                     const uint8_t *matched, const uint32_t *off,
                                     int64_t n_probe, int64_t n_tail, int keep_probe,
                                     uint32_t n_out, uint32_t *build_idx, uint32_t *probe_idx,
                                     hipStream_t s);
hipError_t dd_launch_join_gather_outer(const dd_join_gather *g, const uint32_t *idx,
                                       int64_t n_out, hipStream_t s);
}

#endif
