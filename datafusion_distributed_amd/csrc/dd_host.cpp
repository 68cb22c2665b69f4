/* dd_host.cpp — host side of libdd_shuffle.so: the C ABI (include/dd_shuffle.h), the task
 * cache mirroring the reference's worker execute path, and the RCCL/xGMI exchange replacing
 * the Arrow-Flight data plane. See header citations in include/dd_shuffle.h and DESIGN.md.
 *
 * Product path only: no CPU fallback anywhere — a missing/failed HIP device is a hard error
 * (DD_ERR_NO_DEVICE), by design.
 */

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dd_shuffle.h"
#include "dd_internal.h"

/* ---------------- error plumbing ---------------- */

static thread_local std::string g_last_error;

static dd_status set_err(dd_status s, const std::string &msg) {
    g_last_error = msg;
    return s;
}

extern "C" const char *dd_last_error(void) { return g_last_error.c_str(); }
/* shared with dd_proto.cpp (declared in dd_internal.h) */
extern "C" dd_status dd_set_error(dd_status s, const char *msg) {
    g_last_error = msg;
    return s;
}
extern "C" const char *dd_version(void) { return "dd_shuffle 0.1 (gfx950)"; }

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return set_err(DD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

#define NCCL_TRY(expr)                                                                       \
    do {                                                                                     \
        ncclResult_t _r = (expr);                                                            \
        if (_r != ncclSuccess)                                                               \
            return set_err(DD_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
    } while (0)

/* Dedicated stream for pooled (stream-ordered) allocations: hipMallocAsync/hipFreeAsync
 * on the NULL stream never reuse the pool on ROCm 7.2 (measured: 50x 16 MB alloc/free
 * cycles leak ~190 MB on NULL stream, 0 on a real stream), so all pool traffic goes
 * through this stream and users of the buffers sync it once after allocating. */
static hipStream_t dd_pool_stream(void) {
    static hipStream_t s = nullptr;
    static std::once_flag once;
    std::call_once(once, [] { (void)hipStreamCreate(&s); });
    return s;
}

extern "C" int dd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ---------------- device helpers ---------------- */

extern "C" dd_status dd_dev_alloc(int64_t bytes, void **out) {
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");
    HIP_TRY(hipMalloc(out, bytes > 0 ? (size_t)bytes : 1));
    return DD_OK;
}
extern "C" dd_status dd_dev_free(void *p) {
    HIP_TRY(hipFree(p));
    return DD_OK;
}
extern "C" dd_status dd_memcpy_h2d(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return DD_OK;
}
extern "C" dd_status dd_memcpy_h2d_async(void *dst, const void *src, int64_t bytes,
                                          void *stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice,
                           (hipStream_t)stream));
    return DD_OK;
}
extern "C" dd_status dd_memcpy_d2h(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return DD_OK;
}
extern "C" dd_status dd_memcpy_d2d(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice));
    return DD_OK;
}
extern "C" dd_status dd_device_sync(void) {
    HIP_TRY(hipDeviceSynchronize());
    return DD_OK;
}

/* ---------------- partitioner ---------------- */

static int fixed_elem_size(int dtype) {
    switch (dtype) {
    case DD_DT_U8:
    case DD_DT_BOOL:
        return 1;
    case DD_DT_I16:
        return 2;
    case DD_DT_I32:
    case DD_DT_F32:
    case DD_DT_DICT32:
        return 4;
    case DD_DT_I64:
    case DD_DT_F64:
        return 8;
    case DD_DT_DEC128:
        return 16;
    default:
        return 0; /* utf8 */
    }
}

/* Wide rounds (R = 8192) halve the block count of a batch, so they are
 * the default only from DD_WIDE_MIN_ROWS rows up. All three eligible tiers (headline,
 * dictkey, multikey) measured a step win beyond noise in both repeats at bench size, and
 * the headline wins from 6 M rows up (profiles/r06_wide_rounds.txt); the threshold is held
 * at 8 M so that plans of smaller batches stay what they were. */
#define DD_WIDE_MIN_ROWS 8000000LL

struct dd_partitioner {
    dd_batch_desc batch;
    dd_kargs ka;
    uint32_t nparts = 0;
    int nbits = 0;
    int64_t nchunks = 0, chunk_rows = 0;
    size_t lds_k1 = 0, lds_k3 = 0;
    bool staged = false; /* v2 path: block-tile + LDS-staged scatter (fixed-width only) */
    int gmax = 0;        /* v2 groups per wave per round */
    int wpb = 4;         /* v2 waves per block; rows per round R = gmax * wpb * 64 */
    bool pre = false;    /* K3-P: precomputed round layout (k_scatter_pre) */
    int64_t nrounds = 0, nseg_pad = 0; /* pre: globally-aligned rounds / padded segments */
    int rpb = 1;                       /* pre: rounds per block */
    int pre_nranges = 0;               /* pre: scan ranges (segment-granular counts) */
    uint32_t sP2 = 0;                  /* pre: imgb row stride (u16, even) */
    int pre_layout = 0; /* 0 not pre, 1 seg (k_hash_count_seg), 2 round (k_hash_count_round) */
    int pre_xcd = 0;    /* DD_PRE_XCD=1: k_scatter_pre walks rounds in XCD-contiguous order */
    bool pre_wide = false; /* wide rounds: k_scatter_pre_wide (gmax 8, R = 8192) */
    int round_nr1 = 0, round_nr2 = 0; /* round layout: scan ranges (nr2 == 0: one level) */
    int k1_spec = 0; /* K1 key-signature code (DD_K1_CODE; 0 = generic dd_row_hash body) */

    /* device buffers (owned) */
    uint32_t *pid = nullptr;
    uint32_t *counts = nullptr;          /* [nchunks][P] */
    uint32_t *partials = nullptr;        /* [RANGES][P] */
    uint64_t *part_offsets = nullptr;    /* [P+1] */
    uint32_t *bcounts = nullptr;         /* v1: [nvar][nchunks][P] */
    uint32_t *bpartials = nullptr;       /* v1: [nvar][RANGES][P] */
    uint64_t *part_boffsets = nullptr;   /* [nvar][P+1] */
    uint16_t *imgb = nullptr;            /* pre: [nrounds][sP2] round image bases (roff) */
    uint32_t *partials2 = nullptr;       /* pre: second-level scan partials [64][P] */
    uint16_t *counts16 = nullptr;        /* pre seg: [nseg][P] u16 segment counts;
                                            pre round: segoff [nseg][sP2] u16 */
    uint32_t *gbase = nullptr;           /* pre seg: [nseg][P] u32 global slot bases */
    uint32_t *roundcnt = nullptr;        /* pre round: [nrounds][sP2] rows per round */
    uint32_t *rbase = nullptr;           /* pre round: [nrounds][sP2] global slot bases */
    uint32_t *totals = nullptr;          /* pre round: [sP2] rows per partition */
    uint32_t *src_row = nullptr;         /* staged-var: permutation out[slot] = input row */
    uint32_t *k4w_meta = nullptr;        /* staged-var: window hist/base (k4_copy_ord) */
    uint32_t *k4w_order = nullptr;       /* staged-var: window-bucketed group order */
    int k5 = 0;                          /* LDS-staged var-byte scatter (small strings) */
    int k5_wpb = 16;                     /* waves/block (8 = 2 blocks/CU overlap) */
    int k5_nranges = 2048;               /* fused-partials ranges (scales with nseg5) */
    int64_t k5_nrounds = 0, k5_nseg = 0;
    uint32_t k5_maxlen = 0;
    size_t lds_k5 = 0, lds_k5c = 0;
    uint16_t *k5_bcounts = nullptr;      /* [nseg5][P] u16 byte counts */
    uint32_t *k5_gbase = nullptr;        /* [nseg5][P] u32 global byte bases */
    uint32_t *k5_partials = nullptr;     /* [2048][P] */
    uint32_t *k5_partials2 = nullptr;    /* [64][P] */
    uint32_t *k5_roffB = nullptr;        /* [nrounds5][P+1] */
    uint64_t *out_off[DD_KMAX_VAR] = {}; /* staged-var: Arrow byte offsets [n+1] per var */
    uint64_t *k4_partials = nullptr;     /* staged-var scan scratch */
    uint64_t *dict_hashes[DD_KMAX_COLS] = {};
    void *out_data[DD_KMAX_COLS] = {};
    uint8_t *out_valid[DD_KMAX_COLS] = {};
    uint32_t *out_lengths[DD_KMAX_COLS] = {};

    hipEvent_t ev[5] = {}; /* 0 K1start 1 K1end 2 scans-end 3 K3end 4 K3start */
    std::atomic<bool> has_run{false}; /* release/acquire pairs with dd_execute_task */

    ~dd_partitioner() {
        (void)hipFree(pid);
        (void)hipFree(imgb);
        (void)hipFree(partials2);
        (void)hipFree(counts);
        (void)hipFree(partials);
        (void)hipFree(part_offsets);
        (void)hipFree(bcounts);
        (void)hipFree(bpartials);
        (void)hipFree(part_boffsets);
        (void)hipFree(src_row);
        (void)hipFree(k4w_meta);
        (void)hipFree(k4w_order);
        (void)hipFree(counts16);
        (void)hipFree(gbase);
        (void)hipFree(roundcnt);
        (void)hipFree(rbase);
        (void)hipFree(totals);
        (void)hipFree(k5_bcounts);
        (void)hipFree(k5_gbase);
        (void)hipFree(k5_partials);
        (void)hipFree(k5_partials2);
        (void)hipFree(k5_roffB);
        for (auto &o : out_off) hipFree(o);
        (void)hipFree(k4_partials);
        for (int i = 0; i < DD_KMAX_COLS; i++) {
            (void)hipFree(dict_hashes[i]);
            (void)hipFree(out_data[i]);
            (void)hipFree(out_valid[i]);
            (void)hipFree(out_lengths[i]);
        }
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" dd_status dd_partitioner_create(const dd_batch_desc *batch, const int32_t *key_cols,
                                           int32_t n_keys, uint32_t n_partitions,
                                           dd_partitioner **out) {
    if (!batch || !key_cols || !out) return set_err(DD_ERR_INVALID, "null argument");
    if (dd_device_count() == 0)
        return set_err(DD_ERR_NO_DEVICE,
                       "no HIP device: the product path has no CPU fallback (DESIGN.md §2)");
    if (batch->n_cols < 1 || batch->n_cols > DD_MAX_COLS)
        return set_err(DD_ERR_INVALID, "n_cols out of range");
    if (n_keys < 1 || n_keys > DD_MAX_KEYS) return set_err(DD_ERR_INVALID, "n_keys out of range");
    if (n_partitions < 1 || n_partitions > DD_MAX_PARTITIONS)
        return set_err(DD_ERR_UNSUPPORTED, "n_partitions outside round-1 cap");
    if (batch->n_rows < 0 || batch->n_rows >= (int64_t)UINT32_MAX)
        return set_err(DD_ERR_UNSUPPORTED, "n_rows >= 2^32: chunk the batch");

    auto p = new dd_partitioner();
    p->batch = *batch;
    p->nparts = n_partitions;
    p->nbits = 0;
    while ((1u << p->nbits) < n_partitions) p->nbits++;

    const int64_t n = batch->n_rows;
    dd_kargs &ka = p->ka;
    memset(&ka, 0, sizeof(ka));
    ka.n_rows = n;
    ka.n_cols = batch->n_cols;
    ka.n_keys = n_keys;
    ka.pid_total = n_partitions;
    ka.pid_shift = 0;

    auto fail = [&](dd_status s, const char *m) {
        delete p;
        return set_err(s, m);
    };

    for (int k = 0; k < n_keys; k++) {
        if (key_cols[k] < 0 || key_cols[k] >= batch->n_cols)
            return fail(DD_ERR_INVALID, "key column index out of range");
        ka.key_idx[k] = key_cols[k];
    }

    for (int c = 0; c < batch->n_cols; c++) {
        const dd_col_desc &cd = batch->cols[c];
        dd_kcol &kc = ka.cols[c];
        kc.dtype = cd.dtype;
        kc.elem = fixed_elem_size(cd.dtype);
        kc.data = cd.data;
        kc.valid = cd.validity;
        kc.offsets = cd.offsets;
        /* the kernels move a dec128 value with one 16-byte access */
        if (cd.dtype == DD_DT_DEC128 && ((uintptr_t)cd.data & 15) != 0)
            return fail(DD_ERR_INVALID, "dec128 column data must be 16-byte aligned");
        if (cd.dtype == DD_DT_UTF8) {
            if (ka.n_var >= DD_KMAX_VAR) return fail(DD_ERR_UNSUPPORTED, "too many var columns");
            /* Arrow utf8 offsets are int32: a column past INT32_MAX bytes has already
             * overflowed its own offsets — reject rather than read garbage (chunked.py
             * splits larger inputs before they get here) */
            if (cd.data_len < 0 || cd.data_len > (int64_t)INT32_MAX)
                return fail(DD_ERR_UNSUPPORTED, "utf8 data > 2 GB (int32 Arrow offsets): chunk the batch");
            ka.var_idx[ka.n_var++] = c;
        }
    }

    const int64_t P = n_partitions;
    const int nvar = ka.n_var;

    /* v2 (staged) eligibility: <= DD_STAGE_MAXC columns including the synthetic staged-var
     * entries (per var col a VARLEN length column + one ROWID permutation column; the var
     * BYTES go through K4), staging fits LDS */
    /* staged-var (synthetic VARLEN/ROWID cols + wave-cooperative K4 gather-copy) measured
     * faster than the v1 direct path for string-heavy batches (457 vs 334 GB/s on the
     * ClickBench shape) — default on; DD_V2_VAR=0 forces the v1 path */
    const bool allow_staged_var =
        !(getenv("DD_V2_VAR") && atoi(getenv("DD_V2_VAR")) == 0);
    const int aug_cols = batch->n_cols + nvar + (nvar > 0 ? 1 : 0);
    if (aug_cols <= DD_STAGE_MAXC && (nvar == 0 || allow_staged_var)) {
        size_t row_stage = 4; /* dstg */
        int nvalid = 0;
        bool has16 = false; /* a dec128 column: 16-byte image slots, W16 kernel form */
        for (int c = 0; c < batch->n_cols; c++) {
            row_stage += fixed_elem_size(batch->cols[c].dtype);
            if (fixed_elem_size(batch->cols[c].dtype) == 16) has16 = true;
            if (batch->cols[c].validity) nvalid++;
        }
        row_stage += nvalid;
        row_stage += 4 * nvar + (nvar > 0 ? 4 : 0); /* VARLEN cols + ROWID col */
        /* auto: 8 waves x 4 groups (R=2048, 2 blocks/CU at the bench shape) measured best;
         * DD_V2_GMAX / DD_V2_WPB override for experiments */
        /* wpb cascade: 16-wave blocks measured best at the bench shape (wpb=16 g=4:
         * K3 1.381 ms vs 1.408 at 8/4) but their partition arrays outgrow LDS at large P
         * — fall back to 8 then 4 waves. Aim for R >= 32P (16/4 measured best at P=128),
         * floor g=2. DD_V2_WPB / DD_V2_GMAX override for experiments. */
        int wpb_cands[3] = {16, 8, 4};
        if (const char *e = getenv("DD_V2_WPB")) {
            int v = atoi(e);
            if (v == 4 || v == 8 || v == 16) {
                wpb_cands[0] = v;
                wpb_cands[1] = wpb_cands[2] = 0;
            }
        }
        for (int wi = 0; wi < 3 && !p->staged; wi++) {
            const int wpb = wpb_cands[wi];
            if (!wpb) continue;
            /* k_scatter_staged is instantiated for (gmax, wpb) in {2,4,8}x{4,8} and
             * {2,4}x{16} */
            int gcap = (wpb == 16) ? 4 : 8;
            /* W16 forms past 4 columns exist up to gmax 2 / 4 / 8 at wpb 16 / 8 / 4 (their
             * second value register per row group; DD_CASE16 in dd_launch_scatter_staged) */
            if (has16 && aug_cols > 4) gcap = (wpb == 16) ? 2 : (wpb == 8) ? 4 : 8;
            int gtop = 2;
            while (gtop < gcap && (size_t)gtop * wpb * 64 < 32 * (size_t)P) gtop *= 2;
            if (const char *e = getenv("DD_V2_GMAX")) {
                int v = atoi(e);
                if (v == 2 || v == 4 || v == 8) gtop = (v <= gcap) ? v : gcap;
            }
            for (int g = gtop; g >= 2; g /= 2) {
                const size_t part_lds =
                    (size_t)P * (8 + 4 * wpb + 4 + 4) + (size_t)wpb * 64 * 4;
                size_t lds = part_lds + (size_t)g * wpb * 64 * row_stage;
                if (lds <= 163840) {
                    p->staged = true;
                    p->gmax = g;
                    p->wpb = wpb;
                    p->lds_k3 = lds;
                    break;
                }
            }
        }
    }
    if (p->staged) {
        p->lds_k1 = (size_t)WAVES_PER_BLOCK_H * P * 4;
        int64_t nblocks = (n + 16383) / 16384;
        if (nblocks < 8) nblocks = 8;
        if (nblocks > 2048) nblocks = 2048;
        if (const char *e = getenv("DD_V2_BLOCKS")) { /* tile-count experiment knob */
            int64_t v = atoll(e);
            if (v >= 8 && v <= 8192) nblocks = v;
        }
        p->nchunks = nblocks;
        p->chunk_rows = (n + nblocks - 1) / nblocks;
        if (p->chunk_rows < 1) p->chunk_rows = 1;
    } else {
        p->lds_k1 = (size_t)WAVES_PER_BLOCK_H * P * 4 * (1 + nvar);
        p->lds_k3 =
            (size_t)WAVES_PER_BLOCK_H * P * 8 * (1 + nvar) + WAVES_PER_BLOCK_H * 64 * 4;
        if (p->lds_k1 > 163840 || p->lds_k3 > 163840)
            return fail(DD_ERR_UNSUPPORTED, "partition count x var columns exceeds LDS budget");
        int64_t nchunks = (n + 4095) / 4096;
        if (nchunks < 4) nchunks = 4;
        if (nchunks > 8192) nchunks = 8192;
        nchunks = (nchunks + 3) & ~3LL;
        p->nchunks = nchunks;
        p->chunk_rows = (n + nchunks - 1) / nchunks;
        if (p->chunk_rows < 1) p->chunk_rows = 1;
    }
    /* K3-P (precomputed round layout, round 2 — DESIGN.md §13): replaces the in-kernel
     * cross-wave scan / round_off scan / serial dstbase chain of the staged scatter with
     * segment-granular precomputed bases (k_hash_count_seg + global-base scan fold +
     * k_round_layout + k_scatter_pre). Default ON for its instantiated shapes;
     * DD_K3_PRE=0 reverts to the HL/spec path for A/B. Mutually exclusive with rhash
     * (pre reads the pid array). Shape whitelist mirrors dd_launch_scatter_pre. */
    if (p->staged && p->wpb == 16 && nvar == 0 &&
        !(getenv("DD_K3_PRE") && atoi(getenv("DD_K3_PRE")) == 0) &&
        !(getenv("DD_RHASH") && atoi(getenv("DD_RHASH")) == 1)) {
        bool fixed_ok = true;
        int rowb = 0;
        for (int c = 0; c < batch->n_cols && fixed_ok; c++) {
            const int e = fixed_elem_size(batch->cols[c].dtype);
            if (batch->cols[c].validity || e == 0) fixed_ok = false;
            rowb += e;
        }
        auto pre_is = [&](std::initializer_list<int> want) {
            if ((int)want.size() != batch->n_cols) return false;
            int c = 0;
            for (int w : want)
                if (fixed_elem_size(batch->cols[c++].dtype) != w) return false;
            return true;
        };
        int pgmax = 0;
        if (fixed_ok) {
            const uint32_t Pn = n_partitions;
            bool all48 = batch->n_cols == 4;
            for (int c = 0; c < batch->n_cols && all48; c++) {
                const int e = fixed_elem_size(batch->cols[c].dtype);
                if (e != 4 && e != 8) all48 = false;
            }
            if (Pn <= 128 && (all48 || pre_is({8, 8, 8, 4, 4})))
                pgmax = 4;
            else if (Pn <= 128 && pre_is({1, 1, 8, 8, 8, 8, 4}))
                pgmax = 2;
            else if (Pn <= 256 && pre_is({8, 8, 8, 4}))
                pgmax = 4;
            else if (Pn <= 512 && (pre_is({8, 8, 8, 4}) || pre_is({8, 8, 8, 4, 4})))
                pgmax = 2;
        }
        if (pgmax > 0) {
            if (const char *e = getenv("DD_PRE_GMAX")) { /* experiment knob */
                int v = atoi(e);
                if (v == 2 || v == 4) pgmax = v;
            }
            int wpb = 16;
            if (const char *e = getenv("DD_PRE_WPB")) { /* experiment knob (8: 2 blk/CU) */
                int v = atoi(e);
                if (v == 8 || v == 16) wpb = v;
            }
            const uint32_t sP2 = (n_partitions + 1) & ~1u;
            /* wide rounds (k_scatter_pre_wide): gmax 8 x wpb 16,
             * R = 8192, round layout only, on the whitelisted shapes at P <= 128 (must
             * mirror dd_launch_scatter_pre_wide). DD_PRE_WIDE=1 forces it on an eligible
             * shape, 0 forbids it; unset, it is taken from DD_WIDE_MIN_ROWS rows up
             * (DD_PRE_WIDE_MIN_ROWS overrides the threshold, for tests).
             * DD_PRE_LAYOUT=seg always gets the narrow form. */
            bool wide = false;
            /* n < 2^29: the kernel addresses rows by 32-bit byte offsets (8 B elements) */
            const bool wide_shape =
                fixed_ok && n_partitions <= 128 && n < (1LL << 29) &&
                (pre_is({8, 8, 8, 4}) || pre_is({4, 8, 8, 4}) || pre_is({8, 8, 8, 4, 4}));
            const char *lay_env = getenv("DD_PRE_LAYOUT");
            if (wide_shape && !(lay_env && strcmp(lay_env, "seg") == 0)) {
                int64_t min_rows = DD_WIDE_MIN_ROWS;
                if (const char *e = getenv("DD_PRE_WIDE_MIN_ROWS")) {
                    const int64_t v = atoll(e);
                    if (v >= 1) min_rows = v;
                }
                wide = n >= min_rows;
                if (const char *e = getenv("DD_PRE_WIDE")) wide = atoi(e) == 1;
            }
            size_t lds_wide = 0;
            if (wide) {
                const size_t Rw = 8 * 16 * 64;
                /* stage R x 16 B | gdelta u32[2][P] | pslot u8[R] | per-wave rf u16[sP2]
                 * and ms u16[P] */
                lds_wide = Rw * 16 + 8 * (size_t)n_partitions + Rw +
                           16 * (2 * (size_t)sP2 + 2 * (size_t)n_partitions);
                if (lds_wide > 163840) wide = false;
            }
            if (wide) {
                pgmax = 8;
                wpb = 16;
            }
            const int64_t R = (int64_t)pgmax * wpb * 64;
            const size_t lds = wide ? lds_wide
                                    : (size_t)R * rowb + 4 * (size_t)R +
                                          (size_t)wpb * (4 * (size_t)n_partitions +
                                                         2 * (size_t)sP2 +
                                                         2 * (size_t)n_partitions);
            if (lds <= 163840) {
                p->pre = true;
                p->pre_wide = wide;
                p->gmax = pgmax;
                p->wpb = wpb;
                p->lds_k3 = lds;
                p->sP2 = sP2;
                p->nrounds = (n + R - 1) / R;
                if (p->nrounds < 1) p->nrounds = 1;
                const int64_t nseg = p->nrounds * wpb;
                p->nseg_pad = (nseg + 3) & ~3LL;
                p->rpb = 2; /* sweep (tools/sweep_pre.py): rpb2 K3 0.896 ms vs rpb1
                               0.953 / rpb4 0.924 / ceil(nrounds/2048)=8 1.079 on the
                               bench shape — small rpb beats in-block pipelining depth */
                if (wide) p->rpb = 1; /* wide rounds, headline with the XCD order: rpb1 K3
                                         0.72-0.77 ms vs rpb2 0.90-0.97 / rpb4 1.02; best
                                         on dictkey and multikey too */
                /* u8 pid array when P fits: 3 B/row less HBM write (K1) + read (K3);
                   DD_PID8=0 reverts */
                if (n_partitions <= 256 &&
                    !(getenv("DD_PID8") && atoi(getenv("DD_PID8")) == 0))
                    ka.pid8 = 1;
                if (const char *e = getenv("DD_PRE_RPB")) { /* experiment knob */
                    int v = atoi(e);
                    if (v >= 1 && v <= 256) p->rpb = v;
                }
                /* scale the fused-partials range count with the segment count so the
                 * per-(range,partition) atomic contention stays ~constant (~114 adds):
                 * fixed 2048 measured K1 +28%/row at 600 M rows (SF100) */
                {
                    const int64_t nseg_tmp = ((n + R - 1) / R < 1 ? 1 : (n + R - 1) / R) * wpb;
                    int64_t nr = nseg_tmp / 114;
                    if (nr < 2048) nr = 2048;
                    if (nr > 16384) nr = 16384;
                    p->pre_nranges = (int)nr;
                }
                /* layout precompute granularity: per round unless
                 * DD_PRE_LAYOUT=seg */
                p->pre_layout = 2;
                if (const char *e = getenv("DD_PRE_LAYOUT")) {
                    if (strcmp(e, "seg") == 0) p->pre_layout = 1;
                    else if (strcmp(e, "round") != 0)
                        return fail(DD_ERR_INVALID, "DD_PRE_LAYOUT must be seg or round");
                }
                /* XCD-contiguous round order in K3: default only where it measured a win
                 * on the round layout — the 4-column shapes at P <= 128 (headline,
                 * dictkey) and at 257..512. It LOSES on the 5-column multikey tier and
                 * ties within noise on q1 and at 129..256.
                 * DD_PRE_XCD=0/1 overrides on any tier. */
                p->pre_xcd = p->pre_layout == 2 && batch->n_cols == 4 &&
                             (n_partitions <= 128 || n_partitions > 256);
                /* wide rounds: on at rpb 1 on all three tiers, the 5-column multikey
                 * included (K3 0.81 against 0.95-1.06 ms with it off, §13.6) */
                if (wide) p->pre_xcd = 1;
                if (const char *e = getenv("DD_PRE_XCD")) p->pre_xcd = atoi(e) == 1;
                /* round-granular scan: a thread walks <= span = 64 rounds; past 16*span
                 * ranges (> 65 k rounds) the range partials get a second level of
                 * span-range groups. DD_PRE_SCAN_SPAN (1..64) shrinks span so a small
                 * batch reaches the two-level form (tests). */
                int64_t span = 64;
                if (const char *e = getenv("DD_PRE_SCAN_SPAN")) {
                    int v = atoi(e);
                    if (v >= 1 && v <= 64) span = v;
                }
                p->round_nr1 = (int)((p->nrounds + span - 1) / span);
                p->round_nr2 =
                    p->round_nr1 > 16 * span ? (int)((p->round_nr1 + span - 1) / span) : 0;
                p->nchunks = p->nseg_pad;       /* counts rows (scan granularity) */
                p->chunk_rows = (int64_t)pgmax * 64; /* = SEG (K1seg rows per wave) */
                p->lds_k1 = (size_t)WAVES_PER_BLOCK_H * n_partitions * 4;
            }
        }
    }
    const int64_t nchunks = p->nchunks;

    /* rhash (opt-in, DD_RHASH=1): spec-path batches (wpb 16, all fixed, no validity)
     * with integer/bool keys recompute the row hash in K3 from its own key loads and
     * skip the pid array (4 B/row HBM write in K1 + read in K3). MEASURED NEGATIVE as a
     * default at the bench shape (K3 1.65-1.70 ms vs 1.30 ms, same box, both the
     * hash-after-preload and keys-first forms): the pid load's latency is fully hidden
     * in the staged pipeline, while pidr's dependency on hashed key loads stalls the
     * wave-synchronous rank() ballots — 0.24 GB less traffic does not buy back a 27%
     * stall. Kept parity-tested for re-evaluation on future silicon.
     * Must mirror the launcher's can_spec/can_spec8 conditions exactly
     * (dd_launch_scatter_staged fails loudly if not). */
    if (getenv("DD_RHASH") && atoi(getenv("DD_RHASH")) == 1 && p->staged && !p->pre &&
        p->wpb == 16 && nvar == 0 && batch->n_cols <= DD_STAGE_MAXC) {
        bool rhash = true;
        for (int c = 0; c < batch->n_cols && rhash; c++)
            if (batch->cols[c].validity || fixed_elem_size(batch->cols[c].dtype) == 0 ||
                fixed_elem_size(batch->cols[c].dtype) > 8) /* no 16-byte spec form */
                rhash = false;
        for (int k = 0; k < n_keys && rhash; k++) {
            const int dt = batch->cols[key_cols[k]].dtype;
            if (!(dt == DD_DT_U8 || dt == DD_DT_BOOL || dt == DD_DT_I16 ||
                  dt == DD_DT_I32 || dt == DD_DT_I64))
                rhash = false; /* float needs canon, dict32 a table gather: pid path */
        }
        ka.rhash = rhash ? 1 : 0;
    }

    /* hidden-load scatter (dd_kernels.hip HL header): default ON for its gated shape —
     * measured K3 1.015 vs 1.166 ms (−13 %), headline +10.6 % on the same box
     * (profiles/). DD_K3_HL=0 reverts to the plain spec path for A/B.
     * Gate must match the instantiated shapes exactly (4 fixed cols, elems 4/8, no
     * validity, gmax 4, wpb 16); mutually exclusive with rhash (HL reads the pid
     * array). */
    if (!ka.rhash && !p->pre && !(getenv("DD_K3_HL") && atoi(getenv("DD_K3_HL")) == 0) &&
        p->staged && p->wpb == 16 && p->gmax == 4 && nvar == 0 && batch->n_cols == 4) {
        bool okhl = true;
        for (int c = 0; c < 4; c++) {
            const int e = fixed_elem_size(batch->cols[c].dtype);
            if (batch->cols[c].validity || (e != 4 && e != 8)) okhl = false;
        }
        if (okhl) ka.hl = 1;
    }
    /* generalized HL (k_scatter_hlg): exact whitelisted shapes only — must mirror the
     * launcher's DD_HLG table */
    if (!ka.rhash && !ka.hl && !p->pre &&
        !(getenv("DD_K3_HL") && atoi(getenv("DD_K3_HL")) == 0) &&
        p->staged && p->wpb == 16) {
        bool novalid = true;
        for (int c = 0; c < batch->n_cols && novalid; c++)
            if (batch->cols[c].validity) novalid = false;
        auto elems_are = [&](std::initializer_list<int> want) {
            if ((int)want.size() != batch->n_cols) return false;
            int c = 0;
            for (int w : want)
                if (fixed_elem_size(batch->cols[c++].dtype) != w) return false;
            return true;
        };
        if (novalid && nvar == 0 &&
            ((p->gmax == 4 && elems_are({8, 8, 8, 4, 4})) ||
             (p->gmax == 2 && elems_are({1, 1, 8, 8, 8, 8, 4}))))
            ka.hl = 2;
    }

    /* K1 key signature (dd_hash_device.h): the tile / seg / round K1
     * kernels are instantiated for one or two non-nullable fixed-width keys of the kinds
     * below, where every key load of a wave's row groups issues before the first wait.
     * Anything else (a validity buffer on a key, utf8, three or more keys, other pairs),
     * the v1 path, and rhash (no pid array to store to) keep the generic body.
     * DD_K1_SPEC=0 forces the generic body for A/B. Must mirror DD_K1_TABLE. */
    if (p->staged && !ka.rhash && !(getenv("DD_K1_SPEC") && atoi(getenv("DD_K1_SPEC")) == 0)) {
        auto kind = [&](int k) {
            const dd_col_desc &cd = batch->cols[key_cols[k]];
            if (cd.validity) return (int)DD_KK_NONE;
            switch (cd.dtype) {
            case DD_DT_U8:
            case DD_DT_BOOL: return (int)DD_KK_B1;
            case DD_DT_I16: return (int)DD_KK_B2;
            case DD_DT_I32: return (int)DD_KK_B4;
            case DD_DT_I64: return (int)DD_KK_B8;
            case DD_DT_F32: return (int)DD_KK_F32;
            case DD_DT_F64: return (int)DD_KK_F64;
            case DD_DT_DICT32: return (int)DD_KK_DICT32;
            default: return (int)DD_KK_NONE;
            }
        };
        if (n_keys == 1) {
            p->k1_spec = DD_K1_CODE(kind(0), DD_KK_NONE);
        } else if (n_keys == 2) {
            const int k0 = kind(0), k1 = kind(1);
            if ((k0 == DD_KK_B8 && k1 == DD_KK_B4) || (k0 == DD_KK_B1 && k1 == DD_KK_B1))
                p->k1_spec = DD_K1_CODE(k0, k1);
        }
    }

    auto halloc = [&](void **ptr, size_t bytes) {
        return hipMalloc(ptr, bytes > 0 ? bytes : 1) == hipSuccess;
    };
    bool ok = (ka.rhash ? true
                        : halloc((void **)&p->pid, (size_t)n * (ka.pid8 ? 1 : 4))) &&
              halloc((void **)&p->counts, p->pre ? 4 : (size_t)nchunks * P * 4) &&
              halloc((void **)&p->partials,
                     p->pre_layout == 2
                         ? (size_t)p->round_nr1 * p->sP2 * 4
                         : (size_t)(p->pre ? p->pre_nranges : DD_SCAN_RANGES) * P * 4) &&
              halloc((void **)&p->part_offsets, (size_t)(P + 1) * 8);
    if (ok && p->pre_layout == 2) /* round-layout tables carry sP2 columns */
        ok = halloc((void **)&p->imgb, (size_t)p->nrounds * p->sP2 * 2) &&
             halloc((void **)&p->partials2, (size_t)(p->round_nr2 + 1) * p->sP2 * 4) &&
             halloc((void **)&p->counts16, (size_t)p->nseg_pad * p->sP2 * 2) &&
             halloc((void **)&p->roundcnt, (size_t)p->nrounds * p->sP2 * 4) &&
             halloc((void **)&p->rbase, (size_t)p->nrounds * p->sP2 * 4) &&
             halloc((void **)&p->totals, (size_t)p->sP2 * 4);
    else if (ok && p->pre)
        ok = halloc((void **)&p->imgb, (size_t)p->nrounds * p->sP2 * 2) &&
             halloc((void **)&p->partials2, (size_t)64 * P * 4) &&
             halloc((void **)&p->counts16, (size_t)p->nseg_pad * P * 2) &&
             halloc((void **)&p->gbase, (size_t)p->nseg_pad * P * 4);
    if (ok && nvar > 0) {
        ok = halloc((void **)&p->part_boffsets, (size_t)nvar * (P + 1) * 8);
        if (p->staged) {
            ok = ok && halloc((void **)&p->src_row, (size_t)n * 4) &&
                 halloc((void **)&p->k4_partials, (size_t)8192 * 8) &&
                 halloc((void **)&p->k4w_meta, (64 + 65) * 4) &&
                 halloc((void **)&p->k4w_order, ((size_t)(n + 63) / 64) * 4);
            for (int v = 0; v < nvar && ok; v++)
                ok = halloc((void **)&p->out_off[v], (size_t)(n + 1) * 8);
            /* K5 (LDS-staged var-byte scatter, dd_kernels.hip K5 header): one var
             * column with small strings. Needs the real max string length -> one tiny
             * create-time kernel + 4 B d2h (amortized across runs). DD_K5=0 reverts
             * to the K4 gather. */
            if (ok && nvar == 1 && n > 0 &&
                !(getenv("DD_K5") && atoi(getenv("DD_K5")) == 0)) {
                const dd_col_desc &vc = batch->cols[ka.var_idx[0]];
                uint32_t *mdev = nullptr;
                if (hipMalloc((void **)&mdev, 4) == hipSuccess) {
                    uint32_t maxlen = 0;
                    bool mok = hipMemset(mdev, 0, 4) == hipSuccess &&
                               dd_launch_k5_maxlen(vc.offsets, n, mdev, nullptr) ==
                                   hipSuccess &&
                               hipMemcpy(&maxlen, mdev, 4, hipMemcpyDeviceToHost) ==
                                   hipSuccess;
                    (void)hipFree(mdev);
                    int wpb5 = 16;
                    if (const char *e = getenv("DD_K5_WPB")) { /* experiment knob */
                        int v = atoi(e);
                        if (v == 8 || v == 16) wpb5 = v;
                    }
                    const int64_t R5 = (int64_t)wpb5 * 64;
                    const size_t img = (size_t)R5 * maxlen + 8;
                    /* k5_scatter's whole LDS: it declares no static __shared__ beside
                     * this dynamic carve, so the gate below is the launch limit */
                    const size_t lds5 =
                        (size_t)wpb5 * P * 4 + (size_t)(P + 1) * 4 + img;
                    if (mok && maxlen > 0 && maxlen <= 128 && lds5 <= 163840) {
                        p->k5_wpb = wpb5;
                        p->k5_nrounds = (n + R5 - 1) / R5;
                        p->k5_nseg = p->k5_nrounds * wpb5;
                        {
                            int64_t nr = p->k5_nseg / 114;
                            if (nr < 2048) nr = 2048;
                            if (nr > 16384) nr = 16384;
                            p->k5_nranges = (int)nr;
                        }
                        p->k5_maxlen = maxlen;
                        p->lds_k5 = lds5;
                        p->lds_k5c = (size_t)WAVES_PER_BLOCK_H * P * 4;
                        ok = halloc((void **)&p->k5_bcounts,
                                    (size_t)p->k5_nseg * P * 2) &&
                             halloc((void **)&p->k5_gbase,
                                    (size_t)p->k5_nseg * P * 4) &&
                             halloc((void **)&p->k5_partials,
                                    (size_t)p->k5_nranges * P * 4) &&
                             halloc((void **)&p->k5_partials2, (size_t)64 * P * 4) &&
                             halloc((void **)&p->k5_roffB,
                                    (size_t)p->k5_nrounds * (P + 1) * 4);
                        if (ok) p->k5 = 1;
                    }
                }
            }
        } else {
            ok = ok && halloc((void **)&p->bcounts, (size_t)nvar * nchunks * P * 4) &&
                 halloc((void **)&p->bpartials, (size_t)nvar * DD_SCAN_RANGES * P * 4);
        }
    }
    if (!ok) return fail(DD_ERR_HIP, "allocation failed (workspace)");

    for (int c = 0; c < batch->n_cols && ok; c++) {
        const dd_col_desc &cd = batch->cols[c];
        dd_kcol &kc = ka.cols[c];
        if (cd.dtype == DD_DT_UTF8) {
            ok = halloc(&p->out_data[c], (size_t)cd.data_len) &&
                 halloc((void **)&p->out_lengths[c], (size_t)n * 4);
            kc.out_lengths = p->out_lengths[c];
        } else {
            ok = halloc(&p->out_data[c], (size_t)n * kc.elem);
        }
        kc.out_data = p->out_data[c];
        if (ok && cd.validity) {
            ok = halloc((void **)&p->out_valid[c], (size_t)n);
            kc.out_valid = p->out_valid[c];
        }
        if (ok && cd.dtype == DD_DT_DICT32) {
            ok = halloc((void **)&p->dict_hashes[c], (size_t)cd.dict_n * 8);
            if (ok) {
                hipError_t e = dd_launch_dict_hashes((const uint8_t *)cd.dict_bytes,
                                                     cd.dict_offsets, cd.dict_n,
                                                     p->dict_hashes[c], nullptr);
                ok = (e == hipSuccess);
            }
            kc.dict_hashes = p->dict_hashes[c];
        }
    }
    if (!ok) return fail(DD_ERR_HIP, "allocation failed (outputs)");

    if (p->staged && nvar > 0) {
        /* synthetic staged columns: per var col its LENGTHS (u32, written partition-major
         * into out_lengths) and one ROWID permutation column (u32 -> src_row); the var
         * BYTES are materialized by K4 after the scatter (dd_kernels.hip K4 header) */
        for (int v = 0; v < nvar; v++) {
            const int ci = ka.var_idx[v];
            dd_kcol &kc = ka.cols[ka.n_cols];
            memset(&kc, 0, sizeof(kc));
            kc.dtype = DD_KDT_VARLEN;
            kc.elem = 4;
            kc.data = batch->cols[ci].offsets;
            kc.out_data = p->out_lengths[ci];
            ka.n_cols++;
        }
        if (!p->k5) { /* ROWID (src_row) only feeds the K4 gather; K5 replaces it */
            dd_kcol &kr = ka.cols[ka.n_cols];
            memset(&kr, 0, sizeof(kr));
            kr.dtype = DD_KDT_ROWID;
            kr.elem = 4;
            kr.out_data = p->src_row;
            ka.n_cols++;
        }
    }

    for (auto &e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(DD_ERR_HIP, "event create failed");

    *out = p;
    return DD_OK;
}

/* coarse-bucket partitioner: pid = (h % pid_total) >> log2(coarse_div). The effective
 * partition count is pid_total/coarse_div CONTIGUOUS ranges of the final partition space
 * — pass A of the two-level var scatter. Power-of-two args only. */
extern "C" dd_status dd_partitioner_create_ranged(const dd_batch_desc *batch,
                                                  const int32_t *key_cols, int32_t n_keys,
                                                  uint32_t pid_total, uint32_t coarse_div,
                                                  dd_partitioner **out) {
    if (coarse_div == 0 || (coarse_div & (coarse_div - 1)) != 0 ||
        (pid_total & (pid_total - 1)) != 0 || pid_total % coarse_div != 0)
        return set_err(DD_ERR_INVALID, "pid_total and coarse_div must be powers of two "
                                       "with coarse_div | pid_total");
    dd_status st = dd_partitioner_create(batch, key_cols, n_keys, pid_total / coarse_div,
                                         out);
    if (st != DD_OK) return st;
    (*out)->ka.pid_total = pid_total;
    int shift = 0;
    while ((1u << shift) < coarse_div) shift++;
    (*out)->ka.pid_shift = shift;
    return DD_OK;
}

extern "C" dd_status dd_partitioner_run_phase1(dd_partitioner *p, void *stream) {
    if (!p) return set_err(DD_ERR_INVALID, "null partitioner");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipEventRecord(p->ev[0], s));
    if (p->pre_layout == 2) {
        HIP_TRY(dd_launch_hash_count_round(&p->ka, p->k1_spec, p->nrounds, p->chunk_rows, p->wpb,
                                           p->nparts, p->sP2, p->pid, p->counts16,
                                           p->roundcnt, p->imgb, s));
    } else if (p->pre) {
        HIP_TRY(hipMemsetAsync(p->partials, 0, (size_t)p->pre_nranges * p->nparts * 4, s));
        HIP_TRY(dd_launch_hash_count_seg(&p->ka, p->k1_spec, p->nseg_pad, p->chunk_rows, p->nparts,
                                         p->nbits, p->pid, p->counts16, p->partials,
                                         p->pre_nranges, p->lds_k1, s));
    } else if (p->staged) {
        HIP_TRY(dd_launch_hash_count_tile(&p->ka, p->k1_spec, p->nchunks, p->chunk_rows, p->nparts,
                                          p->nbits, p->pid, p->counts, p->lds_k1, s));
    } else {
        HIP_TRY(dd_launch_hash_count(&p->ka, p->nchunks, p->chunk_rows, p->nparts, p->nbits,
                                     p->pid, p->counts, p->bcounts, p->lds_k1, s));
    }
    HIP_TRY(hipEventRecord(p->ev[1], s));
    if (p->pre_layout == 2) {
        HIP_TRY(dd_launch_scan_round(p->roundcnt, p->nrounds, p->nparts, p->sP2,
                                     p->round_nr1, p->round_nr2, p->partials,
                                     p->partials2, p->totals, p->part_offsets, p->rbase,
                                     s));
    } else if (p->pre) {
        HIP_TRY(dd_launch_scan_deep(p->counts16, p->nchunks, p->nparts, p->pre_nranges,
                                    64, p->partials, p->partials2, p->part_offsets,
                                    p->gbase, s));
    } else {
        HIP_TRY(dd_launch_scan(p->counts, p->nchunks, p->nparts, DD_SCAN_RANGES,
                               p->partials, p->part_offsets, 0, s));
    }
    if (p->pre_layout == 1) {
        HIP_TRY(dd_launch_round_layout(p->gbase, p->part_offsets, p->nrounds, p->wpb,
                                       p->nparts, p->sP2, p->imgb, s));
    }
    if (p->k5) { /* byte-base precompute for the K5 var scatter */
        const int ci = p->ka.var_idx[0];
        HIP_TRY(hipMemsetAsync(p->k5_partials, 0,
                               (size_t)p->k5_nranges * p->nparts * 4, s));
        HIP_TRY(dd_launch_k5_count(p->ka.n_rows, p->nparts, p->pid,
                                   p->batch.cols[ci].offsets, p->k5_bcounts,
                                   p->k5_partials, p->k5_nranges, p->k5_nseg,
                                   p->lds_k5c, s));
        HIP_TRY(dd_launch_scan_deep(p->k5_bcounts, p->k5_nseg, p->nparts, p->k5_nranges,
                                    64, p->k5_partials, p->k5_partials2,
                                    p->part_boffsets, p->k5_gbase, s));
        HIP_TRY(dd_launch_k5_roff(p->k5_gbase, p->part_boffsets, p->k5_nrounds,
                                  p->k5_wpb, p->nparts, p->k5_roffB, s));
    }
    if (!p->staged) {
        for (int v = 0; v < p->ka.n_var; v++) {
            HIP_TRY(dd_launch_scan(p->bcounts + (size_t)v * p->nchunks * p->nparts,
                                   p->nchunks, p->nparts, DD_SCAN_RANGES,
                                   p->bpartials + (size_t)v * DD_SCAN_RANGES * p->nparts,
                                   p->part_boffsets + (size_t)v * (p->nparts + 1), 0, s));
        }
    }
    HIP_TRY(hipEventRecord(p->ev[2], s));
    return DD_OK;
}

extern "C" dd_status dd_partitioner_run_phase2(dd_partitioner *p, void *stream) {
    if (!p) return set_err(DD_ERR_INVALID, "null partitioner");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipEventRecord(p->ev[4], s)); /* K3 start on the phase2 stream */
    if (p->pre_wide) {
        const int64_t nblocks = (p->nrounds + p->rpb - 1) / p->rpb;
        HIP_TRY(dd_launch_scatter_pre_wide(&p->ka, nblocks, p->nrounds, p->rpb, p->nparts,
                                           p->nbits, p->pid, p->imgb, p->sP2, p->counts16,
                                           p->rbase, p->pre_xcd, p->lds_k3, s));
    } else if (p->pre) {
        const int64_t nblocks = (p->nrounds + p->rpb - 1) / p->rpb;
        HIP_TRY(dd_launch_scatter_pre(&p->ka, nblocks, p->nrounds, p->rpb, p->nparts,
                                      p->nbits, p->pid, p->gbase, p->imgb, p->sP2,
                                      p->counts16, p->rbase, p->pre_layout, p->pre_xcd,
                                      p->gmax, p->wpb, p->lds_k3, s));
    } else if (p->staged) {
        HIP_TRY(dd_launch_scatter_staged(&p->ka, p->nchunks, p->chunk_rows, p->nparts,
                                         p->nbits, p->pid, p->counts, p->part_offsets,
                                         p->gmax, p->wpb, p->lds_k3, s));
        for (int v = 0; v < p->ka.n_var; v++) {
            const int ci = p->ka.var_idx[v];
            const dd_col_desc &cd = p->batch.cols[ci];
            HIP_TRY(dd_launch_var_bytes(
                p->out_lengths[ci], p->src_row, cd.offsets, (const uint8_t *)cd.data,
                p->ka.n_rows, p->k4_partials, p->out_off[v],
                (uint8_t *)p->out_data[ci], p->part_offsets, p->nparts,
                p->part_boffsets + (size_t)v * (p->nparts + 1), p->k4w_meta,
                p->k4w_order, p->k5 ? 1 : 0, s));
            if (p->k5) {
                HIP_TRY(dd_launch_k5_scatter(
                    p->ka.n_rows, p->nparts, p->nbits, p->pid, cd.offsets,
                    (const uint8_t *)cd.data, p->k5_gbase, p->k5_roffB, p->k5_nrounds,
                    (uint8_t *)p->out_data[ci], p->k5_wpb, p->lds_k5, s));
            }
        }
    } else {
        HIP_TRY(dd_launch_scatter(&p->ka, p->nchunks, p->chunk_rows, p->nparts, p->nbits,
                                  p->pid, p->counts, p->part_offsets, p->bcounts,
                                  p->part_boffsets, p->lds_k3, s));
    }
    HIP_TRY(hipEventRecord(p->ev[3], s));
    p->has_run.store(true, std::memory_order_release);
    return DD_OK;
}

extern "C" dd_status dd_partitioner_wait_phase1(dd_partitioner *p, void *stream) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, p->ev[2], 0));
    return DD_OK;
}

extern "C" dd_status dd_partitioner_wait_phase2(dd_partitioner *p, void *stream) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, p->ev[3], 0));
    return DD_OK;
}

extern "C" dd_status dd_partitioner_run(dd_partitioner *p, void *stream) {
    dd_status st = dd_partitioner_run_phase1(p, stream);
    if (st != DD_OK) return st;
    return dd_partitioner_run_phase2(p, stream);
}

extern "C" void dd_partitioner_destroy(dd_partitioner *p) { delete p; }

extern "C" int32_t dd_partitioner_pid_elem(const dd_partitioner *p) {
    return p->ka.pid8 ? 1 : 4;
}

extern "C" int32_t dd_partitioner_pre_layout(const dd_partitioner *p) {
    return p ? p->pre_layout : 0;
}

extern "C" int32_t dd_partitioner_pre_wide(const dd_partitioner *p) {
    return p && p->pre_wide ? 1 : 0;
}

extern "C" int32_t dd_partitioner_k1_spec(const dd_partitioner *p) {
    return p ? p->k1_spec : 0;
}

extern "C" void dd_pre_xcd_block_map(int64_t nblocks, int64_t *out) {
    for (int64_t b = 0; b < nblocks; b++) out[b] = dd_xcd_block_map(b, nblocks);
}

extern "C" dd_status dd_partitioner_get_info(const dd_partitioner *p,
                                             dd_partitioner_info *out) {
    if (!p || !out) return set_err(DD_ERR_INVALID, "null argument");
    const bool tiled = p->staged || p->pre;
    out->path = p->pre ? 2 : (p->staged ? 1 : 0);
    out->wpb = tiled ? p->wpb : 0;
    out->gmax = tiled ? p->gmax : 0;
    out->hl = p->ka.hl;
    out->rhash = p->ka.rhash;
    out->pid_elem = p->ka.pid8 ? 1 : 4;
    out->k5 = p->k5;
    out->k5_wpb = p->k5 ? p->k5_wpb : 0;
    out->k5_maxlen = (int32_t)p->k5_maxlen;
    out->rpb = p->pre ? p->rpb : 0;
    out->round_rows = tiled ? (int64_t)p->gmax * p->wpb * 64 : 0;
    out->n_launch = p->pre ? p->nrounds : p->nchunks;
    return DD_OK;
}

extern "C" const uint32_t *dd_partitioner_pids(const dd_partitioner *p) { return p->pid; }
extern "C" const void *dd_partitioner_col_data(const dd_partitioner *p, int32_t c) {
    return (c >= 0 && c < p->batch.n_cols) ? p->out_data[c] : nullptr;
}
extern "C" const uint8_t *dd_partitioner_col_validity(const dd_partitioner *p, int32_t c) {
    return (c >= 0 && c < p->batch.n_cols) ? p->out_valid[c] : nullptr;
}
extern "C" const uint32_t *dd_partitioner_col_lengths(const dd_partitioner *p, int32_t c) {
    return (c >= 0 && c < p->batch.n_cols) ? p->out_lengths[c] : nullptr;
}

extern "C" dd_status dd_partitioner_row_offsets(const dd_partitioner *p, int64_t *host_out) {
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    HIP_TRY(hipMemcpy(host_out, p->part_offsets, (size_t)(p->nparts + 1) * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

extern "C" const uint64_t *dd_partitioner_var_offsets64(const dd_partitioner *p,
                                                        int32_t col) {
    if (!p->staged) return nullptr;
    for (int v = 0; v < p->ka.n_var; v++)
        if (p->ka.var_idx[v] == col) return p->out_off[v];
    return nullptr;
}

extern "C" dd_status dd_make_offsets32(const uint64_t *off64, int64_t lo_row, int64_t n,
                                       int32_t *out32, void *stream) {
    if (!off64 || !out32) return set_err(DD_ERR_INVALID, "null argument");
    HIP_TRY(dd_launch_off64_to_off32(off64, lo_row, n, out32, (hipStream_t)stream));
    return DD_OK;
}

extern "C" dd_status dd_partitioner_byte_offsets(const dd_partitioner *p, int32_t col,
                                                 int64_t *host_out) {
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    for (int v = 0; v < p->ka.n_var; v++) {
        if (p->ka.var_idx[v] == col) {
            HIP_TRY(hipMemcpy(host_out, p->part_boffsets + (size_t)v * (p->nparts + 1),
                              (size_t)(p->nparts + 1) * 8, hipMemcpyDeviceToHost));
            return DD_OK;
        }
    }
    return set_err(DD_ERR_INVALID, "not a var column");
}

extern "C" dd_status dd_partitioner_kernel_ms(const dd_partitioner *p, float out_ms[3]) {
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    HIP_TRY(hipEventSynchronize(p->ev[3]));
    HIP_TRY(hipEventElapsedTime(&out_ms[0], p->ev[0], p->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out_ms[1], p->ev[1], p->ev[2]));
    HIP_TRY(hipEventElapsedTime(&out_ms[2], p->ev[4], p->ev[3]));
    return DD_OK;
}

/* ---------------- task cache (mirrors src/worker/task_data.rs, worker_service.rs:12,31) --- */

struct TaskKeyCmp {
    bool operator()(const dd_task_key &a, const dd_task_key &b) const {
        return memcmp(&a, &b, sizeof(a)) < 0;
    }
};

/* Entries are shared_ptr so a concurrent dd_drop_task / dd_set_plan replacing the key
 * cannot free the partitioner out from under an in-flight dd_execute_task (the execute
 * call pins its own reference for the duration of the call — the reference worker keeps
 * task state alive the same way via Arc'd entries in its TTI cache, task_data.rs:16-29).
 * The raw pointer RETURNED to the caller is only guaranteed while the cache entry lives:
 * see the lifetime note on dd_execute_task in dd_shuffle.h. */
static std::mutex g_tasks_mu;
static std::map<dd_task_key, std::shared_ptr<dd_partitioner>, TaskKeyCmp> g_tasks;

extern "C" dd_status dd_set_plan(const dd_task_key *key, const dd_batch_desc *batch,
                                 const int32_t *key_cols, int32_t n_keys,
                                 uint32_t n_partitions) {
    if (!key) return set_err(DD_ERR_INVALID, "null key");
    dd_partitioner *p = nullptr;
    dd_status st = dd_partitioner_create(batch, key_cols, n_keys, n_partitions, &p);
    if (st != DD_OK) return st;
    std::shared_ptr<dd_partitioner> sp(p, dd_partitioner_destroy);
    std::lock_guard<std::mutex> g(g_tasks_mu);
    g_tasks[*key] = std::move(sp); /* replaces; pinned in-flight executes keep the old one */
    return DD_OK;
}

extern "C" dd_status dd_execute_task(const dd_task_key *key, uint32_t part_lo, uint32_t part_hi,
                                     void *stream, dd_partitioner **out) {
    if (!key || !out) return set_err(DD_ERR_INVALID, "null argument");
    std::shared_ptr<dd_partitioner> pin; /* keeps p alive for the whole call */
    {
        std::lock_guard<std::mutex> g(g_tasks_mu);
        auto it = g_tasks.find(*key);
        if (it == g_tasks.end())
            return set_err(DD_ERR_NOT_FOUND,
                           "unknown TaskKey (no plan was set: cf. impl_execute_task.rs:29-34)");
        pin = it->second;
    }
    dd_partitioner *p = pin.get();
    if (part_lo > part_hi || part_hi > p->nparts)
        return set_err(DD_ERR_INVALID, "partition range out of bounds");
    if (!p->has_run.load(std::memory_order_acquire)) {
        /* run under the cache lock: launches are async enqueues (cheap), and this keeps
         * two concurrent execute_task calls on the same key from double-launching */
        std::lock_guard<std::mutex> g(g_tasks_mu);
        if (!p->has_run.load(std::memory_order_relaxed)) {
            dd_status st = dd_partitioner_run(p, stream);
            if (st != DD_OK) return st;
        }
    }
    *out = p;
    return DD_OK;
}

extern "C" dd_status dd_drop_task(const dd_task_key *key) {
    std::shared_ptr<dd_partitioner> dead; /* destroy outside the lock */
    std::lock_guard<std::mutex> g(g_tasks_mu);
    auto it = g_tasks.find(*key);
    if (it == g_tasks.end()) return set_err(DD_ERR_NOT_FOUND, "unknown TaskKey");
    dead = std::move(it->second);
    g_tasks.erase(it);
    return DD_OK;
}

/* ---------------- RCCL exchange ---------------- */

struct dd_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    ~dd_comm() {
        if (comm) ncclCommDestroy(comm);
    }
};

extern "C" dd_status dd_comm_unique_id(void *bytes128) {
    if (!bytes128) return set_err(DD_ERR_INVALID, "null argument");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(bytes128, &id, sizeof(id));
    return DD_OK;
}

extern "C" dd_status dd_comm_init(const void *bytes128, int rank, int nranks, dd_comm **out) {
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");
    auto c = new dd_comm();
    c->rank = rank;
    c->nranks = nranks;
    ncclUniqueId id;
    memcpy(&id, bytes128, sizeof(id));
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        delete c;
        return set_err(DD_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    *out = c;
    return DD_OK;
}

extern "C" void dd_comm_destroy(dd_comm *c) { delete c; }

/* allgather of the per-rank size matrix (exchange + coalesce); device staging buffers are
 * freed on every path, including RCCL/HIP failure */
static dd_status dd_meta_allgather(dd_comm *c, const std::vector<int64_t> &mine,
                                   std::vector<int64_t> &all, hipStream_t s) {
    const size_t meta_n = mine.size();
    int64_t *d_in = nullptr, *d_all = nullptr;
    HIP_TRY(hipMalloc(&d_in, meta_n * 8));
    if (hipMalloc(&d_all, all.size() * 8) != hipSuccess) {
        (void)hipFree(d_in);
        return set_err(DD_ERR_HIP, "meta allgather alloc");
    }
    hipError_t he = hipMemcpyAsync(d_in, mine.data(), meta_n * 8, hipMemcpyHostToDevice, s);
    ncclResult_t nr = ncclSuccess;
    if (he == hipSuccess) nr = ncclAllGather(d_in, d_all, meta_n, ncclInt64, c->comm, s);
    if (he == hipSuccess && nr == ncclSuccess) he = hipStreamSynchronize(s);
    if (he == hipSuccess && nr == ncclSuccess)
        he = hipMemcpy(all.data(), d_all, all.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_all);
    if (nr != ncclSuccess)
        return set_err(DD_ERR_RCCL, std::string("size allgather: ") + ncclGetErrorString(nr));
    if (he != hipSuccess)
        return set_err(DD_ERR_HIP, std::string("size allgather: ") + hipGetErrorString(he));
    return DD_OK;
}

/* ---------------- broadcast (dd_bcast) ---------------- */

struct dd_bcast {
    int64_t n_rows = 0;
    int32_t n_cols = 0;
    int32_t dtypes[DD_MAX_COLS] = {};
    int64_t data_lens[DD_MAX_COLS] = {};
    void *data[DD_MAX_COLS] = {};
    uint8_t *valid[DD_MAX_COLS] = {};
    int32_t *offsets[DD_MAX_COLS] = {};
    void *dict_bytes[DD_MAX_COLS] = {};
    int32_t *dict_offsets[DD_MAX_COLS] = {};
    bool owns = false; /* non-root ranks own their buffers */
    ~dd_bcast() {
        if (!owns) return;
        for (int i = 0; i < DD_MAX_COLS; i++) {
            (void)hipFree(data[i]);
            (void)hipFree(valid[i]);
            (void)hipFree(offsets[i]);
            (void)hipFree(dict_bytes[i]);
            (void)hipFree(dict_offsets[i]);
        }
    }
};

/* header: [n_rows, n_cols] + per col [dtype, data_bytes, has_valid, n_offsets, dict_n,
 * dict_bytes_len] — broadcast first so non-root ranks can allocate */
#define DD_BHDR (2 + DD_MAX_COLS * 6)

extern "C" dd_status dd_broadcast_run(dd_comm *c, const dd_batch_desc *batch, int root,
                                      void *stream, dd_bcast **out) {
    if (!c || !out) return set_err(DD_ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const bool is_root = c->rank == root;
    if (is_root && !batch) return set_err(DD_ERR_INVALID, "root needs a batch");

    int64_t hdr[DD_BHDR] = {};
    if (is_root) {
        hdr[0] = batch->n_rows;
        hdr[1] = batch->n_cols;
        for (int i = 0; i < batch->n_cols; i++) {
            const dd_col_desc &cd = batch->cols[i];
            int64_t *h = hdr + 2 + (size_t)i * 6;
            h[0] = cd.dtype;
            h[1] = (cd.dtype == DD_DT_UTF8) ? cd.data_len
                                            : batch->n_rows * fixed_elem_size(cd.dtype);
            h[2] = cd.validity ? 1 : 0;
            h[3] = cd.offsets ? batch->n_rows + 1 : 0;
            h[4] = cd.dict_n;
            h[5] = (cd.dtype == DD_DT_DICT32 && cd.dict_offsets)
                       ? 0 /* filled below via D2H of last offset */
                       : 0;
        }
        /* dict byte lengths require the last dict offset */
        for (int i = 0; i < batch->n_cols; i++) {
            const dd_col_desc &cd = batch->cols[i];
            if (cd.dtype == DD_DT_DICT32 && cd.dict_n > 0) {
                int32_t last = 0;
                HIP_TRY(hipMemcpy(&last, cd.dict_offsets + cd.dict_n, 4,
                                  hipMemcpyDeviceToHost));
                hdr[2 + (size_t)i * 6 + 5] = last;
            }
        }
    }
    int64_t *d_hdr = nullptr;
    HIP_TRY(hipMalloc(&d_hdr, sizeof(hdr)));
    {
        /* merged checks so d_hdr is freed on every path */
        hipError_t he = hipSuccess;
        ncclResult_t nr = ncclSuccess;
        if (is_root) he = hipMemcpyAsync(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, s);
        if (he == hipSuccess)
            nr = ncclBroadcast(d_hdr, d_hdr, DD_BHDR, ncclInt64, root, c->comm, s);
        if (he == hipSuccess && nr == ncclSuccess) he = hipStreamSynchronize(s);
        if (he == hipSuccess && nr == ncclSuccess)
            he = hipMemcpy(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost);
        (void)hipFree(d_hdr);
        if (nr != ncclSuccess)
            return set_err(DD_ERR_RCCL,
                           std::string("header broadcast: ") + ncclGetErrorString(nr));
        if (he != hipSuccess)
            return set_err(DD_ERR_HIP,
                           std::string("header broadcast: ") + hipGetErrorString(he));
    }

    std::unique_ptr<dd_bcast> b_own(new dd_bcast()); /* freed on every error return */
    dd_bcast *b = b_own.get();
    b->n_rows = hdr[0];
    b->n_cols = (int32_t)hdr[1];
    b->owns = !is_root;
    auto fail = [&](const char *m) { return set_err(DD_ERR_HIP, m); };
    for (int i = 0; i < b->n_cols; i++) {
        const int64_t *h = hdr + 2 + (size_t)i * 6;
        b->dtypes[i] = (int32_t)h[0];
        b->data_lens[i] = h[1];
        if (is_root) {
            const dd_col_desc &cd = batch->cols[i];
            b->data[i] = const_cast<void *>(cd.data);
            b->valid[i] = const_cast<uint8_t *>(cd.validity);
            b->offsets[i] = const_cast<int32_t *>(cd.offsets);
            b->dict_bytes[i] = const_cast<void *>(cd.dict_bytes);
            b->dict_offsets[i] = const_cast<int32_t *>(cd.dict_offsets);
        } else {
            if (hipMalloc(&b->data[i], (size_t)h[1] + 1) != hipSuccess)
                return fail("bcast alloc data");
            if (h[2] && hipMalloc((void **)&b->valid[i], (size_t)b->n_rows + 1) != hipSuccess)
                return fail("bcast alloc valid");
            if (h[3] && hipMalloc((void **)&b->offsets[i], (size_t)h[3] * 4) != hipSuccess)
                return fail("bcast alloc offsets");
            if (h[4]) {
                if (hipMalloc(&b->dict_bytes[i], (size_t)h[5] + 1) != hipSuccess ||
                    hipMalloc((void **)&b->dict_offsets[i], ((size_t)h[4] + 1) * 4) !=
                        hipSuccess)
                    return fail("bcast alloc dict");
            }
        }
    }
    NCCL_TRY(ncclGroupStart());
    for (int i = 0; i < b->n_cols; i++) {
        const int64_t *h = hdr + 2 + (size_t)i * 6;
        if (h[1] > 0)
            NCCL_TRY(ncclBroadcast(b->data[i], b->data[i], h[1], ncclUint8, root, c->comm, s));
        if (h[2] && b->n_rows > 0)
            NCCL_TRY(ncclBroadcast(b->valid[i], b->valid[i], b->n_rows, ncclUint8, root,
                                   c->comm, s));
        if (h[3])
            NCCL_TRY(ncclBroadcast(b->offsets[i], b->offsets[i], h[3] * 4, ncclUint8, root,
                                   c->comm, s));
        if (h[4]) {
            if (h[5] > 0)
                NCCL_TRY(ncclBroadcast(b->dict_bytes[i], b->dict_bytes[i], h[5], ncclUint8,
                                       root, c->comm, s));
            NCCL_TRY(ncclBroadcast(b->dict_offsets[i], b->dict_offsets[i], (h[4] + 1) * 4,
                                   ncclUint8, root, c->comm, s));
        }
    }
    NCCL_TRY(ncclGroupEnd());
    HIP_TRY(hipStreamSynchronize(s));
    *out = b_own.release();
    return DD_OK;
}

extern "C" void dd_bcast_destroy(dd_bcast *b) { delete b; }
extern "C" int64_t dd_bcast_n_rows(const dd_bcast *b) { return b->n_rows; }
extern "C" int32_t dd_bcast_n_cols(const dd_bcast *b) { return b->n_cols; }
extern "C" const void *dd_bcast_col_data(const dd_bcast *b, int32_t col) {
    return (col >= 0 && col < b->n_cols) ? b->data[col] : nullptr;
}
extern "C" const uint8_t *dd_bcast_col_validity(const dd_bcast *b, int32_t col) {
    return (col >= 0 && col < b->n_cols) ? b->valid[col] : nullptr;
}
extern "C" const int32_t *dd_bcast_col_offsets(const dd_bcast *b, int32_t col) {
    return (col >= 0 && col < b->n_cols) ? b->offsets[col] : nullptr;
}
extern "C" dd_status dd_bcast_col_meta(const dd_bcast *b, int32_t col, int32_t *dtype,
                                       int64_t *data_len) {
    if (col < 0 || col >= b->n_cols) return set_err(DD_ERR_INVALID, "col out of range");
    *dtype = b->dtypes[col];
    *data_len = b->data_lens[col];
    return DD_OK;
}

/* ---------------- dictionary GC (dd_dict_gc; kernels in dd_dictgc.hip) ----------------
 * Device statement of the reference's pre-wire dictionary compaction
 * (garbage_collect_arrays, src/protocol/grpc/worker_service.rs:363-433). */

struct dd_dict_gc {
    const dd_partitioner *p = nullptr;
    int32_t col = -1;
    uint32_t W = 0, nw = 0, dict_n = 0;
    int64_t n_rows = 0;
    int lds = 0;
    std::vector<int64_t> val_off, byte_off; /* host prefix sums [W+1] */
    dd_gc_tile *tiles = nullptr;
    uint32_t *bits = nullptr, *prefix = nullptr; /* [W][nw] */
    uint32_t *nvals = nullptr;                   /* [W] */
    uint64_t *nbytes = nullptr;                  /* [W] */
    uint32_t *flag = nullptr;
    int64_t *d_off = nullptr; /* device copies: val_off [W+1] then byte_off [W+1] */
    int32_t *indices = nullptr;
    int32_t *offs = nullptr;
    uint8_t *bytes = nullptr;
    hipEvent_t ev[6] = {}; /* mark: 0-1, rank: 1-2, compact: 3-4, remap: 4-5 */
    ~dd_dict_gc() {
        (void)hipFree(tiles);
        (void)hipFree(bits);
        (void)hipFree(prefix);
        (void)hipFree(nvals);
        (void)hipFree(nbytes);
        (void)hipFree(flag);
        (void)hipFree(d_off);
        (void)hipFree(indices);
        (void)hipFree(offs);
        (void)hipFree(bytes);
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" dd_status dd_dict_gc_run(const dd_partitioner *p, int32_t col, uint32_t n_windows,
                                    void *stream, dd_dict_gc **out) {
    if (!p || !out) return set_err(DD_ERR_INVALID, "null argument");
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    if (col < 0 || col >= p->batch.n_cols || p->batch.cols[col].dtype != DD_DT_DICT32)
        return set_err(DD_ERR_INVALID, "dictionary GC needs a dict32 column");
    if (n_windows == 0 || p->nparts % n_windows != 0)
        return set_err(DD_ERR_INVALID, "n_windows must be > 0 and divide P_total");
    const dd_col_desc &cd = p->batch.cols[col];
    if (cd.dict_n < 0 || cd.dict_n > INT32_MAX || (cd.dict_n > 0 && !cd.dict_offsets))
        return set_err(DD_ERR_INVALID, "bad dictionary (dict_n / dict_offsets)");
    const uint64_t nw64 = ((uint64_t)cd.dict_n + 31) / 32;
    if (nw64 * n_windows > (1ull << 28))
        return set_err(DD_ERR_UNSUPPORTED,
                       "dictionary GC bitmap n_windows * ceil(dict_n/32) exceeds 2^28 words "
                       "(1 GiB): use fewer windows");
    hipStream_t s = (hipStream_t)stream;

    std::unique_ptr<dd_dict_gc> g(new dd_dict_gc());
    g->p = p;
    g->col = col;
    g->W = n_windows;
    g->nw = (uint32_t)nw64;
    g->dict_n = (uint32_t)cd.dict_n;
    g->n_rows = p->batch.n_rows;
    /* DD_GC_LDS=0 forces the global tier (A/B knob, read per call) */
    g->lds = g->nw <= DD_GC_LDS_MAX_WORDS &&
             !(getenv("DD_GC_LDS") && atoi(getenv("DD_GC_LDS")) == 0);
    const uint32_t W = g->W, nw = g->nw;

    /* tile table from the host-known row offsets: no tile straddles a window; skewed
     * windows split into many tiles; empty windows produce none. The LDS tier amortises
     * staging the nw-word bitmap over >= 8 rows per word. */
    std::vector<int64_t> roff(p->nparts + 1);
    dd_status st = dd_partitioner_row_offsets(p, roff.data());
    if (st != DD_OK) return st;
    int64_t tile_rows = 8192;
    if (g->lds) {
        tile_rows = (((int64_t)nw * 8 + 1023) / 1024) * 1024;
        if (tile_rows < 4096) tile_rows = 4096;
        if (tile_rows > 32768) tile_rows = 32768;
    }
    const uint32_t ppw = p->nparts / W;
    std::vector<dd_gc_tile> tiles;
    for (uint32_t w = 0; w < W; w++) {
        const int64_t lo = roff[(size_t)w * ppw], hi = roff[(size_t)(w + 1) * ppw];
        for (int64_t r = lo; r < hi; r += tile_rows)
            tiles.push_back({r, r + tile_rows < hi ? r + tile_rows : hi, w, 0u});
    }
    const int64_t n_tiles = (int64_t)tiles.size();
    if (n_tiles > INT32_MAX) return set_err(DD_ERR_UNSUPPORTED, "too many GC tiles");

    const size_t words = (size_t)W * nw;
    HIP_TRY(hipMalloc((void **)&g->tiles, (n_tiles ? n_tiles : 1) * sizeof(dd_gc_tile)));
    HIP_TRY(hipMalloc((void **)&g->bits, words * 4 + 4));
    HIP_TRY(hipMalloc((void **)&g->prefix, words * 4 + 4));
    HIP_TRY(hipMalloc((void **)&g->nvals, (size_t)W * 4));
    HIP_TRY(hipMalloc((void **)&g->nbytes, (size_t)W * 8));
    HIP_TRY(hipMalloc((void **)&g->flag, 4));
    HIP_TRY(hipMalloc((void **)&g->d_off, (size_t)(W + 1) * 16));
    HIP_TRY(hipMalloc((void **)&g->indices, (size_t)g->n_rows * 4 + 4));
    for (auto &e : g->ev) HIP_TRY(hipEventCreate(&e));
    if (n_tiles)
        HIP_TRY(hipMemcpyAsync(g->tiles, tiles.data(), n_tiles * sizeof(dd_gc_tile),
                               hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(g->bits, 0, words * 4 + 4, s));
    HIP_TRY(hipMemsetAsync(g->flag, 0, 4, s));

    const int32_t *idx = (const int32_t *)p->out_data[col];
    const uint8_t *valid = p->out_valid[col];
    HIP_TRY(hipEventRecord(g->ev[0], s));
    HIP_TRY(dd_launch_gc_mark(g->tiles, n_tiles, idx, valid, g->dict_n, nw, g->lds, g->bits,
                              g->flag, s));
    HIP_TRY(hipEventRecord(g->ev[1], s));
    HIP_TRY(dd_launch_gc_rank(g->bits, W, nw, cd.dict_offsets, g->prefix, g->nvals, g->nbytes,
                              s));
    HIP_TRY(hipEventRecord(g->ev[2], s));

    /* the one host sync: flag + per-window totals, to size the dictionaries */
    uint32_t flag_h = 0;
    std::vector<uint32_t> nvals_h(W);
    std::vector<uint64_t> nbytes_h(W);
    HIP_TRY(hipMemcpyAsync(&flag_h, g->flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nvals_h.data(), g->nvals, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nbytes_h.data(), g->nbytes, (size_t)W * 8, hipMemcpyDeviceToHost,
                           s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flag_h)
        return set_err(DD_ERR_INVALID, "dictionary GC: a valid row's index is outside "
                                       "[0, dict_n) (column " + std::to_string(col) + ")");
    g->val_off.assign(W + 1, 0);
    g->byte_off.assign(W + 1, 0);
    for (uint32_t w = 0; w < W; w++) {
        g->val_off[w + 1] = g->val_off[w] + nvals_h[w];
        g->byte_off[w + 1] = g->byte_off[w] + (int64_t)nbytes_h[w];
    }
    HIP_TRY(hipMalloc((void **)&g->offs, (size_t)(g->val_off[W] + W) * 4));
    HIP_TRY(hipMalloc((void **)&g->bytes, (size_t)g->byte_off[W] + 1));
    HIP_TRY(hipMemcpyAsync(g->d_off, g->val_off.data(), (size_t)(W + 1) * 8,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g->d_off + W + 1, g->byte_off.data(), (size_t)(W + 1) * 8,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(g->ev[3], s));
    HIP_TRY(dd_launch_gc_compact(g->bits, g->prefix, W, nw, cd.dict_offsets,
                                 (const uint8_t *)cd.dict_bytes, g->d_off, g->d_off + W + 1,
                                 g->offs, g->bytes, s));
    HIP_TRY(hipEventRecord(g->ev[4], s));
    HIP_TRY(dd_launch_gc_remap(g->tiles, n_tiles, idx, valid, g->dict_n, nw, g->lds, g->bits,
                               g->prefix, g->indices, s));
    HIP_TRY(hipEventRecord(g->ev[5], s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = g.release();
    return DD_OK;
}

extern "C" void dd_dict_gc_destroy(dd_dict_gc *g) { delete g; }
extern "C" int32_t dd_dict_gc_col(const dd_dict_gc *g) { return g ? g->col : -1; }
extern "C" uint32_t dd_dict_gc_n_windows(const dd_dict_gc *g) { return g ? g->W : 0; }
extern "C" const int32_t *dd_dict_gc_indices(const dd_dict_gc *g) { return g->indices; }
extern "C" const int32_t *dd_dict_gc_dict_offsets(const dd_dict_gc *g) { return g->offs; }
extern "C" const uint8_t *dd_dict_gc_dict_bytes(const dd_dict_gc *g) { return g->bytes; }

extern "C" dd_status dd_dict_gc_counts(const dd_dict_gc *g, int64_t *val_off,
                                       int64_t *byte_off) {
    if (!g || !val_off || !byte_off) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(val_off, g->val_off.data(), g->val_off.size() * 8);
    memcpy(byte_off, g->byte_off.data(), g->byte_off.size() * 8);
    return DD_OK;
}

extern "C" dd_status dd_dict_gc_kernel_ms(const dd_dict_gc *g, float out_ms[4]) {
    if (!g || !out_ms) return set_err(DD_ERR_INVALID, "null argument");
    HIP_TRY(hipEventSynchronize(g->ev[5]));
    HIP_TRY(hipEventElapsedTime(&out_ms[0], g->ev[0], g->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out_ms[1], g->ev[1], g->ev[2]));
    HIP_TRY(hipEventElapsedTime(&out_ms[2], g->ev[3], g->ev[4]));
    HIP_TRY(hipEventElapsedTime(&out_ms[3], g->ev[4], g->ev[5]));
    return DD_OK;
}

/* ---------------- view columns (dd_view_ingest / dd_view_emit; kernels in dd_views.hip) ---
 * Device statement of the view half of garbage_collect_arrays
 * (src/protocol/grpc/worker_service.rs:408-433). DESIGN.md §15. */

/* Copy tier knob, read per call: DD_VIEW_LDS=1 takes the LDS-staged tier, 0 or unset the
 * direct tier. Direct is the default because it measured 1.5-1.6x faster on the
 * clickbench_userid shape (profiles/r07_views.json). */
static int dd_view_lds_enabled(void) {
    const char *e = getenv("DD_VIEW_LDS");
    return e && atoi(e) != 0;
}

extern "C" int32_t dd_view_tile_rows(void) { return DD_VW_TILE_ROWS; }
extern "C" int32_t dd_view_image_bytes(void) { return DD_VW_IMAGE_BYTES; }

struct dd_view_ingest {
    int64_t n_rows = 0, n_tiles = 0, data_len = 0;
    int32_t tier = 0;
    int32_t *offs = nullptr;   /* [n_tiles * DD_VW_TILE_ROWS + 4]; offsets[n_rows+1] */
    uint8_t *bytes = nullptr;
    uint64_t *tsum = nullptr;  /* [n_tiles] then the scan [n_tiles+1] then meta[2] */
    uint32_t *flag = nullptr;
    void *tab = nullptr;       /* device: n_bufs pointers then n_bufs i64 lengths */
    hipEvent_t ev[5] = {};     /* len: 0-1, scan (+add): 1-2, copy: 3-4 */
    bool copied = false;
    ~dd_view_ingest() {
        (void)hipFree(offs);
        (void)hipFree(bytes);
        (void)hipFree(tsum);
        (void)hipFree(flag);
        (void)hipFree(tab);
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" dd_status dd_view_ingest_run(const void *views, const uint8_t *validity,
                                        int64_t n_rows, const void *const *data_bufs,
                                        const int64_t *data_buf_lens, int32_t n_bufs,
                                        void *stream, dd_view_ingest **out) {
    if (!out || n_rows < 0 || n_bufs < 0 || (n_rows > 0 && !views) ||
        (n_bufs > 0 && (!data_bufs || !data_buf_lens)))
        return set_err(DD_ERR_INVALID, "dd_view_ingest_run: null or negative argument");
    if (((uintptr_t)views & 15) != 0)
        return set_err(DD_ERR_INVALID, "dd_view_ingest_run: views must be 16-byte aligned");
    for (int32_t b = 0; b < n_bufs; b++)
        if (data_buf_lens[b] < 0 || (data_buf_lens[b] > 0 && !data_bufs[b]))
            return set_err(DD_ERR_INVALID, "dd_view_ingest_run: bad data buffer " +
                                               std::to_string(b));
    if (n_rows >= (1ll << 32))
        return set_err(DD_ERR_UNSUPPORTED, "n_rows >= 2^32: chunk the batch");
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");
    hipStream_t s = (hipStream_t)stream;

    std::unique_ptr<dd_view_ingest> g(new dd_view_ingest());
    g->n_rows = n_rows;
    g->n_tiles = (n_rows + DD_VW_TILE_ROWS - 1) / DD_VW_TILE_ROWS;
    const int64_t nt = g->n_tiles;
    const int lds = dd_view_lds_enabled();
    HIP_TRY(hipMalloc((void **)&g->offs, ((size_t)nt * DD_VW_TILE_ROWS + 4) * 4));
    HIP_TRY(hipMalloc((void **)&g->tsum, (size_t)(2 * nt + 3) * 8));
    HIP_TRY(hipMalloc((void **)&g->flag, 4));
    HIP_TRY(hipMalloc(&g->tab, (size_t)(n_bufs ? n_bufs : 1) * 16));
    for (auto &e : g->ev) HIP_TRY(hipEventCreate(&e));
    uint64_t *scan = g->tsum + nt, *meta = g->tsum + 2 * nt + 1;
    const uint8_t *const *d_bufs = (const uint8_t *const *)g->tab;
    const int64_t *d_lens = (const int64_t *)((char *)g->tab + (size_t)n_bufs * 8);
    if (n_bufs) {
        HIP_TRY(hipMemcpyAsync(g->tab, data_bufs, (size_t)n_bufs * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync((void *)d_lens, data_buf_lens, (size_t)n_bufs * 8,
                               hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(g->flag, 0, 4, s));

    HIP_TRY(hipEventRecord(g->ev[0], s));
    HIP_TRY(dd_launch_vw_len(views, validity, n_rows, d_lens, n_bufs, g->offs, g->tsum,
                             g->flag, s));
    HIP_TRY(hipEventRecord(g->ev[1], s));
    HIP_TRY(dd_launch_vw_scan(g->tsum, nt, 1, scan, meta, g->offs + n_rows, s));
    HIP_TRY(dd_launch_vw_add(g->offs, nt, scan, s));
    HIP_TRY(hipEventRecord(g->ev[2], s));

    /* the one host sync: flag, byte total, and how many tiles outgrow the LDS image */
    uint32_t flag_h = 0;
    uint64_t meta_h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&flag_h, g->flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(meta_h, meta, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flag_h)
        return set_err(DD_ERR_INVALID,
                       "view ingest: a valid row has a negative length or points outside "
                       "its data buffer (buffer_index / offset / length)");
    if (meta_h[0] > (uint64_t)INT32_MAX)
        return set_err(DD_ERR_UNSUPPORTED,
                       "view ingest: value bytes exceed INT32_MAX: chunk the rows");
    g->data_len = (int64_t)meta_h[0];
    /* LDS-staged when the knob asks for it, unless every tile outgrew the image */
    g->tier = lds && (nt == 0 || (int64_t)meta_h[1] < nt);
    HIP_TRY(hipMalloc((void **)&g->bytes, (size_t)g->data_len + 8));
    HIP_TRY(hipEventRecord(g->ev[3], s));
    if (g->data_len)
        HIP_TRY(dd_launch_vw_copy(views, n_rows, d_bufs, g->offs, g->bytes, g->tier, s));
    HIP_TRY(hipEventRecord(g->ev[4], s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = g.release();
    return DD_OK;
}

extern "C" const int32_t *dd_view_ingest_offsets(const dd_view_ingest *g) {
    return g ? g->offs : nullptr;
}
extern "C" const uint8_t *dd_view_ingest_bytes(const dd_view_ingest *g) {
    return g ? g->bytes : nullptr;
}
extern "C" int64_t dd_view_ingest_data_len(const dd_view_ingest *g) {
    return g ? g->data_len : -1;
}
extern "C" int32_t dd_view_ingest_tier(const dd_view_ingest *g) { return g ? g->tier : -1; }
extern "C" void dd_view_ingest_destroy(dd_view_ingest *g) { delete g; }

extern "C" dd_status dd_view_ingest_kernel_ms(const dd_view_ingest *g, float out_ms[3]) {
    if (!g || !out_ms) return set_err(DD_ERR_INVALID, "null argument");
    HIP_TRY(hipEventSynchronize(g->ev[4]));
    HIP_TRY(hipEventElapsedTime(&out_ms[0], g->ev[0], g->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out_ms[1], g->ev[1], g->ev[2]));
    HIP_TRY(hipEventElapsedTime(&out_ms[2], g->ev[3], g->ev[4]));
    return DD_OK;
}

struct dd_view_emit {
    const dd_partitioner *p = nullptr;
    uint32_t W = 0;
    int64_t n_rows = 0;
    std::vector<int64_t> long_off; /* host prefix sums [W+1] */
    dd_vw_tile *tiles = nullptr;
    uint64_t *tsum = nullptr; /* [n_tiles][2] then the scan [n_tiles+1][2] then meta[3] */
    void *views = nullptr;
    uint8_t *bytes = nullptr;
    hipEvent_t ev[5] = {}; /* scan: 0-1, build: 2-3, copy: 3-4 */
    ~dd_view_emit() {
        (void)hipFree(tiles);
        (void)hipFree(tsum);
        (void)hipFree(views);
        (void)hipFree(bytes);
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

extern "C" dd_status dd_view_emit_run(const dd_partitioner *p, int32_t col,
                                      uint32_t n_windows, void *stream, dd_view_emit **out) {
    if (!p || !out) return set_err(DD_ERR_INVALID, "null argument");
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    if (col < 0 || col >= p->batch.n_cols || p->batch.cols[col].dtype != DD_DT_UTF8)
        return set_err(DD_ERR_INVALID, "view emit needs a utf8 column");
    if (n_windows == 0 || p->nparts % n_windows != 0)
        return set_err(DD_ERR_INVALID, "n_windows must be > 0 and divide P_total");
    int var = -1;
    for (int v = 0; v < p->ka.n_var; v++)
        if (p->ka.var_idx[v] == col) var = v;
    if (var < 0 || !p->out_lengths[col])
        return set_err(DD_ERR_INVALID, "view emit: column has no var-width output");
    hipStream_t s = (hipStream_t)stream;

    std::unique_ptr<dd_view_emit> g(new dd_view_emit());
    g->p = p;
    g->W = n_windows;
    g->n_rows = p->batch.n_rows;
    const uint32_t W = n_windows, ppw = p->nparts / W;

    /* tile table from the host-known row offsets: no tile straddles a partition (hence a
     * window); empty partitions and windows produce none */
    std::vector<int64_t> roff(p->nparts + 1);
    dd_status st = dd_partitioner_row_offsets(p, roff.data());
    if (st != DD_OK) return st;
    std::vector<dd_vw_tile> tiles;
    std::vector<int64_t> win_first(W + 1, 0);
    for (uint32_t w = 0; w < W; w++) {
        win_first[w] = (int64_t)tiles.size();
        for (uint32_t q = w * ppw; q < (w + 1) * ppw; q++) {
            const uint32_t pf = (uint32_t)tiles.size();
            for (int64_t r = roff[q]; r < roff[q + 1]; r += DD_VW_TILE_ROWS)
                tiles.push_back({r, r + DD_VW_TILE_ROWS < roff[q + 1] ? r + DD_VW_TILE_ROWS
                                                                      : roff[q + 1],
                                 q, pf, (uint32_t)win_first[w], 0u});
        }
    }
    const int64_t nt = (int64_t)tiles.size();
    win_first[W] = nt;
    if (nt > INT32_MAX) return set_err(DD_ERR_UNSUPPORTED, "too many view tiles");

    HIP_TRY(hipMalloc((void **)&g->tiles, (size_t)(nt ? nt : 1) * sizeof(dd_vw_tile)));
    HIP_TRY(hipMalloc((void **)&g->tsum, (size_t)(4 * nt + 2 + 3) * 8));
    HIP_TRY(hipMalloc(&g->views, (size_t)g->n_rows * 16 + 16));
    for (auto &e : g->ev) HIP_TRY(hipEventCreate(&e));
    uint64_t *S = g->tsum + 2 * nt, *meta = g->tsum + 4 * nt + 2;
    if (nt)
        HIP_TRY(hipMemcpyAsync(g->tiles, tiles.data(), (size_t)nt * sizeof(dd_vw_tile),
                               hipMemcpyHostToDevice, s));
    const uint32_t *lens = p->out_lengths[col];
    const uint8_t *valid = p->out_valid[col];
    const uint8_t *src = (const uint8_t *)p->out_data[col];
    const uint64_t *pboff = p->part_boffsets + (size_t)var * (p->nparts + 1);

    HIP_TRY(hipEventRecord(g->ev[0], s));
    HIP_TRY(dd_launch_ve_sums(g->tiles, nt, lens, valid, g->tsum, s));
    HIP_TRY(dd_launch_vw_scan(g->tsum, nt, 2, S, meta, nullptr, s));
    HIP_TRY(hipEventRecord(g->ev[1], s));

    /* the one host sync: the long-byte scan, to size the buffer and cut it by window */
    std::vector<uint64_t> S_h((size_t)2 * (nt + 1));
    HIP_TRY(hipMemcpyAsync(S_h.data(), S, S_h.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    g->long_off.assign(W + 1, 0);
    for (uint32_t w = 0; w <= W; w++) g->long_off[w] = (int64_t)S_h[2 * win_first[w] + 1];
    for (uint32_t w = 0; w < W; w++)
        if (g->long_off[w + 1] - g->long_off[w] > (int64_t)INT32_MAX)
            return set_err(DD_ERR_UNSUPPORTED, "view emit: window " + std::to_string(w) +
                                                   " holds more than INT32_MAX long bytes: "
                                                   "use more windows");
    HIP_TRY(hipMalloc((void **)&g->bytes, (size_t)g->long_off[W] + 8));
    HIP_TRY(hipEventRecord(g->ev[2], s));
    HIP_TRY(dd_launch_ve_build(g->tiles, nt, lens, valid, src, pboff, S, g->views, s));
    HIP_TRY(hipEventRecord(g->ev[3], s));
    if (g->long_off[W])
        HIP_TRY(dd_launch_ve_copy(g->tiles, nt, lens, valid, src, pboff, S, g->bytes,
                                  dd_view_lds_enabled(), s));
    HIP_TRY(hipEventRecord(g->ev[4], s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = g.release();
    return DD_OK;
}

extern "C" const void *dd_view_emit_views(const dd_view_emit *g) {
    return g ? g->views : nullptr;
}
extern "C" const uint8_t *dd_view_emit_bytes(const dd_view_emit *g) {
    return g ? g->bytes : nullptr;
}
extern "C" void dd_view_emit_destroy(dd_view_emit *g) { delete g; }

extern "C" dd_status dd_view_emit_counts(const dd_view_emit *g, int64_t *long_byte_off) {
    if (!g || !long_byte_off) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(long_byte_off, g->long_off.data(), g->long_off.size() * 8);
    return DD_OK;
}

extern "C" dd_status dd_view_emit_kernel_ms(const dd_view_emit *g, float out_ms[3]) {
    if (!g || !out_ms) return set_err(DD_ERR_INVALID, "null argument");
    HIP_TRY(hipEventSynchronize(g->ev[4]));
    HIP_TRY(hipEventElapsedTime(&out_ms[0], g->ev[0], g->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out_ms[1], g->ev[2], g->ev[3]));
    HIP_TRY(hipEventElapsedTime(&out_ms[2], g->ev[3], g->ev[4]));
    return DD_OK;
}

/* rebase with host tables: uploads them, runs k_gc_rebase, syncs, frees (every path) */
static dd_status dd_rebase_run(const int32_t *in, int64_t n, const int64_t *host_seg_off,
                               const int32_t *host_bases, int32_t n_seg, int32_t skew,
                               int32_t *out, hipStream_t s) {
    if (n <= 0 || n_seg <= 0) return DD_OK;
    int64_t *d_seg = nullptr;
    int32_t *d_base = nullptr;
    HIP_TRY(hipMalloc((void **)&d_seg, (size_t)(n_seg + 1) * 8));
    hipError_t he = hipMalloc((void **)&d_base, (size_t)n_seg * 4);
    if (he == hipSuccess)
        he = hipMemcpyAsync(d_seg, host_seg_off, (size_t)(n_seg + 1) * 8,
                            hipMemcpyHostToDevice, s);
    if (he == hipSuccess)
        he = hipMemcpyAsync(d_base, host_bases, (size_t)n_seg * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = dd_launch_gc_rebase(in, n, d_seg, d_base, n_seg, skew, out, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    (void)hipFree(d_seg);
    (void)hipFree(d_base);
    if (he != hipSuccess)
        return set_err(DD_ERR_HIP, std::string("dict rebase: ") + hipGetErrorString(he));
    return DD_OK;
}

extern "C" dd_status dd_dict_rebase(const int32_t *in, int64_t n, const int64_t *host_seg_off,
                                    const int32_t *host_bases, int32_t n_seg, int32_t *out,
                                    void *stream) {
    if (!host_seg_off || !host_bases || n < 0 || n_seg <= 0 || (n > 0 && (!in || !out)))
        return set_err(DD_ERR_INVALID, "dd_dict_rebase: null or negative argument");
    if (host_seg_off[0] != 0 || host_seg_off[n_seg] != n)
        return set_err(DD_ERR_INVALID, "dd_dict_rebase: segments must cover [0, n)");
    for (int32_t q = 0; q < n_seg; q++)
        if (host_seg_off[q + 1] < host_seg_off[q])
            return set_err(DD_ERR_INVALID, "dd_dict_rebase: segment offsets must ascend");
    return dd_rebase_run(in, n, host_seg_off, host_bases, n_seg, 0, out, (hipStream_t)stream);
}


struct dd_exchanged {
    int32_t n_cols = 0;
    int nranks = 1;
    uint32_t P = 0;
    int64_t total_rows = 0;
    hipStream_t alloc_stream = nullptr; /* buffers are stream-ordered (hipMallocAsync):
                                           repeated exchanges reuse the pool instead of
                                           paying a device malloc per step */
    std::vector<int64_t> row_counts;                 /* [nranks][P] */
    std::vector<std::vector<int64_t>> byte_counts;   /* per col: [nranks][P] (var only) */
    void *data[DD_MAX_COLS] = {};
    uint8_t *valid[DD_MAX_COLS] = {};
    uint32_t *lengths[DD_MAX_COLS] = {};
    /* GC'd dict32 columns (dd_exchange_run_gc): the received dictionaries, concatenated in
     * producer-rank order; dict_raw is the per-producer offsets arrays as received */
    int64_t dict_n[DD_MAX_COLS];
    int32_t *dict_off[DD_MAX_COLS] = {};
    int32_t *dict_raw[DD_MAX_COLS] = {};
    uint8_t *dict_bytes[DD_MAX_COLS] = {};
    std::vector<std::vector<int64_t>> dict_vals; /* per col: [nranks] values per producer */
    float ms = 0;
    int64_t egress = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    dd_exchanged() {
        for (auto &d : dict_n) d = -1;
    }
    ~dd_exchanged() {
        for (int i = 0; i < DD_MAX_COLS; i++) {
            if (dict_off[i]) (void)hipFreeAsync(dict_off[i], alloc_stream);
            if (dict_raw[i]) (void)hipFreeAsync(dict_raw[i], alloc_stream);
            if (dict_bytes[i]) (void)hipFreeAsync(dict_bytes[i], alloc_stream);
            if (data[i]) (void)hipFreeAsync(data[i], alloc_stream);
            if (valid[i]) (void)hipFreeAsync(valid[i], alloc_stream);
            if (lengths[i]) (void)hipFreeAsync(lengths[i], alloc_stream);
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

/* shared body of dd_exchange_run (n_gcs == 0) and dd_exchange_run_gc */
static dd_status dd_exchange_impl(dd_comm *c, const dd_partitioner *p, dd_dict_gc *const *gcs,
                                  int32_t n_gcs, void *stream, dd_exchanged **out) {
    if (!c || !p || !out || n_gcs < 0 || (n_gcs > 0 && !gcs))
        return set_err(DD_ERR_INVALID, "null argument");
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    if (p->nparts % c->nranks != 0)
        return set_err(DD_ERR_INVALID, "P_total must be nranks * partitions-per-consumer "
                                       "(scale_partitioning, common.rs:18-30)");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t P = p->nparts / c->nranks;
    const int R = c->nranks;
    const int nvar = p->ka.n_var;
    /* gc_of[col]: the GC covering a dict32 column, or null (crosses as plain indices) */
    const dd_dict_gc *gc_of[DD_MAX_COLS] = {};
    for (int32_t gi = 0; gi < n_gcs; gi++) {
        const dd_dict_gc *g = gcs[gi];
        if (!g || g->p != p || g->W != (uint32_t)R || gc_of[g->col])
            return set_err(DD_ERR_INVALID, "each dictionary GC must belong to this "
                                           "partitioner, have n_windows == nranks and "
                                           "cover its column once");
        gc_of[g->col] = g;
    }

    /* 1) size matrix: my per-partition row counts (+ per var col byte counts), allgathered.
     * meta layout per rank: [P_total rows][nvar * P_total bytes] (u64), then per GC'd
     * column, in gcs[] order, [R value counts][R byte counts] of its R windows */
    const size_t meta_gc0 = (size_t)p->nparts * (1 + nvar);
    const size_t meta_n = meta_gc0 + (size_t)n_gcs * 2 * R;
    std::vector<int64_t> my_meta(meta_n);
    for (int32_t gi = 0; gi < n_gcs; gi++)
        for (int j = 0; j < R; j++) {
            my_meta[meta_gc0 + (size_t)gi * 2 * R + j] =
                gcs[gi]->val_off[j + 1] - gcs[gi]->val_off[j];
            my_meta[meta_gc0 + (size_t)gi * 2 * R + R + j] =
                gcs[gi]->byte_off[j + 1] - gcs[gi]->byte_off[j];
        }
    std::vector<int64_t> off_h(p->nparts + 1);
    dd_status st = dd_partitioner_row_offsets(p, off_h.data());
    if (st != DD_OK) return st;
    for (uint32_t q = 0; q < p->nparts; q++) my_meta[q] = off_h[q + 1] - off_h[q];
    std::vector<std::vector<int64_t>> boff_h(nvar, std::vector<int64_t>(p->nparts + 1));
    for (int v = 0; v < nvar; v++) {
        st = dd_partitioner_byte_offsets(p, p->ka.var_idx[v], boff_h[v].data());
        if (st != DD_OK) return st;
        for (uint32_t q = 0; q < p->nparts; q++)
            my_meta[(size_t)(1 + v) * p->nparts + q] = boff_h[v][q + 1] - boff_h[v][q];
    }
    std::vector<int64_t> all_meta((size_t)R * meta_n);
    {
        dd_status ms = dd_meta_allgather(c, my_meta, all_meta, s);
        if (ms != DD_OK) return ms;
    }

    /* a consumer's concatenated dictionary keeps i32 offsets. Checked for EVERY consumer
     * from the allgathered matrix, so all ranks take the same exit before the collective */
    for (int32_t gi = 0; gi < n_gcs; gi++)
        for (int j = 0; j < R; j++) {
            int64_t tb = 0;
            for (int r = 0; r < R; r++)
                tb += all_meta[(size_t)r * meta_n + meta_gc0 + (size_t)gi * 2 * R + R + j];
            if (tb > INT32_MAX)
                return set_err(DD_ERR_UNSUPPORTED, "received dictionary bytes exceed "
                                                   "INT32_MAX (i32 Arrow offsets)");
        }

    std::unique_ptr<dd_exchanged> e_own(new dd_exchanged()); /* freed on error returns */
    dd_exchanged *e = e_own.get();
    e->alloc_stream = dd_pool_stream();
    e->n_cols = p->batch.n_cols;
    e->nranks = R;
    e->P = P;
    e->row_counts.assign((size_t)R * P, 0);
    e->byte_counts.assign(p->batch.n_cols, {});
    /* my window = partitions [P*rank, P*(rank+1)) of every producer */
    for (int r = 0; r < R; r++)
        for (uint32_t q = 0; q < P; q++) {
            e->row_counts[(size_t)r * P + q] =
                all_meta[(size_t)r * meta_n + (size_t)P * c->rank + q];
            e->total_rows += e->row_counts[(size_t)r * P + q];
        }
    std::vector<int64_t> recv_rows_per_producer(R, 0);
    for (int r = 0; r < R; r++)
        for (uint32_t q = 0; q < P; q++)
            recv_rows_per_producer[r] += e->row_counts[(size_t)r * P + q];

    auto fail = [&](dd_status sc, const char *m) { return set_err(sc, m); };

    /* allocate receive buffers */
    std::vector<std::vector<int64_t>> recv_bytes_per_producer(p->batch.n_cols,
                                                              std::vector<int64_t>(R, 0));
    for (int ci = 0; ci < p->batch.n_cols; ci++) {
        const dd_kcol &kc = p->ka.cols[ci];
        if (kc.elem > 0) {
            if (hipMallocAsync(&e->data[ci], (size_t)e->total_rows * kc.elem + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "recv alloc");
        } else {
            /* var col: find its v index, total bytes of my window */
            int v = -1;
            for (int vv = 0; vv < nvar; vv++)
                if (p->ka.var_idx[vv] == ci) v = vv;
            e->byte_counts[ci].assign((size_t)R * P, 0);
            int64_t total_b = 0;
            for (int r = 0; r < R; r++)
                for (uint32_t q = 0; q < P; q++) {
                    int64_t b = all_meta[(size_t)r * meta_n + (size_t)(1 + v) * p->nparts +
                                         (size_t)P * c->rank + q];
                    e->byte_counts[ci][(size_t)r * P + q] = b;
                    recv_bytes_per_producer[ci][r] += b;
                    total_b += b;
                }
            if (hipMallocAsync(&e->data[ci], (size_t)total_b + 1, e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "recv alloc (var)");
            if (hipMallocAsync((void **)&e->lengths[ci], (size_t)e->total_rows * 4 + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "recv alloc (lengths)");
        }
        if (kc.valid) {
            if (hipMallocAsync((void **)&e->valid[ci], (size_t)e->total_rows + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "recv alloc (validity)");
        }
    }
    /* received dictionaries: per GC'd column, values/bytes per producer for MY window */
    e->dict_vals.assign(p->batch.n_cols, {});
    std::vector<std::vector<int64_t>> dict_rb(p->batch.n_cols); /* bytes per producer */
    for (int32_t gi = 0; gi < n_gcs; gi++) {
        const int ci = gcs[gi]->col;
        e->dict_vals[ci].assign(R, 0);
        dict_rb[ci].assign(R, 0);
        int64_t tv = 0, tb = 0;
        for (int r = 0; r < R; r++) {
            const size_t b = (size_t)r * meta_n + meta_gc0 + (size_t)gi * 2 * R;
            tv += e->dict_vals[ci][r] = all_meta[b + c->rank];
            tb += dict_rb[ci][r] = all_meta[b + R + c->rank];
        }
        e->dict_n[ci] = tv;
        if (hipMallocAsync((void **)&e->dict_raw[ci], (size_t)(tv + R) * 4, e->alloc_stream) !=
                hipSuccess ||
            hipMallocAsync((void **)&e->dict_off[ci], (size_t)(tv + 1) * 4, e->alloc_stream) !=
                hipSuccess ||
            hipMallocAsync((void **)&e->dict_bytes[ci], (size_t)tb + 1, e->alloc_stream) !=
                hipSuccess)
            return fail(DD_ERR_HIP, "recv alloc (dictionary)");
    }

    if (hipStreamSynchronize(e->alloc_stream) != hipSuccess) /* allocations ready */
        return fail(DD_ERR_HIP, "pool stream sync");
    if (hipEventCreate(&e->e0) != hipSuccess || hipEventCreate(&e->e1) != hipSuccess)
        return fail(DD_ERR_HIP, "event create");

    /* 2) grouped send/recv: one contiguous slice per (column-stream, peer).
     * send slice for peer j = partitions [P*j, P*(j+1)) of my partition-major output;
     * recv placed producer-major. */
    HIP_TRY(hipEventRecord(e->e0, s));
    NCCL_TRY(ncclGroupStart());
    for (int j = 0; j < R; j++) {
        const int64_t srow0 = off_h[(size_t)P * j], srow1 = off_h[(size_t)P * (j + 1)];
        int64_t rrow0 = 0;
        for (int r = 0; r < j; r++) rrow0 += recv_rows_per_producer[r];
        const int64_t rrows = recv_rows_per_producer[j];
        for (int ci = 0; ci < p->batch.n_cols; ci++) {
            const dd_kcol &kc = p->ka.cols[ci];
            if (kc.elem > 0) {
                int64_t sb = (srow1 - srow0) * kc.elem;
                /* a GC'd column sends its window-local indices, not the partitioner's */
                const uint8_t *src = gc_of[ci] ? (const uint8_t *)gc_of[ci]->indices
                                               : (const uint8_t *)p->out_data[ci];
                if (sb > 0)
                    NCCL_TRY(ncclSend(src + srow0 * kc.elem, sb, ncclUint8, j, c->comm, s));
                int64_t rb = rrows * kc.elem;
                if (rb > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->data[ci] + rrow0 * kc.elem, rb, ncclUint8,
                                      j, c->comm, s));
                if (j != c->rank) e->egress += sb;
            } else {
                int v = -1;
                for (int vv = 0; vv < nvar; vv++)
                    if (p->ka.var_idx[vv] == ci) v = vv;
                int64_t sb0 = boff_h[v][(size_t)P * j], sb1 = boff_h[v][(size_t)P * (j + 1)];
                if (sb1 > sb0)
                    NCCL_TRY(ncclSend((const uint8_t *)p->out_data[ci] + sb0, sb1 - sb0,
                                      ncclUint8, j, c->comm, s));
                int64_t rb0 = 0;
                for (int r = 0; r < j; r++) rb0 += recv_bytes_per_producer[ci][r];
                int64_t rb = recv_bytes_per_producer[ci][j];
                if (rb > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->data[ci] + rb0, rb, ncclUint8, j, c->comm, s));
                if ((srow1 - srow0) > 0)
                    NCCL_TRY(ncclSend(p->out_lengths[ci] + srow0, (srow1 - srow0) * 4,
                                      ncclUint8, j, c->comm, s));
                if (rrows > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->lengths[ci] + rrow0 * 4, rrows * 4,
                                      ncclUint8, j, c->comm, s));
                if (j != c->rank) e->egress += (sb1 - sb0) + (srow1 - srow0) * 4;
            }
            if (kc.valid) {
                if (srow1 > srow0)
                    NCCL_TRY(ncclSend(p->out_valid[ci] + srow0, srow1 - srow0, ncclUint8, j,
                                      c->comm, s));
                if (rrows > 0)
                    NCCL_TRY(ncclRecv(e->valid[ci] + rrow0, rrows, ncclUint8, j, c->comm, s));
                if (j != c->rank) e->egress += srow1 - srow0;
            }
            if (const dd_dict_gc *g = gc_of[ci]) {
                /* window j's dictionary: nvals+1 zero-based offsets and its bytes, each one
                 * contiguous slice; received producer-major */
                const int64_t sv = g->val_off[j + 1] - g->val_off[j];
                const int64_t sbb = g->byte_off[j + 1] - g->byte_off[j];
                NCCL_TRY(ncclSend(g->offs + g->val_off[j] + j, (sv + 1) * 4, ncclUint8, j,
                                  c->comm, s));
                if (sbb > 0)
                    NCCL_TRY(ncclSend(g->bytes + g->byte_off[j], sbb, ncclUint8, j, c->comm, s));
                int64_t rv0 = 0, rb0 = 0;
                for (int r = 0; r < j; r++) {
                    rv0 += e->dict_vals[ci][r];
                    rb0 += dict_rb[ci][r];
                }
                NCCL_TRY(ncclRecv(e->dict_raw[ci] + rv0 + j, (e->dict_vals[ci][j] + 1) * 4,
                                  ncclUint8, j, c->comm, s));
                if (dict_rb[ci][j] > 0)
                    NCCL_TRY(ncclRecv(e->dict_bytes[ci] + rb0, dict_rb[ci][j], ncclUint8, j,
                                      c->comm, s));
                if (j != c->rank) e->egress += (sv + 1) * 4 + sbb;
            }
        }
    }
    NCCL_TRY(ncclGroupEnd());
    HIP_TRY(hipEventRecord(e->e1, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&e->ms, e->e0, e->e1));

    /* after the collective: rebase producer r's indices by the values received from
     * producers < r, and splice the R zero-based offsets arrays into one [dict_n + 1] */
    for (int32_t gi = 0; gi < n_gcs; gi++) {
        const int ci = gcs[gi]->col;
        std::vector<int64_t> seg(R + 1, 0);
        std::vector<int32_t> vbase(R, 0), bbase(R, 0);
        for (int r = 0; r < R; r++) seg[r + 1] = seg[r] + recv_rows_per_producer[r];
        for (int r = 1; r < R; r++) {
            vbase[r] = vbase[r - 1] + (int32_t)e->dict_vals[ci][r - 1];
            bbase[r] = bbase[r - 1] + (int32_t)dict_rb[ci][r - 1];
        }
        st = dd_rebase_run((const int32_t *)e->data[ci], e->total_rows, seg.data(),
                           vbase.data(), R, 0, (int32_t *)e->data[ci], s);
        if (st != DD_OK) return st;
        /* offsets: output segment r = producer r's first nvals entries (its closing entry
         * equals the next producer's rebased 0); the last segment keeps its closing entry */
        for (int r = 0; r < R; r++) seg[r + 1] = seg[r] + e->dict_vals[ci][r];
        seg[R] += 1;
        st = dd_rebase_run(e->dict_raw[ci], e->dict_n[ci] + 1, seg.data(), bbase.data(), R, 1,
                           e->dict_off[ci], s);
        if (st != DD_OK) return st;
        (void)hipFreeAsync(e->dict_raw[ci], e->alloc_stream); /* spliced (rebase synced) */
        e->dict_raw[ci] = nullptr;
    }
    *out = e_own.release();
    return DD_OK;
}

extern "C" dd_status dd_exchange_run(dd_comm *c, const dd_partitioner *p, void *stream,
                                     dd_exchanged **out) {
    return dd_exchange_impl(c, p, nullptr, 0, stream, out);
}

extern "C" dd_status dd_exchange_run_gc(dd_comm *c, const dd_partitioner *p,
                                        dd_dict_gc *const *gcs, int32_t n_gcs, void *stream,
                                        dd_exchanged **out) {
    return dd_exchange_impl(c, p, gcs, n_gcs, stream, out);
}

extern "C" int64_t dd_exchanged_dict_n(const dd_exchanged *e, int32_t c) {
    return (e && c >= 0 && c < e->n_cols) ? e->dict_n[c] : -1;
}
extern "C" const int32_t *dd_exchanged_dict_offsets(const dd_exchanged *e, int32_t c) {
    return (e && c >= 0 && c < e->n_cols) ? e->dict_off[c] : nullptr;
}
extern "C" const void *dd_exchanged_dict_bytes(const dd_exchanged *e, int32_t c) {
    return (e && c >= 0 && c < e->n_cols) ? e->dict_bytes[c] : nullptr;
}
extern "C" dd_status dd_exchanged_dict_counts(const dd_exchanged *e, int32_t c,
                                              int64_t *vals_per_producer) {
    if (!e || !vals_per_producer || c < 0 || c >= e->n_cols || e->dict_n[c] < 0)
        return set_err(DD_ERR_INVALID, "column did not cross with a dictionary GC");
    memcpy(vals_per_producer, e->dict_vals[c].data(), e->dict_vals[c].size() * 8);
    return DD_OK;
}

extern "C" void dd_exchanged_destroy(dd_exchanged *e) { delete e; }
extern "C" int64_t dd_exchanged_total_rows(const dd_exchanged *e) { return e->total_rows; }
extern "C" const void *dd_exchanged_col_data(const dd_exchanged *e, int32_t c) {
    return (c >= 0 && c < e->n_cols) ? e->data[c] : nullptr;
}
extern "C" const uint8_t *dd_exchanged_col_validity(const dd_exchanged *e, int32_t c) {
    return (c >= 0 && c < e->n_cols) ? e->valid[c] : nullptr;
}
extern "C" const uint32_t *dd_exchanged_col_lengths(const dd_exchanged *e, int32_t c) {
    return (c >= 0 && c < e->n_cols) ? e->lengths[c] : nullptr;
}
extern "C" dd_status dd_exchanged_row_counts(const dd_exchanged *e, int64_t *host_out) {
    memcpy(host_out, e->row_counts.data(), e->row_counts.size() * 8);
    return DD_OK;
}
extern "C" dd_status dd_exchanged_byte_counts(const dd_exchanged *e, int32_t col,
                                              int64_t *host_out) {
    if (col < 0 || col >= e->n_cols || e->byte_counts[col].empty())
        return set_err(DD_ERR_INVALID, "not a var column");
    memcpy(host_out, e->byte_counts[col].data(), e->byte_counts[col].size() * 8);
    return DD_OK;
}
extern "C" dd_status dd_exchanged_stats(const dd_exchanged *e, float *ms,
                                        int64_t *egress_bytes) {
    *ms = e->ms;
    *egress_bytes = e->egress;
    return DD_OK;
}

/* ---------------- host plumbing the operators share ---------------- */
/* partial reduce, final merge, both joins and the sort: what they check and set up alike.
 * Every check here runs before any device work and opens its message with the caller's
 * prefix. */

/* kernel arguments over a batch as it is: fixed-width keys, no dictionary hashes */
static void dd_fill_kargs(const dd_batch_desc *b, const int32_t *keys, int32_t n_keys,
                          dd_kargs *ka) {
    memset(ka, 0, sizeof(*ka));
    ka->n_rows = b->n_rows;
    ka->n_cols = b->n_cols;
    ka->n_keys = n_keys;
    for (int k = 0; k < n_keys; k++) ka->key_idx[k] = keys[k];
    for (int c = 0; c < b->n_cols; c++) {
        const dd_col_desc &cd = b->cols[c];
        dd_kcol &kc = ka->cols[c];
        kc.dtype = cd.dtype;
        kc.elem = fixed_elem_size(cd.dtype);
        kc.data = cd.data;
        kc.valid = cd.validity;
        kc.offsets = cd.offsets;
    }
}

/* frees every device pointer handed to it when it goes out of scope */
struct dd_dev_scratch {
    std::vector<void *> ptrs;
    template <typename T> bool alloc(T **p, size_t bytes) {
        void *v = nullptr;
        if (hipMalloc(&v, bytes ? bytes : 1) != hipSuccess) return false;
        ptrs.push_back(v);
        *p = (T *)v;
        return true;
    }
    /* alloc, then enqueue the copy of the host array src[n]. src is pageable: the caller
     * synchronises the stream once, after its last upload and before src dies */
    template <typename T> hipError_t upload(T **p, const T *src, size_t n, hipStream_t s) {
        if (!alloc(p, n * sizeof(T))) return hipErrorOutOfMemory;
        return hipMemcpyAsync(*p, src, n * sizeof(T), hipMemcpyHostToDevice, s);
    }
    ~dd_dev_scratch() {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

/* N events, created by init() and destroyed on every exit path */
template <int N> struct dd_events {
    hipEvent_t ev[N] = {};
    hipError_t init() {
        for (auto &e : ev)
            if (hipError_t r = hipEventCreate(&e)) return r;
        return hipSuccess;
    }
    hipError_t record(int i, hipStream_t s) { return hipEventRecord(ev[i], s); }
    void elapsed(float *ms, int from, int to) const {
        (void)hipEventElapsedTime(ms, ev[from], ev[to]);
    }
    ~dd_events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

/* the layout checks of DESIGN.md §18.1; rows_p: rows per partition */
static dd_status dd_check_layout(const std::string &who, int64_t n, const int64_t *seg_offsets,
                                 const int32_t *seg_part, int32_t n_segs, int32_t n_parts,
                                 std::vector<int64_t> *rows_p) {
    if (n_segs < 1 || n_parts < 1)
        return set_err(DD_ERR_INVALID, who + "at least one segment and one partition");
    if (seg_offsets[0] != 0 || seg_offsets[n_segs] != n)
        return set_err(DD_ERR_INVALID, who + "seg_offsets must run from 0 to n_rows");
    rows_p->assign((size_t)n_parts, 0);
    for (int s = 0; s < n_segs; s++) {
        if (seg_offsets[s + 1] < seg_offsets[s])
            return set_err(DD_ERR_INVALID, who + "seg_offsets decrease");
        if (seg_part[s] < 0 || seg_part[s] >= n_parts)
            return set_err(DD_ERR_INVALID, who + "seg_part outside [0, n_parts)");
        (*rows_p)[seg_part[s]] += seg_offsets[s + 1] - seg_offsets[s];
    }
    return DD_OK;
}

/* One claim / build table region per partition. A partition of `rows` rows gets
 * max(64, next_pow2(2 * rows)) slots (finalagg.table_slots is the same arithmetic). */
struct dd_table_regions {
    std::vector<uint32_t> base, log2;
    uint64_t n_slots = 0;
    /* false: the table would pass 2^32 slots, which the caller refuses in its own words */
    bool size(const std::vector<int64_t> &rows_p) {
        base.assign(rows_p.size(), 0);
        log2.assign(rows_p.size(), 0);
        n_slots = 0;
        for (size_t p = 0; p < rows_p.size() && n_slots < ((uint64_t)1 << 32); p++) {
            uint32_t lg = 6;
            static_assert((1 << 6) == DD_F_MIN_SLOTS, "smallest region");
            while (((int64_t)1 << lg) < 2 * rows_p[p]) lg++;
            log2[p] = lg;
            base[p] = (uint32_t)n_slots;
            n_slots += (uint64_t)1 << lg;
        }
        return n_slots < ((uint64_t)1 << 32);
    }
};

/* a list of columns to gather: indices in range, fixed-width dtypes only */
static dd_status dd_check_projection(const std::string &who, const dd_batch_desc *b,
                                     const int32_t *proj, int32_t n_proj) {
    if (n_proj < 0 || n_proj > DD_MAX_COLS || (n_proj > 0 && !proj))
        return set_err(DD_ERR_INVALID, who + "projection list out of range");
    for (int i = 0; i < n_proj; i++) {
        if (proj[i] < 0 || proj[i] >= b->n_cols)
            return set_err(DD_ERR_INVALID, who + "projected column index out of range");
        const dd_col_desc &cd = b->cols[proj[i]];
        if (cd.dtype == DD_DT_UTF8)
            return set_err(DD_ERR_UNSUPPORTED,
                           who + "projection: a var-width (utf8 / utf8view) column is not "
                                 "supported");
        if (cd.dtype == DD_DT_DICT32)
            return set_err(DD_ERR_UNSUPPORTED,
                           who + "projection: a dict32 column is not supported");
        if (fixed_elem_size(cd.dtype) == 0)
            return set_err(DD_ERR_INVALID, who + "projection: unknown dtype");
        if (cd.dtype == DD_DT_DEC128 && (uintptr_t)cd.data % 16)
            return set_err(DD_ERR_INVALID, who + "dec128 column data must be 16-byte aligned");
    }
    return DD_OK;
}

/* the typed output columns of a run, owned: dd_joiner, dd_sorter and dd_finalizer embed it */
struct dd_out_cols {
    std::vector<void *> data;        /* per column; null only at zero rows */
    std::vector<uint8_t *> validity; /* null: the column has none */
    /* a column of n_out rows gathered from cd, added here and to g. always_valid: it
     * carries validity even where its source has none (a NULL-extended outer-join side) */
    hipError_t add(const dd_col_desc &cd, int64_t n_out, bool always_valid, dd_join_gather *g) {
        const int c = g->n_cols++;
        g->elem[c] = fixed_elem_size(cd.dtype);
        g->src[c] = cd.data;
        g->src_valid[c] = (const uint8_t *)cd.validity;
        data.push_back(nullptr);
        validity.push_back(nullptr);
        hipError_t e = hipMalloc(&data.back(), n_out ? (size_t)n_out * g->elem[c] : 1);
        if (e == hipSuccess && (cd.validity || always_valid))
            e = hipMalloc((void **)&validity.back(), n_out ? (size_t)n_out : 1);
        g->dst[c] = data.back();
        g->dst_valid[c] = validity.back();
        return e;
    }
    const void *data_at(int32_t i) const {
        return i >= 0 && (size_t)i < data.size() ? data[(size_t)i] : nullptr;
    }
    const uint8_t *validity_at(int32_t i) const {
        return i >= 0 && (size_t)i < validity.size() ? validity[(size_t)i] : nullptr;
    }
    void clear() {
        for (void *p : data) (void)hipFree(p);
        for (uint8_t *p : validity) (void)hipFree(p);
        data.clear();
        validity.clear();
    }
    ~dd_out_cols() { clear(); }
};

/* ---------------- partial aggregation (dd_reducer) ---------------- */

struct dd_reducer {
    int32_t n_keys = 0, n_aggs = 0;
    uint64_t *dict_hashes[DD_KMAX_KEYS] = {}; /* per dict32 KEY col (hash input) */
    int64_t n_rows = 0; /* output rows */
    uint64_t *keys = nullptr;
    uint32_t *keynull = nullptr;
    double *aggs = nullptr;
    uint64_t *nn = nullptr; /* [max_rows][n_aggs] non-null input counts */
    uint64_t *hi = nullptr; /* wide kernel: [max_rows][n_aggs] high halves of decimal sums */
    uint64_t *n_dev = nullptr;
    int32_t *meta = nullptr; /* device: agg_cols + agg_ops */
    float kernel_ms = 0;     /* hipEvent time of the reduce kernel alone */
    int32_t kernel = 0;      /* 0 = k_partial_reduce, 1 = k_partial_reduce_wide */
    int32_t waveagg = 0;     /* the wide kernel's wave-aggregation setting (0 for kernel 0) */
    ~dd_reducer() {
        for (auto &d : dict_hashes) (void)hipFree(d);
        (void)hipFree(keys);
        (void)hipFree(keynull);
        (void)hipFree(aggs);
        (void)hipFree(nn);
        (void)hipFree(hi);
        (void)hipFree(n_dev);
        (void)hipFree(meta);
    }
};

/* launch geometry of k_partial_reduce: the one place this arithmetic lives (used by the
 * run below and reported by dd_partial_reduce_geometry) */
static void dd_reduce_geometry(int64_t n, int64_t *nblocks, int64_t *chunk) {
    int64_t nb = (n + DD_R_BLOCK_ROWS - 1) / DD_R_BLOCK_ROWS;
    if (nb < DD_R_MIN_BLOCKS) nb = DD_R_MIN_BLOCKS;
    if (nb > DD_R_MAX_BLOCKS) nb = DD_R_MAX_BLOCKS;
    *nblocks = nb;
    *chunk = (n + nb - 1) / nb;
}

extern "C" dd_status dd_partial_reduce_geometry(int64_t n_rows, int32_t *table_slots,
                                                int32_t *probe_limit, int64_t *nblocks,
                                                int64_t *chunk_rows) {
    if (n_rows < 0 || !table_slots || !probe_limit || !nblocks || !chunk_rows)
        return set_err(DD_ERR_INVALID, "null argument or negative row count");
    *table_slots = DD_R_CAP;
    *probe_limit = DD_R_PROBE;
    dd_reduce_geometry(n_rows, nblocks, chunk_rows);
    return DD_OK;
}

/* The plan of one partial reduce: which kernel runs it and with what geometry. The one
 * place the wide kernel's arithmetic lives (used by the run below and reported by
 * dd_partial_reduce_plan_geometry). */
struct dd_reduce_plan {
    int32_t kernel, table_slots, probe_limit, block_threads, lds_bytes;
    int64_t nblocks, chunk;
};

static dd_status dd_reduce_make_plan(int64_t n, int32_t n_keys, const int32_t *agg_ops,
                                     int32_t n_aggs, dd_reduce_plan *p) {
    if (n_keys < 1 || n_keys > 4) return set_err(DD_ERR_UNSUPPORTED, "1..4 key columns");
    if (n_aggs < 1)
        return set_err(DD_ERR_UNSUPPORTED, "partial reduce: at least 1 aggregate");
    if (n_aggs > DD_RW_MAX_AGGS)
        return set_err(DD_ERR_UNSUPPORTED, "partial reduce: at most 8 aggregates");
    int n_dec = 0;
    for (int g = 0; g < n_aggs; g++) {
        if (agg_ops[g] < 0 || agg_ops[g] > DD_AGG_SUM_DEC128)
            return set_err(DD_ERR_INVALID, "unknown aggregate op");
        if (agg_ops[g] == DD_AGG_SUM_DEC128) n_dec++;
    }
    if (n_aggs <= DD_R_NARROW_AGGS && n_dec == 0) {
        p->kernel = 0;
        p->table_slots = DD_R_CAP;
        p->probe_limit = DD_R_PROBE;
        p->block_threads = 256;
        /* k_partial_reduce's static tables: hash 8, ready 4, null 4, 4 keys, 4 states, 4 nn */
        p->lds_bytes = DD_R_CAP * (8 + 4 + 4 + 4 * 8 + 4 * 8 + 4 * 4);
        dd_reduce_geometry(n, &p->nblocks, &p->chunk);
        return DD_OK;
    }
    /* per slot: hash 8, ready 4, null mask 4, 8 per key, per aggregate 8 state + 4 nn, and
     * 8 more per decimal sum (its high half) */
    const int32_t per_slot = 8 + 4 + 4 + 8 * n_keys + 12 * n_aggs + 8 * n_dec;
    int32_t slots = DD_RW_MAX_SLOTS;
    while (slots > DD_RW_MIN_SLOTS && (int64_t)slots * per_slot > DD_RW_LDS_LIMIT) slots >>= 1;
    p->kernel = 1;
    p->table_slots = slots;
    p->probe_limit = DD_RW_PROBE;
    p->block_threads = DD_RW_THREADS;
    p->lds_bytes = slots * per_slot;
    int64_t nb = (n + DD_RW_BLOCK_ROWS - 1) / DD_RW_BLOCK_ROWS;
    if (nb < DD_RW_MIN_BLOCKS) nb = DD_RW_MIN_BLOCKS;
    if (nb > DD_RW_MAX_BLOCKS) nb = DD_RW_MAX_BLOCKS;
    p->nblocks = nb;
    p->chunk = (n + nb - 1) / nb;
    return DD_OK;
}

extern "C" dd_status dd_partial_reduce_plan_geometry(
    int64_t n_rows, int32_t n_keys, const int32_t *agg_ops, int32_t n_aggs, int32_t *kernel,
    int32_t *table_slots, int32_t *probe_limit, int32_t *block_threads, int32_t *lds_bytes,
    int64_t *nblocks, int64_t *chunk_rows) {
    if (n_rows < 0 || !agg_ops || !kernel || !table_slots || !probe_limit || !block_threads ||
        !lds_bytes || !nblocks || !chunk_rows)
        return set_err(DD_ERR_INVALID, "null argument or negative row count");
    dd_reduce_plan p;
    dd_status st = dd_reduce_make_plan(n_rows, n_keys, agg_ops, n_aggs, &p);
    if (st != DD_OK) return st;
    *kernel = p.kernel;
    *table_slots = p.table_slots;
    *probe_limit = p.probe_limit;
    *block_threads = p.block_threads;
    *lds_bytes = p.lds_bytes;
    *nblocks = p.nblocks;
    *chunk_rows = p.chunk;
    return DD_OK;
}

/* DD_REDUCE_WAVEAGG=0/1, read per call; unset: the measured default */
#define DD_RW_WAVEAGG_DEFAULT 0
static int dd_reduce_waveagg_setting() {
    if (const char *e = getenv("DD_REDUCE_WAVEAGG")) return atoi(e) == 1;
    return DD_RW_WAVEAGG_DEFAULT;
}

extern "C" dd_status dd_partial_reduce_run(const dd_batch_desc *batch,
                                           const int32_t *key_cols, int32_t n_keys,
                                           const int32_t *agg_cols, const int32_t *agg_ops,
                                           int32_t n_aggs, void *stream, dd_reducer **out) {
    if (!batch || !key_cols || !agg_ops || !out)
        return set_err(DD_ERR_INVALID, "null argument");
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");
    if (n_keys < 1 || n_keys > 4) return set_err(DD_ERR_UNSUPPORTED, "1..4 key columns");
    if (n_aggs < 1)
        return set_err(DD_ERR_UNSUPPORTED, "partial reduce: at least 1 aggregate");
    if (n_aggs > DD_RW_MAX_AGGS)
        return set_err(DD_ERR_UNSUPPORTED, "partial reduce: at most 8 aggregates");
    for (int k = 0; k < n_keys; k++) {
        if (key_cols[k] < 0 || key_cols[k] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "key column out of range");
        if (batch->cols[key_cols[k]].dtype == DD_DT_UTF8)
            return set_err(DD_ERR_UNSUPPORTED,
                           "partial reduce: fixed-width or dictionary keys only");
        if (batch->cols[key_cols[k]].dtype == DD_DT_DEC128)
            return set_err(DD_ERR_UNSUPPORTED, "partial reduce: dec128 keys are not supported");
    }
    for (int g = 0; g < n_aggs; g++) {
        if (agg_ops[g] == DD_AGG_COUNT) continue;
        if (!agg_cols || agg_cols[g] < 0 || agg_cols[g] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "agg column out of range");
        int dt = batch->cols[agg_cols[g]].dtype;
        if (agg_ops[g] == DD_AGG_SUM_DEC128) {
            if (dt != DD_DT_DEC128)
                return set_err(DD_ERR_UNSUPPORTED,
                               "partial reduce: sum_dec128 needs a dec128 column");
            continue;
        }
        if (dt == DD_DT_DEC128)
            return set_err(DD_ERR_UNSUPPORTED,
                           "partial reduce: a dec128 column takes sum_dec128 only");
        if ((agg_ops[g] == DD_AGG_SUM_F64 || agg_ops[g] == DD_AGG_MIN_F64 ||
             agg_ops[g] == DD_AGG_MAX_F64) &&
            dt != DD_DT_F64)
            return set_err(DD_ERR_UNSUPPORTED, "f64 aggregate needs an f64 column");
        if ((agg_ops[g] == DD_AGG_SUM_I64 || agg_ops[g] == DD_AGG_MIN_I64 ||
             agg_ops[g] == DD_AGG_MAX_I64) &&
            dt != DD_DT_I64)
            return set_err(DD_ERR_UNSUPPORTED, "i64 aggregate needs an i64 column");
        if (agg_ops[g] < 0 || agg_ops[g] > DD_AGG_MAX_I64)
            return set_err(DD_ERR_INVALID, "unknown aggregate op");
    }
    const int64_t n = batch->n_rows;
    dd_reduce_plan plan;
    if (dd_status st = dd_reduce_make_plan(n, n_keys, agg_ops, n_aggs, &plan)) return st;
    const bool wide = plan.kernel == 1;

    dd_kargs ka;
    dd_fill_kargs(batch, key_cols, n_keys, &ka);

    const int64_t nblocks = plan.nblocks, chunk = plan.chunk;
    /* spill worst case + table flush */
    const int64_t max_rows = n + nblocks * plan.table_slots + 1;

    auto r = new dd_reducer();
    r->n_keys = n_keys;
    r->n_aggs = n_aggs;
    r->kernel = plan.kernel;
    r->waveagg = wide ? dd_reduce_waveagg_setting() : 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto fail = [&](const char *m) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        delete r;
        return set_err(DD_ERR_HIP, m);
    };

    /* dict32 key columns: the row hash reads precomputed per-value hashes */
    for (int k = 0; k < n_keys; k++) {
        const dd_col_desc &cd = batch->cols[key_cols[k]];
        if (cd.dtype != DD_DT_DICT32) continue;
        if (hipMalloc((void **)&r->dict_hashes[k], (size_t)cd.dict_n * 8 + 8) != hipSuccess)
            return fail("dict hash alloc");
        if (dd_launch_dict_hashes((const uint8_t *)cd.dict_bytes, cd.dict_offsets,
                                  cd.dict_n, r->dict_hashes[k],
                                  (hipStream_t)stream) != hipSuccess)
            return fail("dict hash launch");
        ka.cols[key_cols[k]].dict_hashes = r->dict_hashes[k];
    }
    if (hipMalloc((void **)&r->keys, (size_t)max_rows * n_keys * 8) != hipSuccess ||
        hipMalloc((void **)&r->keynull, (size_t)max_rows * 4) != hipSuccess ||
        hipMalloc((void **)&r->aggs, (size_t)max_rows * n_aggs * 8) != hipSuccess ||
        hipMalloc((void **)&r->nn, (size_t)max_rows * n_aggs * 8) != hipSuccess ||
        hipMalloc((void **)&r->n_dev, 8) != hipSuccess ||
        hipMalloc((void **)&r->meta, 2 * DD_RW_MAX_AGGS * 4) != hipSuccess)
        return fail("partial reduce alloc");
    if (wide && hipMalloc((void **)&r->hi, (size_t)max_rows * n_aggs * 8) != hipSuccess)
        return fail("partial reduce alloc");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(r->n_dev, 0, 8, s) != hipSuccess) return fail("memset");
    /* agg_cols then agg_ops, each padded to the running kernel's aggregate cap */
    const int cap = wide ? DD_RW_MAX_AGGS : DD_R_NARROW_AGGS;
    int32_t meta_h[2 * DD_RW_MAX_AGGS] = {};
    for (int g = 0; g < n_aggs; g++) {
        meta_h[g] = agg_cols ? agg_cols[g] : 0;
        meta_h[cap + g] = agg_ops[g];
    }
    if (hipMemcpyAsync(r->meta, meta_h, (size_t)2 * cap * 4, hipMemcpyHostToDevice, s) !=
        hipSuccess)
        return fail("meta upload");
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    hipError_t e;
    if (wide)
        e = dd_launch_partial_reduce_wide(&ka, r->waveagg, nblocks, chunk, n_aggs,
                                          plan.table_slots, plan.probe_limit,
                                          (size_t)plan.lds_bytes, r->meta, r->meta + cap,
                                          r->keys, r->keynull, (uint64_t *)r->aggs, r->hi,
                                          r->nn, r->n_dev, s);
    else
        e = dd_launch_partial_reduce(&ka, nblocks, chunk, n_aggs, r->meta, r->meta + cap,
                                     r->keys, r->keynull, r->aggs, r->nn, r->n_dev, s);
    (void)hipEventRecord(e1, s);
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipStreamSynchronize(s) != hipSuccess) return fail("sync");
    (void)hipEventElapsedTime(&r->kernel_ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    e0 = e1 = nullptr; /* fail() must not double-destroy */
    uint64_t n_out = 0;
    if (hipMemcpy(&n_out, r->n_dev, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("n_out copy");
    r->n_rows = (int64_t)n_out;
    *out = r;
    return DD_OK;
}

extern "C" int64_t dd_reducer_n_rows(const dd_reducer *r) { return r->n_rows; }
extern "C" float dd_reducer_kernel_ms(const dd_reducer *r) { return r->kernel_ms; }

extern "C" dd_status dd_reducer_fetch(const dd_reducer *r, uint64_t *host_keys,
                                      uint32_t *host_keynull, double *host_aggs) {
    HIP_TRY(hipMemcpy(host_keys, r->keys, (size_t)r->n_rows * r->n_keys * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_keynull, r->keynull, (size_t)r->n_rows * 4,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_aggs, r->aggs, (size_t)r->n_rows * r->n_aggs * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

/* non-null input counts per output row per aggregate ([n_rows][n_aggs]): the final
 * merge sums these; total 0 => the merged aggregate is NULL (DataFusion semantics for
 * SUM/MIN/MAX over an all-null group) */
extern "C" dd_status dd_reducer_fetch_nn(const dd_reducer *r, uint64_t *host_nn) {
    HIP_TRY(hipMemcpy(host_nn, r->nn, (size_t)r->n_rows * r->n_aggs * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

/* host_hi[n_rows][n_aggs]: the high 64 bits of each decimal sum, 0 for every other op */
extern "C" dd_status dd_reducer_fetch_hi(const dd_reducer *r, uint64_t *host_hi) {
    const size_t bytes = (size_t)r->n_rows * r->n_aggs * 8;
    if (!r->hi) { /* k_partial_reduce ran: no decimal sum in the plan */
        memset(host_hi, 0, bytes);
        return DD_OK;
    }
    HIP_TRY(hipMemcpy(host_hi, r->hi, bytes, hipMemcpyDeviceToHost));
    return DD_OK;
}

extern "C" int32_t dd_reducer_kernel(const dd_reducer *r) { return r->kernel; }
extern "C" int32_t dd_reducer_waveagg(const dd_reducer *r) { return r->waveagg; }

extern "C" void dd_reducer_destroy(dd_reducer *r) { delete r; }

/* ---------------- final aggregation above the shuffle (dd_finalizer) ------ */

struct dd_finalizer {
    int32_t n_keys = 0, n_aggs = 0, n_parts = 0;
    int64_t n_groups = 0;
    std::vector<int64_t> group_offsets; /* [n_parts + 1] */
    uint64_t *keys = nullptr;           /* [n_groups][n_keys] */
    uint32_t *keynull = nullptr;        /* [n_groups] */
    uint64_t *aggs = nullptr;           /* [n_groups][n_aggs] */
    uint64_t *hi = nullptr;
    uint64_t *nn = nullptr;
    float kernel_ms[3] = {0, 0, 0}; /* claim, scan, merge */
    /* dd_finalizer_columns: keys, aggregates, then the optional nn columns */
    std::vector<int32_t> col_dtype;
    dd_out_cols cols;
    ~dd_finalizer() {
        (void)hipFree(keys);
        (void)hipFree(keynull);
        (void)hipFree(aggs);
        (void)hipFree(hi);
        (void)hipFree(nn);
    }
};

extern "C" dd_status dd_final_merge_run(const dd_batch_desc *batch, const int32_t *key_cols,
                                        int32_t n_keys, const int32_t *state_cols,
                                        const int32_t *agg_ops, const int32_t *nn_cols,
                                        int32_t n_aggs, const int64_t *seg_offsets,
                                        const int32_t *seg_part, int32_t n_segs,
                                        int32_t n_parts, void *stream, dd_finalizer **out) {
    if (!batch || !key_cols || !state_cols || !agg_ops || !nn_cols || !seg_offsets ||
        !seg_part || !out)
        return set_err(DD_ERR_INVALID, "final merge: null argument");
    if (n_keys < 1 || n_keys > 4)
        return set_err(DD_ERR_UNSUPPORTED, "final merge: 1..4 key columns");
    if (n_aggs < 1)
        return set_err(DD_ERR_UNSUPPORTED, "final merge: at least 1 aggregate");
    if (n_aggs > DD_F_MAX_AGGS)
        return set_err(DD_ERR_UNSUPPORTED, "final merge: at most 8 aggregates");
    const int64_t n = batch->n_rows;
    if (n < 0 || n >= ((int64_t)1 << 31))
        return set_err(DD_ERR_INVALID, "final merge: n_rows must be below 2^31 (row ids are "
                                       "32-bit table entries)");
    if (batch->n_cols < 1 || batch->n_cols > DD_MAX_COLS)
        return set_err(DD_ERR_INVALID, "final merge: column count out of range");
    for (int k = 0; k < n_keys; k++) {
        if (key_cols[k] < 0 || key_cols[k] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "final merge: key column out of range");
        switch (batch->cols[key_cols[k]].dtype) {
        case DD_DT_DICT32:
            return set_err(DD_ERR_UNSUPPORTED,
                           "final merge: dict32 keys are not supported: rebased indices "
                           "after a GC'd exchange must be merged by value");
        case DD_DT_UTF8:
            return set_err(DD_ERR_UNSUPPORTED,
                           "final merge: utf8 / utf8view keys are not supported");
        case DD_DT_DEC128:
            return set_err(DD_ERR_UNSUPPORTED, "final merge: dec128 keys are not supported");
        case DD_DT_U8: case DD_DT_BOOL: case DD_DT_I16: case DD_DT_I32: case DD_DT_I64:
        case DD_DT_F32: case DD_DT_F64:
            break;
        default:
            return set_err(DD_ERR_INVALID, "final merge: unknown key dtype");
        }
    }
    dd_final_plan plan;
    memset(&plan, 0, sizeof(plan));
    plan.n_aggs = n_aggs;
    for (int g = 0; g < n_aggs; g++) {
        const int op = agg_ops[g];
        if (op < 0 || op > DD_AGG_SUM_DEC128)
            return set_err(DD_ERR_INVALID, "final merge: unknown aggregate op");
        if (state_cols[g] < 0 || state_cols[g] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "final merge: state column out of range");
        const dd_col_desc &sc = batch->cols[state_cols[g]];
        if (op == DD_AGG_SUM_DEC128) {
            if (sc.dtype != DD_DT_DEC128)
                return set_err(DD_ERR_UNSUPPORTED,
                               "final merge: a sum_dec128 state must be a dec128 column");
            if ((uintptr_t)sc.data % 16)
                return set_err(DD_ERR_INVALID, "final merge: dec128 data must be 16-byte "
                                               "aligned");
        } else if (op == DD_AGG_SUM_F64 || op == DD_AGG_MIN_F64 || op == DD_AGG_MAX_F64) {
            if (sc.dtype != DD_DT_F64)
                return set_err(DD_ERR_UNSUPPORTED,
                               "final merge: an f64 aggregate's state must be an f64 column");
        } else if (sc.dtype != DD_DT_I64) {
            return set_err(DD_ERR_UNSUPPORTED,
                           "final merge: a count / i64 aggregate's state must be an i64 "
                           "column");
        }
        plan.ops[g] = op;
        plan.state_cols[g] = state_cols[g];
        if (op == DD_AGG_COUNT) continue; /* nn is the merged count; nn_col is -1 */
        if (nn_cols[g] < 0 || nn_cols[g] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "final merge: nn column out of range");
        if (batch->cols[nn_cols[g]].dtype != DD_DT_I64)
            return set_err(DD_ERR_UNSUPPORTED, "final merge: an nn column must be i64");
        plan.nn_cols[g] = nn_cols[g];
    }
    /* segment layout -> rows per partition -> table regions */
    std::vector<int64_t> rows_p;
    if (dd_status st = dd_check_layout("final merge: malformed segment layout: ", n,
                                       seg_offsets, seg_part, n_segs, n_parts, &rows_p))
        return st;
    dd_table_regions reg;
    if (!reg.size(rows_p))
        return set_err(DD_ERR_UNSUPPORTED, "final merge: claim table past 2^32 slots");
    const uint64_t n_slots = reg.n_slots;

    auto f = std::unique_ptr<dd_finalizer>(new dd_finalizer());
    f->n_keys = n_keys;
    f->n_aggs = n_aggs;
    f->n_parts = n_parts;
    f->group_offsets.assign((size_t)n_parts + 1, 0);
    if (n == 0) { /* zero groups, no device work */
        *out = f.release();
        return DD_OK;
    }
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");

    dd_kargs ka;
    dd_fill_kargs(batch, key_cols, n_keys, &ka);

    hipStream_t s = (hipStream_t)stream;
    dd_dev_scratch ws;
    int64_t *d_seg_off = nullptr, *d_goff = nullptr;
    int32_t *d_seg_part = nullptr;
    uint32_t *d_base = nullptr, *d_log2 = nullptr, *table = nullptr, *slot_gid = nullptr,
             *row_slot = nullptr, *block_sums = nullptr, *err = nullptr;
    const size_t nb = (size_t)((n_slots + DD_F_SCAN_TILE - 1) / DD_F_SCAN_TILE);
    if (!ws.alloc(&d_goff, ((size_t)n_parts + 1) * 8) ||
        !ws.alloc(&table, (size_t)n_slots * 4) || !ws.alloc(&slot_gid, (size_t)n_slots * 4) ||
        !ws.alloc(&row_slot, (size_t)n * 4) || !ws.alloc(&block_sums, (nb + 1) * 4) ||
        !ws.alloc(&err, 4))
        return set_err(DD_ERR_HIP, "final merge: workspace alloc");
    dd_events<5> ev;
    HIP_TRY(ev.init());
    HIP_TRY(ws.upload(&d_seg_off, seg_offsets, (size_t)n_segs + 1, s));
    HIP_TRY(ws.upload(&d_seg_part, seg_part, (size_t)n_segs, s));
    HIP_TRY(ws.upload(&d_base, reg.base.data(), (size_t)n_parts, s));
    HIP_TRY(ws.upload(&d_log2, reg.log2.data(), (size_t)n_parts, s));
    HIP_TRY(hipMemsetAsync(err, 0, 4, s));
    HIP_TRY(hipStreamSynchronize(s)); /* the uploads have left their pageable sources */

    HIP_TRY(ev.record(0, s));
    HIP_TRY(hipMemsetAsync(table, 0xff, (size_t)n_slots * 4, s)); /* DD_F_EMPTY */
    HIP_TRY(dd_launch_final_claim(&ka, d_seg_off, d_seg_part, n_segs, d_base, d_log2, table,
                                  row_slot, err, s));
    HIP_TRY(ev.record(1, s));
    HIP_TRY(dd_launch_final_scan(table, n_slots, block_sums, slot_gid, d_base, n_parts, d_goff,
                                 s));
    HIP_TRY(ev.record(2, s));
    HIP_TRY(hipMemcpyAsync(f->group_offsets.data(), d_goff, ((size_t)n_parts + 1) * 8,
                           hipMemcpyDeviceToHost, s));
    uint32_t err_h = 0;
    HIP_TRY(hipMemcpyAsync(&err_h, err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err_h) return set_err(DD_ERR_HIP, "final merge: claim table overflow (internal)");
    const int64_t ng = f->group_offsets[n_parts];
    f->n_groups = ng;
    /* state is sized by the groups found, not by the table */
    HIP_TRY(hipMalloc((void **)&f->keys, (size_t)ng * n_keys * 8));
    HIP_TRY(hipMalloc((void **)&f->keynull, (size_t)ng * 4));
    HIP_TRY(hipMalloc((void **)&f->aggs, (size_t)ng * n_aggs * 8));
    HIP_TRY(hipMalloc((void **)&f->hi, (size_t)ng * n_aggs * 8));
    HIP_TRY(hipMalloc((void **)&f->nn, (size_t)ng * n_aggs * 8));
    HIP_TRY(ev.record(3, s));
    HIP_TRY(dd_launch_final_merge(&ka, &plan, table, row_slot, slot_gid, ng, f->keys,
                                  f->keynull, f->aggs, f->hi, f->nn, s));
    HIP_TRY(ev.record(4, s));
    HIP_TRY(hipStreamSynchronize(s));
    ev.elapsed(&f->kernel_ms[0], 0, 1);
    ev.elapsed(&f->kernel_ms[1], 1, 2);
    ev.elapsed(&f->kernel_ms[2], 3, 4);
    *out = f.release();
    return DD_OK;
}

extern "C" int64_t dd_finalizer_n_groups(const dd_finalizer *f) { return f->n_groups; }

extern "C" dd_status dd_finalizer_group_offsets(const dd_finalizer *f, int64_t *host_out) {
    if (!f || !host_out) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(host_out, f->group_offsets.data(), f->group_offsets.size() * 8);
    return DD_OK;
}

extern "C" dd_status dd_finalizer_fetch(const dd_finalizer *f, uint64_t *host_keys,
                                        uint32_t *host_keynull, double *host_aggs) {
    if (f->n_groups == 0) return DD_OK;
    HIP_TRY(hipMemcpy(host_keys, f->keys, (size_t)f->n_groups * f->n_keys * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_keynull, f->keynull, (size_t)f->n_groups * 4,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host_aggs, f->aggs, (size_t)f->n_groups * f->n_aggs * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

extern "C" dd_status dd_finalizer_fetch_nn(const dd_finalizer *f, uint64_t *host_nn) {
    if (f->n_groups == 0) return DD_OK;
    HIP_TRY(hipMemcpy(host_nn, f->nn, (size_t)f->n_groups * f->n_aggs * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

extern "C" dd_status dd_finalizer_fetch_hi(const dd_finalizer *f, uint64_t *host_hi) {
    if (f->n_groups == 0) return DD_OK;
    HIP_TRY(hipMemcpy(host_hi, f->hi, (size_t)f->n_groups * f->n_aggs * 8,
                      hipMemcpyDeviceToHost));
    return DD_OK;
}

extern "C" dd_status dd_finalizer_kernel_ms(const dd_finalizer *f, float *out3) {
    if (!f || !out3) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(out3, f->kernel_ms, sizeof(f->kernel_ms));
    return DD_OK;
}

/* The merged rows as typed device columns (k_final_columns): n_keys key
 * columns, n_aggs aggregate columns, then n_aggs i64 nn columns when with_nn. The finalizer
 * keeps no plan, so the key dtypes and the ops of the run are passed again. */
extern "C" dd_status dd_finalizer_columns(dd_finalizer *f, const int32_t *key_dtypes,
                                          int32_t n_keys, const int32_t *agg_ops,
                                          int32_t n_aggs, int32_t with_nn, void *stream) {
    if (!f || !key_dtypes || !agg_ops) return set_err(DD_ERR_INVALID, "null argument");
    if (n_keys != f->n_keys || n_aggs != f->n_aggs)
        return set_err(DD_ERR_INVALID, "final columns: key / aggregate count differs from "
                                       "the merge's");
    dd_final_cols c;
    memset(&c, 0, sizeof(c));
    c.n_keys = n_keys;
    c.n_aggs = n_aggs;
    for (int k = 0; k < n_keys; k++) {
        switch (key_dtypes[k]) {
        case DD_DT_U8: case DD_DT_BOOL: case DD_DT_I16: case DD_DT_I32: case DD_DT_I64:
        case DD_DT_F32: case DD_DT_F64:
            break;
        default:
            return set_err(DD_ERR_INVALID, "final columns: not a final merge key dtype");
        }
        c.key_dtype[k] = key_dtypes[k];
    }
    for (int j = 0; j < n_aggs; j++) {
        if (agg_ops[j] < 0 || agg_ops[j] > DD_AGG_SUM_DEC128)
            return set_err(DD_ERR_INVALID, "final columns: unknown aggregate op");
        c.ops[j] = agg_ops[j];
    }
    std::vector<void *> &col_data = f->cols.data;
    std::vector<uint8_t *> &col_validity = f->cols.validity;
    f->cols.clear();
    const int64_t ng = f->n_groups;
    const int n_cols = n_keys + n_aggs * (with_nn ? 2 : 1);
    f->col_dtype.assign((size_t)n_cols, 0);
    col_data.assign((size_t)n_cols, nullptr);
    col_validity.assign((size_t)n_cols, nullptr);
    for (int i = 0; i < n_cols; i++) {
        int dt = DD_DT_I64; /* count, the i64 aggregates, nn */
        bool has_valid = true;
        if (i < n_keys) {
            dt = key_dtypes[i];
        } else if (i < n_keys + n_aggs) {
            const int op = agg_ops[i - n_keys];
            if (op == DD_AGG_SUM_DEC128) dt = DD_DT_DEC128;
            else if (op == DD_AGG_SUM_F64 || op == DD_AGG_MIN_F64 || op == DD_AGG_MAX_F64)
                dt = DD_DT_F64;
            has_valid = op != DD_AGG_COUNT;
        } else {
            has_valid = false;
        }
        f->col_dtype[i] = dt;
        if (ng == 0) continue; /* no device work, as the run itself at zero rows */
        HIP_TRY(hipMalloc(&col_data[i], (size_t)ng * fixed_elem_size(dt)));
        if (has_valid) HIP_TRY(hipMalloc((void **)&col_validity[i], (size_t)ng));
        if (i < n_keys) {
            c.key_data[i] = col_data[i];
            c.key_valid[i] = col_validity[i];
        } else if (i < n_keys + n_aggs) {
            c.agg_data[i - n_keys] = col_data[i];
            c.agg_valid[i - n_keys] = col_validity[i];
        } else {
            c.nn_data[i - n_keys - n_aggs] = (int64_t *)col_data[i];
        }
    }
    if (ng == 0) return DD_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(dd_launch_final_columns(&c, ng, f->keys, f->keynull, f->aggs, f->hi, f->nn, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DD_OK;
}

extern "C" int32_t dd_finalizer_n_cols(const dd_finalizer *f) {
    return f ? (int32_t)f->cols.data.size() : 0;
}

extern "C" int32_t dd_finalizer_col_dtype(const dd_finalizer *f, int32_t i) {
    return f && i >= 0 && i < (int32_t)f->col_dtype.size() ? f->col_dtype[i] : 0;
}

extern "C" const void *dd_finalizer_col_data(const dd_finalizer *f, int32_t i) {
    return f ? f->cols.data_at(i) : nullptr;
}

extern "C" const uint8_t *dd_finalizer_col_validity(const dd_finalizer *f, int32_t i) {
    return f ? f->cols.validity_at(i) : nullptr;
}

extern "C" void dd_finalizer_destroy(dd_finalizer *f) { delete f; }

/* ---------------- hash join above two shuffles (dd_joiner) ---------- */

struct dd_joiner {
    int64_t n_rows = 0;
    std::vector<int64_t> seg_offsets; /* [output segments + 1] */
    uint32_t *build_idx = nullptr, *probe_idx = nullptr;
    dd_out_cols cols;                     /* build_proj's columns, then probe_proj's */
    float kernel_ms[5] = {0, 0, 0, 0, 0}; /* build, count, scan, emit, gather */
    ~dd_joiner() {
        (void)hipFree(build_idx);
        (void)hipFree(probe_idx);
    }
};

/* key and projection checks of one side */
static dd_status dd_join_check_side(const char *side, const dd_batch_desc *b,
                                    const int32_t *keys, int32_t n_keys, const int32_t *proj,
                                    int32_t n_proj) {
    const std::string who = std::string("hash join: ") + side + " ";
    if (b->n_rows < 0 || b->n_rows >= ((int64_t)1 << 31))
        return set_err(DD_ERR_INVALID, who + "n_rows must be below 2^31 (row ids are 32-bit "
                                             "table entries)");
    if (b->n_cols < 1 || b->n_cols > DD_MAX_COLS)
        return set_err(DD_ERR_INVALID, who + "column count out of range");
    for (int k = 0; k < n_keys; k++) {
        if (keys[k] < 0 || keys[k] >= b->n_cols)
            return set_err(DD_ERR_INVALID, who + "key column index out of range");
        switch (b->cols[keys[k]].dtype) {
        case DD_DT_F32: case DD_DT_F64:
            return set_err(DD_ERR_UNSUPPORTED,
                           who + "f32 / f64 keys are not supported: Arrow compares float join "
                                 "keys by total order, the key bits here canonicalise -0.0 "
                                 "and NaN");
        case DD_DT_DICT32:
            return set_err(DD_ERR_UNSUPPORTED, who + "dict32 keys are not supported");
        case DD_DT_UTF8:
            return set_err(DD_ERR_UNSUPPORTED, who + "utf8 / utf8view keys are not supported");
        case DD_DT_DEC128:
            return set_err(DD_ERR_UNSUPPORTED, who + "dec128 keys are not supported");
        case DD_DT_U8: case DD_DT_BOOL: case DD_DT_I16: case DD_DT_I32: case DD_DT_I64:
            break;
        default:
            return set_err(DD_ERR_INVALID, who + "unknown key dtype");
        }
    }
    return dd_check_projection(who, b, proj, n_proj);
}

static dd_status dd_join_check_n_keys(int32_t n_keys) {
    if (n_keys > 4) return set_err(DD_ERR_UNSUPPORTED, "hash join: more than 4 key columns");
    if (n_keys < 1) return set_err(DD_ERR_INVALID, "hash join: at least 1 key column");
    return DD_OK;
}

/* The body of dd_hash_join_run and dd_hash_join_outer_run, which have validated join_type
 * and n_keys. `who` opens the messages the two entries word differently. What a join type
 * scans and keeps:
 *   inner, right_semi, right_anti: the probe rows, in the probe side's segments;
 *   left_semi, left_anti: the build rows, in the build side's segments;
 *   left, right, full (outer): the probe rows in the probe side's segments; keep_probe: those
 *   without a match come out with the build side NULL; keep_build: the unmatched build rows
 *   follow in a second section, the build side's segments, with the probe side NULL. */
static dd_status dd_join_run(
    const std::string &who, const dd_batch_desc *build, const int32_t *build_keys,
    const dd_batch_desc *probe, const int32_t *probe_keys, int32_t n_keys, int32_t join_type,
    const int64_t *build_seg_offsets, const int32_t *build_seg_part, int32_t build_n_segs,
    int32_t build_n_parts, const int64_t *probe_seg_offsets, const int32_t *probe_seg_part,
    int32_t probe_n_segs, int32_t probe_n_parts, const int32_t *build_proj,
    int32_t n_build_proj, const int32_t *probe_proj, int32_t n_probe_proj, void *stream,
    dd_joiner **out) {
    /* all before any device work: both sides' keys and projections, both layouts,
     * co-partitioning, and the table regions from the BUILD side's rows per partition */
    dd_status st = dd_join_check_side("build side:", build, build_keys, n_keys, build_proj,
                                      n_build_proj);
    if (st != DD_OK) return st;
    st = dd_join_check_side("probe side:", probe, probe_keys, n_keys, probe_proj, n_probe_proj);
    if (st != DD_OK) return st;
    for (int k = 0; k < n_keys; k++)
        if (build->cols[build_keys[k]].dtype != probe->cols[probe_keys[k]].dtype)
            return set_err(DD_ERR_INVALID, "hash join: key dtypes differ pairwise (key " +
                                               std::to_string(k) + ")");
    if (n_build_proj + n_probe_proj > DD_MAX_COLS)
        return set_err(DD_ERR_INVALID, "hash join: more output columns than a batch holds");
    std::vector<int64_t> rows_b, rows_p;
    st = dd_check_layout("hash join: malformed build segment layout: ", build->n_rows,
                         build_seg_offsets, build_seg_part, build_n_segs, build_n_parts, &rows_b);
    if (st != DD_OK) return st;
    st = dd_check_layout("hash join: malformed probe segment layout: ", probe->n_rows,
                         probe_seg_offsets, probe_seg_part, probe_n_segs, probe_n_parts, &rows_p);
    if (st != DD_OK) return st;
    if (build_n_parts != probe_n_parts)
        return set_err(DD_ERR_INVALID, "hash join: unequal n_parts: the two sides must be "
                                       "co-partitioned");
    const int32_t n_parts = build_n_parts;
    dd_table_regions reg;
    if (!reg.size(rows_b))
        return set_err(DD_ERR_UNSUPPORTED, "hash join: build table past 2^32 slots");

    const bool outer = join_type >= DD_JOIN_LEFT;
    const bool left = join_type == DD_JOIN_LEFT_SEMI || join_type == DD_JOIN_LEFT_ANTI;
    const bool right = join_type == DD_JOIN_RIGHT_SEMI || join_type == DD_JOIN_RIGHT_ANTI;
    const bool anti = join_type == DD_JOIN_LEFT_ANTI || join_type == DD_JOIN_RIGHT_ANTI;
    const bool keep_probe = outer && join_type != DD_JOIN_LEFT;
    const bool keep_build = outer && join_type != DD_JOIN_RIGHT;
    const int64_t nb_rows = build->n_rows, np_rows = probe->n_rows;
    const int64_t n_tail = keep_build ? nb_rows : 0;
    const int64_t n_scan = left ? nb_rows : np_rows + n_tail; /* < 2^32 */
    const int32_t o_n_segs = left ? build_n_segs : probe_n_segs + (keep_build ? build_n_segs : 0);

    auto j = std::unique_ptr<dd_joiner>(new dd_joiner());
    j->seg_offsets.assign((size_t)o_n_segs + 1, 0);
    if (n_scan == 0) { /* nothing can come out: zero rows, no device work */
        *out = j.release();
        return DD_OK;
    }
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");

    /* an outer join's scan boundaries over cnt[np_rows + n_tail]: the probe segments, then
     * the build segments shifted behind the probe rows */
    std::vector<int64_t> oseg_h;
    if (outer) {
        oseg_h.assign(probe_seg_offsets, probe_seg_offsets + probe_n_segs + 1);
        if (keep_build)
            for (int s = 1; s <= build_n_segs; s++)
                oseg_h.push_back(np_rows + build_seg_offsets[s]);
    }

    dd_kargs kb, kp;
    dd_fill_kargs(build, build_keys, n_keys, &kb);
    dd_fill_kargs(probe, probe_keys, n_keys, &kp);

    hipStream_t s = (hipStream_t)stream;
    dd_dev_scratch ws;
    int64_t *d_bseg_off = nullptr, *d_pseg_off = nullptr, *d_oseg_off = nullptr,
            *d_seg_out = nullptr;
    int32_t *d_bseg_part = nullptr, *d_pseg_part = nullptr;
    uint32_t *d_base = nullptr, *d_log2 = nullptr, *table = nullptr, *next = nullptr,
             *cnt = nullptr, *head = nullptr, *err = nullptr;
    uint64_t *sums = nullptr;
    uint8_t *matched = nullptr; /* per build row, where build rows are emitted */
    const size_t n_pad = ((size_t)n_scan + 3) & ~(size_t)3;
    const size_t nb = (n_pad + DD_J_SCAN_TILE - 1) / DD_J_SCAN_TILE;
    if (!ws.alloc(&d_seg_out, ((size_t)o_n_segs + 2) * 8) ||
        !ws.alloc(&table, (size_t)reg.n_slots * 4) || !ws.alloc(&next, (size_t)nb_rows * 4) ||
        !ws.alloc(&cnt, n_pad * 4) || (outer && !ws.alloc(&head, (size_t)np_rows * 4)) ||
        !ws.alloc(&sums, (nb + 1) * 8) || !ws.alloc(&err, 4) ||
        ((left || keep_build) && !ws.alloc(&matched, (size_t)nb_rows)))
        return set_err(DD_ERR_HIP, who + "workspace alloc");
    dd_events<7> ev;
    HIP_TRY(ev.init());
    HIP_TRY(ws.upload(&d_bseg_off, build_seg_offsets, (size_t)build_n_segs + 1, s));
    HIP_TRY(ws.upload(&d_bseg_part, build_seg_part, (size_t)build_n_segs, s));
    HIP_TRY(ws.upload(&d_pseg_off, probe_seg_offsets, (size_t)probe_n_segs + 1, s));
    HIP_TRY(ws.upload(&d_pseg_part, probe_seg_part, (size_t)probe_n_segs, s));
    if (outer) HIP_TRY(ws.upload(&d_oseg_off, oseg_h.data(), oseg_h.size(), s));
    HIP_TRY(ws.upload(&d_base, reg.base.data(), (size_t)n_parts, s));
    HIP_TRY(ws.upload(&d_log2, reg.log2.data(), (size_t)n_parts, s));
    HIP_TRY(hipMemsetAsync(err, 0, 4, s));
    HIP_TRY(hipStreamSynchronize(s)); /* the uploads have left their pageable sources */
    const int64_t *d_scan_off = outer ? d_oseg_off : left ? d_bseg_off : d_pseg_off;

    HIP_TRY(ev.record(0, s));
    HIP_TRY(hipMemsetAsync(table, 0xff, (size_t)reg.n_slots * 4, s)); /* DD_F_EMPTY */
    if (nb_rows) HIP_TRY(hipMemsetAsync(next, 0xff, (size_t)nb_rows * 4, s));
    HIP_TRY(dd_launch_join_build(&kb, d_bseg_off, d_bseg_part, build_n_segs, d_base, d_log2,
                                 table, next, err, s));
    HIP_TRY(ev.record(1, s));
    HIP_TRY(hipMemsetAsync(cnt, 0, n_pad * 4, s));
    if (matched && nb_rows) HIP_TRY(hipMemsetAsync(matched, 0, (size_t)nb_rows, s));
    if (outer)
        HIP_TRY(dd_launch_join_count_outer(&kb, &kp, d_pseg_off, d_pseg_part, probe_n_segs,
                                           d_base, d_log2, table, next, keep_probe, head, cnt,
                                           matched, s));
    else
        HIP_TRY(dd_launch_join_count(&kb, &kp, d_pseg_off, d_pseg_part, probe_n_segs, d_base,
                                     d_log2, table, next, join_type, cnt, matched, s));
    if (left) HIP_TRY(dd_launch_join_left_cnt(matched, nb_rows, anti, cnt, s));
    if (keep_build) HIP_TRY(dd_launch_join_build_cnt_outer(matched, nb_rows, np_rows, cnt, s));
    HIP_TRY(ev.record(2, s));
    HIP_TRY(dd_launch_join_scan(cnt, n_scan, sums, d_scan_off, o_n_segs, d_seg_out, s));
    HIP_TRY(ev.record(3, s));
    /* the one mid-run sync: the output is sized by the result */
    std::vector<int64_t> seg_out_h((size_t)o_n_segs + 2);
    uint32_t err_h = 0;
    HIP_TRY(hipMemcpyAsync(seg_out_h.data(), d_seg_out, ((size_t)o_n_segs + 2) * 8,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&err_h, err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err_h) return set_err(DD_ERR_HIP, who + "build table overflow (internal)");
    const uint64_t total = (uint64_t)seg_out_h[(size_t)o_n_segs + 1];
    if (total >= ((uint64_t)1 << 31))
        return set_err(DD_ERR_UNSUPPORTED, who + "output of " + std::to_string(total) +
                                               " rows is 2^31 or more: chunk the probe side");
    const int64_t n_out = (int64_t)total;
    j->n_rows = n_out;
    memcpy(j->seg_offsets.data(), seg_out_h.data(), ((size_t)o_n_segs + 1) * 8);

    const size_t idx_bytes = n_out ? (size_t)n_out * 4 : 1;
    if (!right) HIP_TRY(hipMalloc((void **)&j->build_idx, idx_bytes));
    if (!left) HIP_TRY(hipMalloc((void **)&j->probe_idx, idx_bytes));
    dd_join_gather gb, gp;
    memset(&gb, 0, sizeof(gb));
    memset(&gp, 0, sizeof(gp));
    /* a NULL-extended side (build when probe rows are kept, probe when build rows are)
     * always carries validity */
    for (int i = 0; i < n_build_proj; i++)
        HIP_TRY(j->cols.add(build->cols[build_proj[i]], n_out, keep_probe, &gb));
    for (int i = 0; i < n_probe_proj; i++)
        HIP_TRY(j->cols.add(probe->cols[probe_proj[i]], n_out, keep_build, &gp));
    HIP_TRY(ev.record(4, s));
    /* every index is written by the emit; preset first so that no gather ever reads an index
     * this run did not produce: to 0, or for an outer join to DD_JOIN_NONE, which its gather
     * never follows */
    if (j->build_idx) HIP_TRY(hipMemsetAsync(j->build_idx, outer ? 0xff : 0, idx_bytes, s));
    if (j->probe_idx) HIP_TRY(hipMemsetAsync(j->probe_idx, outer ? 0xff : 0, idx_bytes, s));
    if (outer)
        HIP_TRY(dd_launch_join_emit_outer(head, next, matched, cnt, np_rows, n_tail, keep_probe,
                                          (uint32_t)n_out, j->build_idx, j->probe_idx, s));
    else if (left)
        HIP_TRY(dd_launch_join_emit_build(matched, nb_rows, anti, cnt, (uint32_t)n_out,
                                          j->build_idx, s));
    else
        HIP_TRY(dd_launch_join_emit_probe(&kb, &kp, d_pseg_off, d_pseg_part, probe_n_segs,
                                          d_base, d_log2, table, next, join_type, cnt,
                                          (uint32_t)n_out, j->build_idx, j->probe_idx, s));
    HIP_TRY(ev.record(5, s));
    auto gather = outer ? dd_launch_join_gather_outer : dd_launch_join_gather;
    HIP_TRY(gather(&gb, j->build_idx, n_out, s));
    HIP_TRY(gather(&gp, j->probe_idx, n_out, s));
    HIP_TRY(ev.record(6, s));
    HIP_TRY(hipStreamSynchronize(s));
    ev.elapsed(&j->kernel_ms[0], 0, 1);
    ev.elapsed(&j->kernel_ms[1], 1, 2);
    ev.elapsed(&j->kernel_ms[2], 2, 3);
    ev.elapsed(&j->kernel_ms[3], 4, 5);
    ev.elapsed(&j->kernel_ms[4], 5, 6);
    *out = j.release();
    return DD_OK;
}

extern "C" dd_status dd_hash_join_run(
    const dd_batch_desc *build, const int32_t *build_keys, const dd_batch_desc *probe,
    const int32_t *probe_keys, int32_t n_keys, int32_t join_type,
    const int64_t *build_seg_offsets, const int32_t *build_seg_part, int32_t build_n_segs,
    int32_t build_n_parts, const int64_t *probe_seg_offsets, const int32_t *probe_seg_part,
    int32_t probe_n_segs, int32_t probe_n_parts, const int32_t *build_proj,
    int32_t n_build_proj, const int32_t *probe_proj, int32_t n_probe_proj, void *stream,
    dd_joiner **out) {
    if (!build || !build_keys || !probe || !probe_keys || !build_seg_offsets ||
        !build_seg_part || !probe_seg_offsets || !probe_seg_part || !out)
        return set_err(DD_ERR_INVALID, "hash join: null argument");
    if (join_type == DD_JOIN_LEFT || join_type == DD_JOIN_RIGHT || join_type == DD_JOIN_FULL)
        return set_err(DD_ERR_UNSUPPORTED, "hash join: outer joins (left, right, full) are not "
                                           "supported");
    if (join_type < DD_JOIN_INNER || join_type > DD_JOIN_FULL)
        return set_err(DD_ERR_INVALID, "hash join: unknown join type");
    dd_status st = dd_join_check_n_keys(n_keys);
    if (st != DD_OK) return st;
    const bool left = join_type == DD_JOIN_LEFT_SEMI || join_type == DD_JOIN_LEFT_ANTI;
    const bool right = join_type == DD_JOIN_RIGHT_SEMI || join_type == DD_JOIN_RIGHT_ANTI;
    if (left && n_probe_proj != 0)
        return set_err(DD_ERR_INVALID, "hash join: a left_semi / left_anti join emits build "
                                       "rows: a probe-side projection list is not allowed");
    if (right && n_build_proj != 0)
        return set_err(DD_ERR_INVALID, "hash join: a right_semi / right_anti join emits probe "
                                       "rows: a build-side projection list is not allowed");
    return dd_join_run("hash join: ", build, build_keys, probe, probe_keys, n_keys, join_type,
                       build_seg_offsets, build_seg_part, build_n_segs, build_n_parts,
                       probe_seg_offsets, probe_seg_part, probe_n_segs, probe_n_parts,
                       build_proj, n_build_proj, probe_proj, n_probe_proj, stream, out);
}

/* outer joins: left, right, full */
extern "C" dd_status dd_hash_join_outer_run(
    const dd_batch_desc *build, const int32_t *build_keys, const dd_batch_desc *probe,
    const int32_t *probe_keys, int32_t n_keys, int32_t join_type,
    const int64_t *build_seg_offsets, const int32_t *build_seg_part, int32_t build_n_segs,
    int32_t build_n_parts, const int64_t *probe_seg_offsets, const int32_t *probe_seg_part,
    int32_t probe_n_segs, int32_t probe_n_parts, const int32_t *build_proj,
    int32_t n_build_proj, const int32_t *probe_proj, int32_t n_probe_proj, void *stream,
    dd_joiner **out) {
    if (!build || !build_keys || !probe || !probe_keys || !build_seg_offsets ||
        !build_seg_part || !probe_seg_offsets || !probe_seg_part || !out)
        return set_err(DD_ERR_INVALID, "hash join: null argument");
    if (join_type < DD_JOIN_INNER || join_type > DD_JOIN_FULL)
        return set_err(DD_ERR_INVALID, "outer join: unknown join type");
    if (join_type != DD_JOIN_LEFT && join_type != DD_JOIN_RIGHT && join_type != DD_JOIN_FULL)
        return set_err(DD_ERR_INVALID, "outer join: inner, semi and anti joins are "
                                       "dd_hash_join_run's; this entry takes left, right and "
                                       "full");
    dd_status st = dd_join_check_n_keys(n_keys);
    if (st != DD_OK) return st;
    return dd_join_run("outer join: ", build, build_keys, probe, probe_keys, n_keys, join_type,
                       build_seg_offsets, build_seg_part, build_n_segs, build_n_parts,
                       probe_seg_offsets, probe_seg_part, probe_n_segs, probe_n_parts,
                       build_proj, n_build_proj, probe_proj, n_probe_proj, stream, out);
}

extern "C" int64_t dd_joiner_n_rows(const dd_joiner *j) { return j ? j->n_rows : 0; }

extern "C" int32_t dd_joiner_n_segs(const dd_joiner *j) {
    return j ? (int32_t)j->seg_offsets.size() - 1 : 0;
}

extern "C" dd_status dd_joiner_seg_offsets(const dd_joiner *j, int64_t *host_out) {
    if (!j || !host_out) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(host_out, j->seg_offsets.data(), j->seg_offsets.size() * 8);
    return DD_OK;
}

extern "C" const uint32_t *dd_joiner_build_idx(const dd_joiner *j) { return j->build_idx; }
extern "C" const uint32_t *dd_joiner_probe_idx(const dd_joiner *j) { return j->probe_idx; }

extern "C" const void *dd_joiner_col_data(const dd_joiner *j, int32_t i) {
    return j ? j->cols.data_at(i) : nullptr;
}

extern "C" const uint8_t *dd_joiner_col_validity(const dd_joiner *j, int32_t i) {
    return j ? j->cols.validity_at(i) : nullptr;
}

extern "C" dd_status dd_joiner_kernel_ms(const dd_joiner *j, float *out5) {
    if (!j || !out5) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(out5, j->kernel_ms, sizeof(j->kernel_ms));
    return DD_OK;
}

extern "C" void dd_joiner_destroy(dd_joiner *j) { delete j; }

/* ---------------- sort / top-k above the shuffle (dd_sorter) -------------- */

struct dd_sorter {
    int64_t n_rows = 0;               /* output rows, after fetch */
    std::vector<int64_t> seg_offsets; /* [n_parts + 1] */
    uint32_t *perm = nullptr;         /* source row of each output row */
    dd_out_cols cols;                 /* the projected columns */
    int32_t info[4] = {0, 0, DD_S_TILE, 0}; /* passes planned, passes run, tile rows, words */
    float kernel_ms[4] = {0, 0, 0, 0};      /* encode + census, passes, seg out, gather */
    ~dd_sorter() { (void)hipFree(perm); }
};

extern "C" dd_status dd_sort_run(const dd_batch_desc *batch, const int32_t *key_cols,
                                 const int32_t *key_flags, int32_t n_keys,
                                 const int32_t *proj_cols, int32_t n_proj,
                                 const int64_t *seg_offsets, const int32_t *seg_part,
                                 int32_t n_segs, int32_t n_parts, int64_t fetch, void *stream,
                                 dd_sorter **out) {
    if (!batch || !key_cols || !key_flags || !seg_offsets || !seg_part || !out)
        return set_err(DD_ERR_INVALID, "sort: null argument");
    if (n_keys < 1 || n_keys > DD_S_MAX_KEYS)
        return set_err(DD_ERR_INVALID, "sort: 1..4 sort keys");
    if (fetch < -1) return set_err(DD_ERR_INVALID, "sort: fetch must be -1 (all rows) or >= 0");
    const int64_t n = batch->n_rows;
    if (n < 0 || n >= ((int64_t)1 << 31))
        return set_err(DD_ERR_INVALID, "sort: n_rows must be below 2^31 (perm holds 32-bit row "
                                       "ids)");
    if (batch->n_cols < 1 || batch->n_cols > DD_MAX_COLS)
        return set_err(DD_ERR_INVALID, "sort: column count out of range");
    for (int k = 0; k < n_keys; k++) {
        if (key_cols[k] < 0 || key_cols[k] >= batch->n_cols)
            return set_err(DD_ERR_INVALID, "sort: key column index out of range");
        if (key_flags[k] & ~(DD_SORT_DESC | DD_SORT_NULLS_FIRST))
            return set_err(DD_ERR_INVALID, "sort: unknown key flag bits");
        const dd_col_desc &cd = batch->cols[key_cols[k]];
        switch (cd.dtype) {
        case DD_DT_DICT32:
            return set_err(DD_ERR_UNSUPPORTED,
                           "sort: dict32 keys are not supported: dictionary index order is "
                           "not value order");
        case DD_DT_UTF8:
            return set_err(DD_ERR_UNSUPPORTED, "sort: utf8 / utf8view keys are not supported");
        case DD_DT_DEC128:
            if ((uintptr_t)cd.data % 16)
                return set_err(DD_ERR_INVALID, "sort: dec128 key data must be 16-byte aligned");
            break;
        case DD_DT_U8: case DD_DT_BOOL: case DD_DT_I16: case DD_DT_I32: case DD_DT_I64:
        case DD_DT_F32: case DD_DT_F64:
            break;
        default:
            return set_err(DD_ERR_INVALID, "sort: unknown key dtype");
        }
    }
    if (dd_status st = dd_check_projection("sort: ", batch, proj_cols, n_proj)) return st;
    std::vector<int64_t> rows_p;
    if (dd_status st = dd_check_layout("sort: malformed segment layout: ", n, seg_offsets,
                                       seg_part, n_segs, n_parts, &rows_p))
        return st;
    /* rows per partition -> where each partition starts in the sorted order, and in the
     * output once fetch has cut it */
    std::vector<int64_t> in_off((size_t)n_parts + 1, 0), out_off((size_t)n_parts + 1, 0);
    for (int p = 0; p < n_parts; p++) {
        const int64_t rows = rows_p[p];
        out_off[(size_t)p + 1] = out_off[p] + (fetch >= 0 && fetch < rows ? fetch : rows);
        in_off[(size_t)p + 1] = in_off[p] + rows;
    }
    const int64_t n_out = out_off[n_parts];

    dd_sort_keys sk;
    memset(&sk, 0, sizeof(sk));
    sk.n_keys = n_keys;
    int word_of[DD_S_MAX_KEYS];
    int nw = 0;
    for (int k = 0; k < n_keys; k++) {
        const dd_col_desc &cd = batch->cols[key_cols[k]];
        sk.dtype[k] = cd.dtype;
        sk.flags[k] = key_flags[k];
        sk.data[k] = cd.data;
        sk.valid[k] = (const uint8_t *)cd.validity;
        word_of[k] = nw;
        sk.wkey[nw] = k;
        sk.wpart[nw++] = 0;
        if (cd.dtype == DD_DT_DEC128) {
            sk.wkey[nw] = k;
            sk.wpart[nw++] = 1;
        }
    }
    const int meta = nw;
    sk.wkey[meta] = -1;
    sk.n_words = nw + 1;

    auto so = std::unique_ptr<dd_sorter>(new dd_sorter());
    so->n_rows = n_out;
    so->seg_offsets = out_off;
    so->info[3] = sk.n_words;
    if (n_out == 0) { /* no rows, or fetch = 0: empty segments, no device work */
        *out = so.release();
        return DD_OK;
    }
    if (dd_device_count() == 0) return set_err(DD_ERR_NO_DEVICE, "no HIP device");

    hipStream_t s = (hipStream_t)stream;
    const size_t n_tiles = (size_t)((n + DD_S_TILE - 1) / DD_S_TILE);
    const size_t n_h = n_tiles * 256;
    const size_t nb = (n_h + DD_S_SCAN_TILE - 1) / DD_S_SCAN_TILE;
    const size_t census_n = (size_t)sk.n_words * 8 * 256;
    dd_dev_scratch ws;
    int64_t *d_seg_off = nullptr, *d_in_off = nullptr, *d_out_off = nullptr;
    int32_t *d_seg_part = nullptr;
    uint64_t *words = nullptr, *wbuf[2] = {nullptr, nullptr};
    uint32_t *pbuf[2] = {nullptr, nullptr}, *census = nullptr, *hist = nullptr, *sums = nullptr;
    if (!ws.alloc(&words, (size_t)sk.n_words * (size_t)n * 8) ||
        !ws.alloc(&wbuf[0], (size_t)n * 8) || !ws.alloc(&wbuf[1], (size_t)n * 8) ||
        !ws.alloc(&pbuf[0], (size_t)n * 4) || !ws.alloc(&pbuf[1], (size_t)n * 4) ||
        !ws.alloc(&census, census_n * 4) || !ws.alloc(&hist, n_h * 4) ||
        !ws.alloc(&sums, (nb + 1) * 4))
        return set_err(DD_ERR_HIP, "sort: workspace alloc");
    dd_events<6> ev;
    HIP_TRY(ev.init());
    HIP_TRY(ws.upload(&d_seg_off, seg_offsets, (size_t)n_segs + 1, s));
    HIP_TRY(ws.upload(&d_seg_part, seg_part, (size_t)n_segs, s));
    HIP_TRY(ws.upload(&d_in_off, in_off.data(), (size_t)n_parts + 1, s));
    HIP_TRY(ws.upload(&d_out_off, out_off.data(), (size_t)n_parts + 1, s));
    HIP_TRY(hipStreamSynchronize(s)); /* the uploads have left their pageable sources */

    HIP_TRY(ev.record(0, s));
    HIP_TRY(hipMemsetAsync(census, 0, census_n * 4, s));
    HIP_TRY(dd_launch_sort_encode(&sk, n, d_seg_off, d_seg_part, n_segs, words, pbuf[0], census,
                                  s));
    HIP_TRY(ev.record(1, s));
    /* the run's one mid-run synchronisation: the census decides which passes run */
    std::vector<uint32_t> census_h(census_n);
    HIP_TRY(hipMemcpyAsync(census_h.data(), census, census_n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    /* DD_SORT_SKIP=0: run every planned pass (A/B and tests); read per call */
    const char *skip_env = getenv("DD_SORT_SKIP");
    const bool skip = !(skip_env && atoi(skip_env) == 0);
    struct dd_sort_pass {
        int word, shift;
    };
    std::vector<dd_sort_pass> passes;
    int planned = 0;
    /* byte j of word w: dropped when one bin holds every row */
    auto consider = [&](int w, int j) {
        planned++;
        const uint32_t *h = census_h.data() + ((size_t)w * 8 + j) * 256;
        bool constant = false;
        for (int b = 0; b < 256; b++) constant = constant || h[b] == (uint32_t)n;
        if (!skip || !constant) passes.push_back({w, 8 * j});
    };
    /* least significant first: the last key's low digit ... the first key's null rank, then
     * the partition id */
    for (int k = n_keys - 1; k >= 0; k--) {
        if (sk.dtype[k] == DD_DT_DEC128) {
            for (int j = 0; j < 8; j++) consider(word_of[k] + 1, j);
            for (int j = 0; j < 8; j++) consider(word_of[k], j);
        } else {
            const int nd = fixed_elem_size(sk.dtype[k]);
            for (int j = 0; j < nd; j++) consider(word_of[k], j);
        }
        if (sk.valid[k]) consider(meta, k);
    }
    int pbits = 0;
    while (((int64_t)1 << pbits) < n_parts) pbits++;
    for (int j = 0; j < (pbits + 7) / 8; j++) consider(meta, 4 + j);
    so->info[0] = planned;
    so->info[1] = (int32_t)passes.size();

    HIP_TRY(ev.record(2, s));
    int wi = -1, pi = 0, cur_word = -1; /* wbuf / pbuf holding the current word and perm */
    for (const dd_sort_pass &ps : passes) {
        const uint64_t *src = words + (size_t)ps.word * (size_t)n;
        const uint64_t *win;
        if (ps.word == cur_word) {
            win = wbuf[wi];
        } else if (cur_word < 0) { /* perm is still the identity: the word array as it is */
            win = src;
        } else {
            HIP_TRY(dd_launch_sort_gather_word(src, pbuf[pi], n, wbuf[0], s));
            wi = 0;
            win = wbuf[0];
        }
        cur_word = ps.word;
        const int wo = wi < 0 ? 0 : 1 - wi;
        HIP_TRY(dd_launch_sort_pass(win, pbuf[pi], n, ps.shift, hist, sums, wbuf[wo],
                                    pbuf[1 - pi], s));
        wi = wo;
        pi = 1 - pi;
    }
    HIP_TRY(ev.record(3, s));
    HIP_TRY(hipMalloc((void **)&so->perm, (size_t)n_out * 4));
    HIP_TRY(dd_launch_sort_seg_out(pbuf[pi], d_in_off, d_out_off, n_parts, n_out, so->perm, s));
    HIP_TRY(ev.record(4, s));
    dd_join_gather g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < n_proj; i++)
        HIP_TRY(so->cols.add(batch->cols[proj_cols[i]], n_out, false, &g));
    HIP_TRY(dd_launch_join_gather(&g, so->perm, n_out, s));
    HIP_TRY(ev.record(5, s));
    HIP_TRY(hipStreamSynchronize(s));
    ev.elapsed(&so->kernel_ms[0], 0, 1);
    ev.elapsed(&so->kernel_ms[1], 2, 3);
    ev.elapsed(&so->kernel_ms[2], 3, 4);
    ev.elapsed(&so->kernel_ms[3], 4, 5);
    *out = so.release();
    return DD_OK;
}

extern "C" int64_t dd_sorter_n_rows(const dd_sorter *so) { return so ? so->n_rows : 0; }

extern "C" dd_status dd_sorter_seg_offsets(const dd_sorter *so, int64_t *host_out) {
    if (!so || !host_out) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(host_out, so->seg_offsets.data(), so->seg_offsets.size() * 8);
    return DD_OK;
}

extern "C" const uint32_t *dd_sorter_perm(const dd_sorter *so) { return so->perm; }

extern "C" const void *dd_sorter_col_data(const dd_sorter *so, int32_t i) {
    return so ? so->cols.data_at(i) : nullptr;
}

extern "C" const uint8_t *dd_sorter_col_validity(const dd_sorter *so, int32_t i) {
    return so ? so->cols.validity_at(i) : nullptr;
}

extern "C" dd_status dd_sorter_info(const dd_sorter *so, int32_t *out4) {
    if (!so || !out4) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(out4, so->info, sizeof(so->info));
    return DD_OK;
}

extern "C" dd_status dd_sorter_kernel_ms(const dd_sorter *so, float *out4) {
    if (!so || !out4) return set_err(DD_ERR_INVALID, "null argument");
    memcpy(out4, so->kernel_ms, sizeof(so->kernel_ms));
    return DD_OK;
}

extern "C" void dd_sorter_destroy(dd_sorter *so) { delete so; }

/* ---------------- coalesce (dd_coalesce_run) ---------------- */

/* task_group (network_coalesce.rs:376-400): contiguous ceil-split of producers */
static void dd_task_group(int input_tasks, int task_index, int task_count, int *start,
                          int *len) {
    const int base = input_tasks / task_count;
    const int extra = input_tasks % task_count;
    *len = base + (task_index < extra ? 1 : 0);
    *start = task_index * base + (task_index < extra ? task_index : extra);
}

extern "C" dd_status dd_coalesce_run(dd_comm *c, const dd_partitioner *p,
                                     int32_t consumer_tasks, void *stream,
                                     dd_exchanged **out) {
    if (!c || !p || !out) return set_err(DD_ERR_INVALID, "null argument");
    if (!p->has_run) return set_err(DD_ERR_INVALID, "partitioner has not run");
    if (consumer_tasks < 1 || consumer_tasks > c->nranks)
        return set_err(DD_ERR_INVALID, "consumer_tasks must be in [1, nranks]");
    hipStream_t s = (hipStream_t)stream;
    const int R = c->nranks;
    const uint32_t P = p->nparts;
    const int nvar = p->ka.n_var;

    /* 1) size matrix allgather (same meta layout as dd_exchange_run) */
    const size_t meta_n = (size_t)P * (1 + nvar);
    std::vector<int64_t> my_meta(meta_n);
    std::vector<int64_t> off_h(P + 1);
    dd_status st = dd_partitioner_row_offsets(p, off_h.data());
    if (st != DD_OK) return st;
    for (uint32_t q = 0; q < P; q++) my_meta[q] = off_h[q + 1] - off_h[q];
    std::vector<std::vector<int64_t>> boff_h(nvar, std::vector<int64_t>(P + 1));
    for (int v = 0; v < nvar; v++) {
        st = dd_partitioner_byte_offsets(p, p->ka.var_idx[v], boff_h[v].data());
        if (st != DD_OK) return st;
        for (uint32_t q = 0; q < P; q++)
            my_meta[(size_t)(1 + v) * P + q] = boff_h[v][q + 1] - boff_h[v][q];
    }
    std::vector<int64_t> all_meta((size_t)R * meta_n);
    {
        dd_status ms = dd_meta_allgather(c, my_meta, all_meta, s);
        if (ms != DD_OK) return ms;
    }

    /* 2) my group as a consumer (ranks >= consumer_tasks consume nothing) */
    int gstart = 0, glen = 0;
    if (c->rank < consumer_tasks) dd_task_group(R, c->rank, consumer_tasks, &gstart, &glen);
    /* my consumer as a producer: the consumer whose group contains me */
    int my_consumer = -1;
    for (int t = 0; t < consumer_tasks; t++) {
        int s0, l0;
        dd_task_group(R, t, consumer_tasks, &s0, &l0);
        if (c->rank >= s0 && c->rank < s0 + l0) my_consumer = t;
    }

    std::unique_ptr<dd_exchanged> e_own(new dd_exchanged()); /* freed on error returns */
    dd_exchanged *e = e_own.get();
    e->alloc_stream = dd_pool_stream();
    e->n_cols = p->batch.n_cols;
    e->nranks = glen; /* producers I consume */
    e->P = P;
    e->row_counts.assign((size_t)(glen > 0 ? glen : 1) * P, 0);
    e->byte_counts.assign(p->batch.n_cols, {});
    std::vector<int64_t> recv_rows(glen, 0);
    for (int gi = 0; gi < glen; gi++) {
        const int r = gstart + gi;
        for (uint32_t q = 0; q < P; q++) {
            int64_t n = all_meta[(size_t)r * meta_n + q];
            e->row_counts[(size_t)gi * P + q] = n;
            recv_rows[gi] += n;
            e->total_rows += n;
        }
    }
    auto fail = [&](dd_status sc, const char *m) { return set_err(sc, m); };

    std::vector<std::vector<int64_t>> recv_bytes(p->batch.n_cols,
                                                 std::vector<int64_t>(glen, 0));
    for (int ci = 0; ci < p->batch.n_cols; ci++) {
        const dd_kcol &kc = p->ka.cols[ci];
        if (kc.elem > 0) {
            if (hipMallocAsync(&e->data[ci], (size_t)e->total_rows * kc.elem + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "coalesce recv alloc");
        } else {
            int v = -1;
            for (int vv = 0; vv < nvar; vv++)
                if (p->ka.var_idx[vv] == ci) v = vv;
            e->byte_counts[ci].assign((size_t)(glen > 0 ? glen : 1) * P, 0);
            int64_t total_b = 0;
            for (int gi = 0; gi < glen; gi++) {
                const int r = gstart + gi;
                for (uint32_t q = 0; q < P; q++) {
                    int64_t b = all_meta[(size_t)r * meta_n + (size_t)(1 + v) * P + q];
                    e->byte_counts[ci][(size_t)gi * P + q] = b;
                    recv_bytes[ci][gi] += b;
                    total_b += b;
                }
            }
            if (hipMallocAsync(&e->data[ci], (size_t)total_b + 1, e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "coalesce recv alloc (var)");
            if (hipMallocAsync((void **)&e->lengths[ci], (size_t)e->total_rows * 4 + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "coalesce recv alloc (lengths)");
        }
        if (kc.valid) {
            if (hipMallocAsync((void **)&e->valid[ci], (size_t)e->total_rows + 1,
                               e->alloc_stream) != hipSuccess)
                return fail(DD_ERR_HIP, "coalesce recv alloc (validity)");
        }
    }
    if (hipStreamSynchronize(e->alloc_stream) != hipSuccess) /* allocations ready */
        return fail(DD_ERR_HIP, "pool stream sync");
    if (hipEventCreate(&e->e0) != hipSuccess || hipEventCreate(&e->e1) != hipSuccess)
        return fail(DD_ERR_HIP, "event create");

    /* 3) grouped p2p: I SEND my whole output to my_consumer; as a consumer I RECV from
     * each producer in my group, producer-major. Post order per peer: per col (data,
     * [lengths], [valid]) — symmetric on both sides. */
    const int64_t my_rows = off_h[P];
    HIP_TRY(hipEventRecord(e->e0, s));
    NCCL_TRY(ncclGroupStart());
    for (int ci = 0; ci < p->batch.n_cols; ci++) {
        const dd_kcol &kc = p->ka.cols[ci];
        /* sends (every rank has exactly one consumer) */
        if (my_consumer >= 0) {
            int64_t sent = 0;
            if (kc.elem > 0) {
                if (my_rows > 0)
                    NCCL_TRY(ncclSend(p->out_data[ci], my_rows * kc.elem, ncclUint8,
                                      my_consumer, c->comm, s));
                sent = my_rows * kc.elem;
            } else {
                int v = -1;
                for (int vv = 0; vv < nvar; vv++)
                    if (p->ka.var_idx[vv] == ci) v = vv;
                const int64_t my_b = boff_h[v][P];
                if (my_b > 0)
                    NCCL_TRY(ncclSend(p->out_data[ci], my_b, ncclUint8, my_consumer,
                                      c->comm, s));
                if (my_rows > 0)
                    NCCL_TRY(ncclSend(p->out_lengths[ci], my_rows * 4, ncclUint8,
                                      my_consumer, c->comm, s));
                sent = my_b + my_rows * 4;
            }
            if (kc.valid && my_rows > 0) {
                NCCL_TRY(ncclSend(p->out_valid[ci], my_rows, ncclUint8, my_consumer,
                                  c->comm, s));
                sent += my_rows;
            }
            if (my_consumer != c->rank) e->egress += sent;
        }
        /* recvs */
        int64_t rrow0 = 0, rb0 = 0;
        for (int gi = 0; gi < glen; gi++) {
            const int r = gstart + gi;
            if (kc.elem > 0) {
                if (recv_rows[gi] > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->data[ci] + rrow0 * kc.elem,
                                      recv_rows[gi] * kc.elem, ncclUint8, r, c->comm, s));
            } else {
                if (recv_bytes[ci][gi] > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->data[ci] + rb0, recv_bytes[ci][gi],
                                      ncclUint8, r, c->comm, s));
                if (recv_rows[gi] > 0)
                    NCCL_TRY(ncclRecv((uint8_t *)e->lengths[ci] + rrow0 * 4,
                                      recv_rows[gi] * 4, ncclUint8, r, c->comm, s));
                rb0 += recv_bytes[ci][gi];
            }
            if (kc.valid && recv_rows[gi] > 0)
                NCCL_TRY(ncclRecv(e->valid[ci] + rrow0, recv_rows[gi], ncclUint8, r,
                                  c->comm, s));
            rrow0 += recv_rows[gi];
        }
    }
    NCCL_TRY(ncclGroupEnd());
    HIP_TRY(hipEventRecord(e->e1, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&e->ms, e->e0, e->e1));
    *out = e_own.release();
    return DD_OK;
}

