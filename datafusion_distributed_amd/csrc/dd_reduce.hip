/* dd_reduce.hip — GPU partial aggregation below the shuffle.
 *
 * Mirrors the reference's partial-reduce pass (/root/reference/src/distributed_planner/
 * partial_reduce_below_network_shuffles.rs, enabled by `distributed.partial_reduce`,
 * distributed_config.rs:50-54): an AggregateExec mode=Partial is placed BELOW the
 * repartition so the exchange moves per-group partials instead of raw rows. Semantics are
 * DataFusion's partial aggregate: each invocation may emit DUPLICATE groups (one per
 * block here, one per input partition there); the downstream final aggregate merges them.
 * Output row order is unspecified (the reference's is stream-order; both are merged by
 * the order-insensitive final aggregate — test_utils/property_based.rs:15-41).
 *
 * Design: per-block LDS open-addressing table keyed by the normative row hash
 * (dd_row_hash — the same hash the shuffle uses). Claim a slot with an LDS CAS on the
 * hash word, publish key values behind a ready flag, aggregate with LDS atomics
 * (f64/u64 add). Rows that do not fit after a bounded probe spill to the output as
 * singleton groups (sum = value, count = 1) — correct for any cardinality, fast for the
 * low-cardinality keys partial-reduce targets (q1: 6 groups).
 *
 * Coverage: fixed-width and dict32-by-index key columns (nullable), aggregate ops
 * sum(f64) / sum(i64, wrapping) / count(*) / min / max (contract: include/dd_shuffle.h).
 * Plans with more than 4 aggregates or an exact decimal sum (sum(dec128), wrapping modulo
 * 2^128) run k_partial_reduce_wide at the end of this file.
 *
 * NULL semantics: each aggregate carries a NON-NULL INPUT COUNT in the partial state
 * (out_nn), so the downstream final merge can emit NULL for a group whose inputs were all
 * NULL — matching DataFusion, where SUM/MIN/MAX over an all-null group is NULL, not the
 * op identity. (COUNT counts every row it sees; its merge can never be NULL.) */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_agg_device.h"
#include "dd_hash_device.h"
#include "dd_internal.h"

#define RWAVE 64
#define R_THREADS 256
#define R_CAP DD_R_CAP     /* table slots per block (dd_internal.h) */
#define R_PROBE DD_R_PROBE /* bounded probe; then spill */

/* agg op codes come from include/dd_shuffle.h (via dd_internal.h); the order-preserving
 * min/max keys, the op identities and dd_key_bits live in dd_agg_device.h, shared with the
 * final merge (dd_final.hip) */

extern "C" __global__ __launch_bounds__(R_THREADS) void k_partial_reduce(
    dd_kargs a, int64_t chunk_rows, int n_aggs, const int32_t *agg_cols,
    const int32_t *agg_ops, uint64_t *out_keys /* [max_rows][n_keys] interleaved */,
    uint32_t *out_keynull /* [max_rows] bitmask */,
    double *out_aggs /* [max_rows][n_aggs] interleaved (i64 sums bit-cast) */,
    uint64_t *out_nn /* [max_rows][n_aggs] non-null input counts */,
    uint64_t *out_n /* global row counter */) {
    __shared__ uint64_t t_hash[R_CAP];
    __shared__ uint32_t t_ready[R_CAP];
    __shared__ uint64_t t_keys[DD_KMAX_KEYS > 4 ? 4 : DD_KMAX_KEYS][R_CAP];
    __shared__ uint32_t t_null[R_CAP];
    __shared__ unsigned long long t_agg[4][R_CAP]; /* f64 or i64 state, bit pattern */
    __shared__ uint32_t t_nn[4][R_CAP];            /* non-null input count per agg */

    const int nk = a.n_keys > 4 ? 4 : a.n_keys;
    for (int s = threadIdx.x; s < R_CAP; s += R_THREADS) {
        t_hash[s] = 0;
        t_ready[s] = 0;
        t_null[s] = 0;
        for (int k = 0; k < nk; k++) t_keys[k][s] = 0;
        for (int g = 0; g < n_aggs; g++) {
            t_agg[g][s] = dd_agg_identity(agg_ops[g]);
            t_nn[g][s] = 0;
        }
    }
    __syncthreads();

    const int64_t start = (int64_t)blockIdx.x * chunk_rows;
    const int64_t end = (start + chunk_rows < a.n_rows) ? (start + chunk_rows) : a.n_rows;

    for (int64_t row = start + threadIdx.x; row < end; row += R_THREADS) {
        uint64_t h = dd_row_hash<false>(a, row); /* host refuses dec128 keys */
        if (h == 0) h = 1; /* 0 is the empty sentinel */
        uint64_t kb[4];
        uint32_t knull = 0;
        for (int k = 0; k < nk; k++) {
            const dd_kcol &c = a.cols[a.key_idx[k]];
            const bool isnull = c.valid && !c.valid[row];
            if (isnull) knull |= 1u << k;
            kb[k] = isnull ? 0 : dd_key_bits(c, row);
        }
        int slot = -1;
        /* Two probe attempts. Within one divergent loop iteration a follower lane may not
         * observe its own wave's claimer publish (no independent thread scheduling, and
         * masked branch bodies need not interleave); after the first attempt's loop
         * reconverges, every publish from this wave IS visible, so attempt 2 matches
         * deterministically instead of claiming a duplicate slot per lane. */
        for (int attempt = 0; attempt < 2 && slot < 0; attempt++) {
        uint32_t s = (uint32_t)(h % R_CAP);
        for (int probe = 0; probe < R_PROBE; probe++, s = (s + 1) % R_CAP) {
            if (attempt == 0 && probe > 0) break; /* attempt 1: claim-or-match at home slot
                                                     only; defer the walk to attempt 2 */
            uint64_t cur = atomicCAS((unsigned long long *)&t_hash[s], 0ull,
                                     (unsigned long long)h);
            if (cur == 0) { /* claimed: publish keys, then ready */
                for (int k = 0; k < nk; k++) t_keys[k][s] = kb[k];
                t_null[s] = knull;
                __threadfence_block();
                atomicExch(&t_ready[s], 1u);
                slot = (int)s;
                break;
            }
            if (cur == h) {
                /* NEVER spin unboundedly on the publisher: the claimer may be a divergent
                 * lane of THIS wave (no independent thread scheduling on CDNA — an
                 * unbounded spin would deadlock the wave). A BOUNDED recheck drains the
                 * common race (claimer in another wave); if still unpublished, keep
                 * probing — worst case the row lands as a duplicate group, which partial
                 * aggregation permits. */
                uint32_t rdy = atomicAdd(&t_ready[s], 0u);
                if (rdy) {
                    __threadfence_block();
                    bool eq = t_null[s] == knull;
                    for (int k = 0; k < nk && eq; k++) eq = t_keys[k][s] == kb[k];
                    if (eq) {
                        slot = (int)s;
                        break;
                    }
                }
            }
            /* different group (or unpublished slot): keep probing */
        }
        }
        if (slot >= 0) {
            for (int g = 0; g < n_aggs; g++) {
                switch (agg_ops[g]) {
                case DD_AGG_SUM_F64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    if (c.valid && !c.valid[row]) break;
                    atomicAdd((double *)&t_agg[g][slot], ((const double *)c.data)[row]);
                    atomicAdd(&t_nn[g][slot], 1u);
                    break;
                }
                case DD_AGG_SUM_I64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    if (c.valid && !c.valid[row]) break;
                    atomicAdd(&t_agg[g][slot],
                              (unsigned long long)((const uint64_t *)c.data)[row]);
                    atomicAdd(&t_nn[g][slot], 1u);
                    break;
                }
                case DD_AGG_MIN_F64:
                case DD_AGG_MAX_F64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    if (c.valid && !c.valid[row]) break;
                    uint64_t k = dd_f64_key(((const double *)c.data)[row]);
                    if (agg_ops[g] == DD_AGG_MIN_F64)
                        atomicMin(&t_agg[g][slot], (unsigned long long)k);
                    else
                        atomicMax(&t_agg[g][slot], (unsigned long long)k);
                    atomicAdd(&t_nn[g][slot], 1u);
                    break;
                }
                case DD_AGG_MIN_I64:
                case DD_AGG_MAX_I64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    if (c.valid && !c.valid[row]) break;
                    uint64_t k = dd_i64_key(((const int64_t *)c.data)[row]);
                    if (agg_ops[g] == DD_AGG_MIN_I64)
                        atomicMin(&t_agg[g][slot], (unsigned long long)k);
                    else
                        atomicMax(&t_agg[g][slot], (unsigned long long)k);
                    atomicAdd(&t_nn[g][slot], 1u);
                    break;
                }
                case DD_AGG_COUNT:
                    atomicAdd(&t_agg[g][slot], 1ull);
                    atomicAdd(&t_nn[g][slot], 1u);
                    break;
                }
            }
        } else {
            /* spill: emit a singleton group */
            uint64_t o = atomicAdd((unsigned long long *)out_n, 1ull);
            for (int k = 0; k < nk; k++) out_keys[o * nk + k] = kb[k];
            out_keynull[o] = knull;
            for (int g = 0; g < n_aggs; g++) {
                double v = 0;
                uint64_t nn = 1;
                switch (agg_ops[g]) {
                case DD_AGG_SUM_F64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    const bool null = c.valid && !c.valid[row];
                    if (null) nn = 0;
                    v = null ? 0.0 : ((const double *)c.data)[row];
                    out_aggs[o * n_aggs + g] = v;
                    break;
                }
                case DD_AGG_MIN_F64:
                case DD_AGG_MAX_F64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    const bool null = c.valid && !c.valid[row];
                    if (null) nn = 0;
                    out_aggs[o * n_aggs + g] =
                        null ? dd_f64_unkey(dd_agg_identity(agg_ops[g]))
                             : ((const double *)c.data)[row];
                    break;
                }
                case DD_AGG_MIN_I64:
                case DD_AGG_MAX_I64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    const bool null = c.valid && !c.valid[row];
                    if (null) nn = 0;
                    out_aggs[o * n_aggs + g] = __longlong_as_double(
                        null ? dd_i64_unkey(dd_agg_identity(agg_ops[g]))
                             : ((const int64_t *)c.data)[row]);
                    break;
                }
                case DD_AGG_SUM_I64: {
                    const dd_kcol &c = a.cols[agg_cols[g]];
                    const bool null = c.valid && !c.valid[row];
                    if (null) nn = 0;
                    uint64_t iv = null ? 0 : ((const uint64_t *)c.data)[row];
                    out_aggs[o * n_aggs + g] = __longlong_as_double((long long)iv);
                    break;
                }
                case DD_AGG_COUNT:
                    out_aggs[o * n_aggs + g] = __longlong_as_double(1ll);
                    break;
                }
                out_nn[o * n_aggs + g] = nn;
            }
        }
    }
    __syncthreads();

    /* flush occupied slots */
    for (int s = threadIdx.x; s < R_CAP; s += R_THREADS) {
        if (t_hash[s] == 0) continue;
        uint64_t o = atomicAdd((unsigned long long *)out_n, 1ull);
        for (int k = 0; k < nk; k++) out_keys[o * nk + k] = t_keys[k][s];
        out_keynull[o] = t_null[s];
        for (int g = 0; g < n_aggs; g++) {
            unsigned long long st = t_agg[g][s];
            switch (agg_ops[g]) {
            case DD_AGG_MIN_F64:
            case DD_AGG_MAX_F64:
                out_aggs[o * n_aggs + g] = dd_f64_unkey(st);
                break;
            case DD_AGG_MIN_I64:
            case DD_AGG_MAX_I64:
                out_aggs[o * n_aggs + g] = __longlong_as_double(dd_i64_unkey(st));
                break;
            default:
                out_aggs[o * n_aggs + g] = __longlong_as_double((long long)st);
            }
            out_nn[o * n_aggs + g] = (uint64_t)t_nn[g][s];
        }
    }
}

extern "C" hipError_t dd_launch_partial_reduce(const dd_kargs *a, int64_t nblocks,
                                               int64_t chunk_rows, int n_aggs,
                                               const int32_t *agg_cols,
                                               const int32_t *agg_ops, uint64_t *out_keys,
                                               uint32_t *out_keynull, double *out_aggs,
                                               uint64_t *out_nn, uint64_t *out_n,
                                               hipStream_t s) {
    hipLaunchKernelGGL(k_partial_reduce, dim3((unsigned)nblocks), dim3(R_THREADS), 0, s, *a,
                       chunk_rows, n_aggs, agg_cols, agg_ops, out_keys, out_keynull,
                       out_aggs, out_nn, out_n);
    return hipGetLastError();
}

/* ---------------- k_partial_reduce_wide ----------------
 *
 * Up to DD_RW_MAX_AGGS aggregates and the exact decimal sum DD_AGG_SUM_DEC128. Same
 * claim / publish / bounded-probe / spill protocol as k_partial_reduce above; what
 * differs:
 *  - the table lives in dynamic LDS laid out for the plan at hand (arrays of table_slots
 *    entries: hash, keys[n_keys], state[n_aggs], high halves[n decimal sums], ready, null
 *    mask, nn[n_aggs]); table_slots is a power of two;
 *  - 1024-thread blocks: one table serves 16 waves;
 *  - every aggregate input is read BEFORE the probe, so the loads overlap it;
 *  - a decimal sum is two u64 LDS adds: old = add(lo, x.lo); add(hi, x.hi + carry) with
 *    carry = (old + x.lo) < old. The low adds are serialised by the atomic and each carry
 *    is a function of its own add's `old`, so after the block barrier (lo, hi) is the sum
 *    modulo 2^128 whatever the order;
 *  - WAVEAGG: lanes of a wave that found the same slot are reduced with cross-lane
 *    shuffles and one leader lane issues the atomics (rw_peel below).
 * Every per-aggregate loop is unrolled over DD_RW_MAX_AGGS with a g < n_aggs guard, so
 * the per-row value arrays stay in registers. */

#define RW_THREADS DD_RW_THREADS
#define RW_MAXA DD_RW_MAX_AGGS

/* one aggregate input as (lo, hi, non-null): min/max values already mapped to their
 * order-preserving u64 key; a NULL input reads as (0, 0, false) */
__device__ __forceinline__ bool rw_load(const dd_kargs &a, int op, int col, int64_t row,
                                        uint64_t &lo, uint64_t &hi) {
    lo = 0;
    hi = 0;
    if (op == DD_AGG_COUNT) {
        lo = 1;
        return true;
    }
    const dd_kcol &c = a.cols[col];
    if (c.valid && !c.valid[row]) return false;
    switch (op) {
    case DD_AGG_SUM_DEC128: {
        const dd_u128 v = ((const dd_u128 *)c.data)[row];
        lo = v.x;
        hi = v.y;
        break;
    }
    case DD_AGG_MIN_F64:
    case DD_AGG_MAX_F64:
        lo = dd_f64_key(((const double *)c.data)[row]);
        break;
    case DD_AGG_MIN_I64:
    case DD_AGG_MAX_I64:
        lo = dd_i64_key(((const int64_t *)c.data)[row]);
        break;
    default: /* SUM_F64 / SUM_I64: the raw 8 bytes */
        lo = ((const uint64_t *)c.data)[row];
    }
    return true;
}

/* fold (lo, hi) standing for nn non-null inputs into one slot's state */
__device__ __forceinline__ void rw_apply(int op, unsigned long long *p_lo,
                                         unsigned long long *p_hi, uint32_t *p_nn,
                                         uint64_t lo, uint64_t hi, uint32_t nn) {
    switch (op) {
    case DD_AGG_SUM_F64:
        atomicAdd((double *)p_lo, __longlong_as_double((long long)lo));
        break;
    case DD_AGG_MIN_F64:
    case DD_AGG_MIN_I64:
        atomicMin(p_lo, (unsigned long long)lo);
        break;
    case DD_AGG_MAX_F64:
    case DD_AGG_MAX_I64:
        atomicMax(p_lo, (unsigned long long)lo);
        break;
    case DD_AGG_SUM_DEC128: {
        const uint64_t old = atomicAdd(p_lo, (unsigned long long)lo);
        const uint64_t up = hi + (uint64_t)((old + lo) < old);
        if (up) atomicAdd(p_hi, (unsigned long long)up); /* adding 0 changes nothing */
        break;
    }
    default: /* COUNT / SUM_I64 */
        atomicAdd(p_lo, (unsigned long long)lo);
    }
    atomicAdd(p_nn, nn);
}

__device__ __forceinline__ uint64_t rw_xor64(uint64_t v, int off) {
    return (uint64_t)__shfl_xor((unsigned long long)v, off, RWAVE);
}

/* the value slot of an output row: min/max keys mapped back, everything else as is */
__device__ __forceinline__ uint64_t rw_out_bits(int op, uint64_t st) {
    switch (op) {
    case DD_AGG_MIN_F64:
    case DD_AGG_MAX_F64:
        return (uint64_t)__double_as_longlong(dd_f64_unkey(st));
    case DD_AGG_MIN_I64:
    case DD_AGG_MAX_I64:
        return (uint64_t)dd_i64_unkey(st);
    default:
        return st;
    }
}

template <bool WAVEAGG>
__global__ __launch_bounds__(RW_THREADS) void k_partial_reduce_wide(
    dd_kargs a, int64_t chunk_rows, int n_aggs, int table_slots, int probe_limit,
    const int32_t *agg_cols /* [RW_MAXA] */, const int32_t *agg_ops /* [RW_MAXA] */,
    uint64_t *out_keys /* [max_rows][n_keys] */, uint32_t *out_keynull /* [max_rows] */,
    uint64_t *out_aggs /* [max_rows][n_aggs] low 64 bits / f64 bits */,
    uint64_t *out_hi /* [max_rows][n_aggs] high 64 bits of a decimal sum, else 0 */,
    uint64_t *out_nn /* [max_rows][n_aggs] */, uint64_t *out_n) {
    extern __shared__ __align__(16) unsigned long long rw_lds[];

    const int S = table_slots;
    const uint32_t smask = (uint32_t)S - 1u;
    const int nk = a.n_keys > 4 ? 4 : a.n_keys;

    /* the plan, wave-uniform: op / column / index of the high-half array per aggregate */
    int ops[RW_MAXA], cols[RW_MAXA], hix[RW_MAXA];
    int n_dec = 0;
#pragma unroll
    for (int g = 0; g < RW_MAXA; g++) {
        ops[g] = g < n_aggs ? agg_ops[g] : -1;
        cols[g] = g < n_aggs ? agg_cols[g] : 0;
        hix[g] = n_dec;
        if (ops[g] == DD_AGG_SUM_DEC128) n_dec++;
    }

    unsigned long long *t_hash = rw_lds;
    unsigned long long *t_keys = t_hash + S;                 /* [nk][S] */
    unsigned long long *t_agg = t_keys + (size_t)nk * S;     /* [n_aggs][S] */
    unsigned long long *t_hi = t_agg + (size_t)n_aggs * S;   /* [n_dec][S] */
    uint32_t *t_ready = (uint32_t *)(t_hi + (size_t)n_dec * S);
    uint32_t *t_null = t_ready + S;
    uint32_t *t_nn = t_null + S;                             /* [n_aggs][S] */

    for (int s = threadIdx.x; s < S; s += RW_THREADS) {
        t_hash[s] = 0;
        t_ready[s] = 0;
        t_null[s] = 0;
        for (int k = 0; k < nk; k++) t_keys[k * S + s] = 0;
#pragma unroll
        for (int g = 0; g < RW_MAXA; g++) {
            if (g >= n_aggs) break;
            t_agg[g * S + s] = dd_agg_identity(ops[g]);
            t_nn[g * S + s] = 0;
            if (ops[g] == DD_AGG_SUM_DEC128) t_hi[hix[g] * S + s] = 0;
        }
    }
    __syncthreads();

    const int64_t start = (int64_t)blockIdx.x * chunk_rows;
    const int64_t end = (start + chunk_rows < a.n_rows) ? (start + chunk_rows) : a.n_rows;
    const int lane = threadIdx.x & (RWAVE - 1);

    /* the trip count is uniform over the block (a lane past `end` idles), so the
     * cross-lane steps below always run with whole waves */
    for (int64_t base = start; base < end; base += RW_THREADS) {
        const int64_t row = base + threadIdx.x;
        const bool active = row < end;
        uint64_t vlo[RW_MAXA], vhi[RW_MAXA];
        uint32_t vok = 0;
        uint64_t kb[4] = {0, 0, 0, 0};
        uint32_t knull = 0;
        int slot = -1;
#pragma unroll
        for (int g = 0; g < RW_MAXA; g++) {
            vlo[g] = 0;
            vhi[g] = 0;
        }
        if (active) {
            /* values first: their loads are in flight while the probe runs */
#pragma unroll
            for (int g = 0; g < RW_MAXA; g++) {
                if (g >= n_aggs) break;
                if (rw_load(a, ops[g], cols[g], row, vlo[g], vhi[g])) vok |= 1u << g;
            }
            uint64_t h = dd_row_hash<false>(a, row); /* host refuses dec128 keys */
            if (h == 0) h = 1; /* 0 is the empty sentinel */
            for (int k = 0; k < nk; k++) {
                const dd_kcol &c = a.cols[a.key_idx[k]];
                const bool isnull = c.valid && !c.valid[row];
                if (isnull) knull |= 1u << k;
                kb[k] = isnull ? 0 : dd_key_bits(c, row);
            }
            /* two probe attempts, as in k_partial_reduce: attempt 1 claims or matches at
             * the home slot only; after its loop reconverges every publish of this wave
             * is visible, so attempt 2 matches instead of claiming a duplicate per lane.
             * A claim is never waited on: an unpublished slot is walked past. */
            for (int attempt = 0; attempt < 2 && slot < 0; attempt++) {
                uint32_t s = (uint32_t)h & smask;
                for (int probe = 0; probe < probe_limit; probe++, s = (s + 1) & smask) {
                    if (attempt == 0 && probe > 0) break;
                    uint64_t cur = atomicCAS(&t_hash[s], 0ull, (unsigned long long)h);
                    if (cur == 0) { /* claimed: publish keys, then ready */
                        for (int k = 0; k < nk; k++) t_keys[k * S + s] = kb[k];
                        t_null[s] = knull;
                        __threadfence_block();
                        atomicExch(&t_ready[s], 1u);
                        slot = (int)s;
                        break;
                    }
                    if (cur == h) {
                        uint32_t rdy = atomicAdd(&t_ready[s], 0u);
                        if (rdy) {
                            __threadfence_block();
                            bool eq = t_null[s] == knull;
                            for (int k = 0; k < nk && eq; k++) eq = t_keys[k * S + s] == kb[k];
                            if (eq) {
                                slot = (int)s;
                                break;
                            }
                        }
                    }
                }
            }
        }

        bool pending = active && slot >= 0;
        if (WAVEAGG) {
            /* peel slot groups off the wave while they are worth a reduce: the first
             * pending lane names a slot, the lanes that hold it are reduced over the
             * whole wave (other lanes feed the op's identity) and the first lane issues
             * the atomics. The first group below DD_RW_PEEL_MIN lanes ends the peeling;
             * whatever is still pending goes per lane below. */
            for (;;) {
                const unsigned long long pm = __ballot(pending);
                if (!pm) break;
                const int first = __ffsll((long long)pm) - 1;
                const int s0 = __shfl(slot, first, RWAVE);
                const bool inm = pending && slot == s0;
                const unsigned long long m = __ballot(inm);
                if (__popcll(m) < DD_RW_PEEL_MIN) break;
#pragma unroll
                for (int g = 0; g < RW_MAXA; g++) {
                    if (g >= n_aggs) break;
                    const bool in = inm && ((vok >> g) & 1u);
                    const uint32_t nn = (uint32_t)__popcll(__ballot(in));
                    if (nn == 0) continue; /* uniform: every input of the group is NULL */
                    uint64_t lo = in ? vlo[g] : dd_agg_identity(ops[g]);
                    uint64_t hi = 0;
                    switch (ops[g]) {
                    case DD_AGG_COUNT:
                        lo = nn;
                        break;
                    case DD_AGG_SUM_I64:
                        for (int off = RWAVE / 2; off > 0; off >>= 1) lo += rw_xor64(lo, off);
                        break;
                    case DD_AGG_SUM_F64:
                        for (int off = RWAVE / 2; off > 0; off >>= 1) {
                            const double o = __longlong_as_double((long long)rw_xor64(lo, off));
                            lo = (uint64_t)__double_as_longlong(
                                __longlong_as_double((long long)lo) + o);
                        }
                        break;
                    case DD_AGG_MIN_F64:
                    case DD_AGG_MIN_I64:
                        for (int off = RWAVE / 2; off > 0; off >>= 1) {
                            const uint64_t o = rw_xor64(lo, off);
                            lo = o < lo ? o : lo;
                        }
                        break;
                    case DD_AGG_MAX_F64:
                    case DD_AGG_MAX_I64:
                        for (int off = RWAVE / 2; off > 0; off >>= 1) {
                            const uint64_t o = rw_xor64(lo, off);
                            lo = o > lo ? o : lo;
                        }
                        break;
                    case DD_AGG_SUM_DEC128:
                        hi = in ? vhi[g] : 0;
                        for (int off = RWAVE / 2; off > 0; off >>= 1) {
                            const uint64_t olo = rw_xor64(lo, off);
                            const uint64_t ohi = rw_xor64(hi, off);
                            const uint64_t sum = lo + olo;
                            hi = hi + ohi + (uint64_t)(sum < lo); /* carry into the high half */
                            lo = sum;
                        }
                        break;
                    }
                    if (lane == first)
                        rw_apply(ops[g], &t_agg[g * S + s0], &t_hi[hix[g] * S + s0],
                                 &t_nn[g * S + s0], lo, hi, nn);
                }
                pending = pending && slot != s0;
            }
        }
        if (pending) {
#pragma unroll
            for (int g = 0; g < RW_MAXA; g++) {
                if (g >= n_aggs) break;
                if (!((vok >> g) & 1u)) continue;
                rw_apply(ops[g], &t_agg[g * S + slot], &t_hi[hix[g] * S + slot],
                         &t_nn[g * S + slot], vlo[g], vhi[g], 1u);
            }
        } else if (active && slot < 0) {
            /* spill: a singleton group carrying the row's full value in (lo, hi) */
            const uint64_t o = atomicAdd((unsigned long long *)out_n, 1ull);
            for (int k = 0; k < nk; k++) out_keys[o * nk + k] = kb[k];
            out_keynull[o] = knull;
#pragma unroll
            for (int g = 0; g < RW_MAXA; g++) {
                if (g >= n_aggs) break;
                const bool ok = (vok >> g) & 1u;
                out_aggs[o * n_aggs + g] =
                    rw_out_bits(ops[g], ok ? vlo[g] : dd_agg_identity(ops[g]));
                out_hi[o * n_aggs + g] = vhi[g];
                out_nn[o * n_aggs + g] = ok ? 1u : 0u;
            }
        }
    }
    __syncthreads();

    /* flush occupied slots */
    for (int s = threadIdx.x; s < S; s += RW_THREADS) {
        if (t_hash[s] == 0) continue;
        const uint64_t o = atomicAdd((unsigned long long *)out_n, 1ull);
        for (int k = 0; k < nk; k++) out_keys[o * nk + k] = t_keys[k * S + s];
        out_keynull[o] = t_null[s];
#pragma unroll
        for (int g = 0; g < RW_MAXA; g++) {
            if (g >= n_aggs) break;
            out_aggs[o * n_aggs + g] = rw_out_bits(ops[g], t_agg[g * S + s]);
            out_hi[o * n_aggs + g] =
                ops[g] == DD_AGG_SUM_DEC128 ? t_hi[hix[g] * S + s] : 0ull;
            out_nn[o * n_aggs + g] = (uint64_t)t_nn[g * S + s];
        }
    }
}

extern "C" hipError_t dd_launch_partial_reduce_wide(
    const dd_kargs *a, int waveagg, int64_t nblocks, int64_t chunk_rows, int n_aggs,
    int table_slots, int probe_limit, size_t lds_bytes, const int32_t *agg_cols,
    const int32_t *agg_ops, uint64_t *out_keys, uint32_t *out_keynull, uint64_t *out_aggs,
    uint64_t *out_hi, uint64_t *out_nn, uint64_t *out_n, hipStream_t s) {
    auto kern = waveagg ? k_partial_reduce_wide<true> : k_partial_reduce_wide<false>;
    if (lds_bytes > 65536) { /* past 64 KiB dynamic LDS is opt-in per function */
        hipError_t e = hipFuncSetAttribute((const void *)kern,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(RW_THREADS), lds_bytes, s, *a,
                       chunk_rows, n_aggs, table_slots, probe_limit, agg_cols, agg_ops,
                       out_keys, out_keynull, out_aggs, out_hi, out_nn, out_n);
    return hipGetLastError();
}
