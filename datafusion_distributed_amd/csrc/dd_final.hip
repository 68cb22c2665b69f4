/* dd_final.hip — GPU final aggregation above the shuffle.
 *
 * The AggregateExec mode=FinalPartitioned that sits on RepartitionExec Hash(keys, P) in the
 * q1 plan (tests/tpch_plans_test.rs): rows of partial states, already routed to their
 * partitions, are merged to one row per (partition, group). Input: a device batch plus a
 * segment layout (seg_offsets / seg_part) that says which rows form which partition.
 *
 * No kernel here waits on another lane. The claim table holds ROW IDS into the immutable
 * input, so a slot is usable the moment its CAS lands: whoever reads a row id compares its
 * own key against that row's input columns; nothing is published behind a flag.
 *
 *   k_final_claim   per row: segment -> partition -> table region; probe from the home slot
 *                   dd_mix64(row hash) >> (64 - log2(region slots)); claim with one CAS or
 *                   match against the resident row; row_slot[row] = slot.
 *   k_final_scan_*  exclusive scan of "slot occupied" over the table: slot_gid, and the
 *                   group offset of each partition (its region's first slot).
 *   k_final_init / k_final_merge / k_final_finish
 *                   state sized by n_groups: identities, then per-row global atomics into
 *                   out[gid] (the representative row also writes the keys), then the
 *                   min / max keys mapped back to value bits and COUNT's nn filled in.
 *
 * A region holds max(64, next_pow2(2 * rows)) slots, so its load never passes 0.5 and a
 * linear probe always meets an empty slot; the probe loop is bounded by the region size all
 * the same and reports through `err` instead of walking on. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_agg_device.h"
#include "dd_hash_device.h"
#include "dd_internal.h"

#define F_THREADS DD_F_THREADS
#define F_WAVE 64
#define F_MAXA DD_F_MAX_AGGS
#define F_MAXK 4
#define F_EMPTY DD_F_EMPTY

/* ---------------- claim ---------------- */

/* does input row `other` carry the group identity (kb, knull)? */
__device__ __forceinline__ bool f_same_group(const dd_kargs &a, int nk, int64_t other,
                                             const uint64_t (&kb)[F_MAXK], uint32_t knull) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < F_MAXK; k++) {
        if (k >= nk) break;
        const dd_kcol &c = a.cols[a.key_idx[k]];
        const bool isnull = c.valid && !c.valid[other];
        const uint64_t bits = isnull ? 0 : dd_key_bits(c, other);
        eq = eq && isnull == (bool)((knull >> k) & 1u) && bits == kb[k];
    }
    return eq;
}

template <bool STAGED>
__global__ __launch_bounds__(F_THREADS) void k_final_claim(
    dd_kargs a, const int64_t *seg_offsets /* [n_segs + 1] */,
    const int32_t *seg_part /* [n_segs] */, int32_t n_segs,
    const uint32_t *part_base /* [n_parts] first slot of the region */,
    const uint32_t *part_log2 /* [n_parts] log2(region slots) */, uint32_t *table,
    uint32_t *row_slot /* [n_rows] */, uint32_t *err) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    if (STAGED) {
        for (int i = threadIdx.x; i <= n_segs; i += F_THREADS) s_off[i] = seg_offsets[i];
        __syncthreads();
    }
    const int nk = a.n_keys > F_MAXK ? F_MAXK : a.n_keys;
    const int64_t start = (int64_t)blockIdx.x * DD_F_BLOCK_ROWS;
    const int64_t end = start + DD_F_BLOCK_ROWS < a.n_rows ? start + DD_F_BLOCK_ROWS : a.n_rows;

    for (int64_t row = start + threadIdx.x; row < end; row += F_THREADS) {
        /* the segment s with seg_offsets[s] <= row < seg_offsets[s + 1]: the smallest s
         * whose END lies past the row (empty segments are stepped over);
         * seg_offsets[n_segs] == n_rows > row bounds the search */
        int lo = 0, hi = n_segs - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int64_t e = STAGED ? s_off[mid + 1] : seg_offsets[mid + 1];
            if (e > row) hi = mid;
            else lo = mid + 1;
        }
        const int32_t p = seg_part[lo];
        const uint32_t base = part_base[p];
        const uint32_t lg = part_log2[p];
        const uint32_t mask = (1u << lg) - 1u;

        const uint64_t h = dd_row_hash<false>(a, row); /* host refuses dec128 keys */
        uint64_t kb[F_MAXK] = {0, 0, 0, 0};
        uint32_t knull = 0;
#pragma unroll
        for (int k = 0; k < F_MAXK; k++) {
            if (k >= nk) break;
            const dd_kcol &c = a.cols[a.key_idx[k]];
            const bool isnull = c.valid && !c.valid[row];
            if (isnull) knull |= 1u << k;
            kb[k] = isnull ? 0 : dd_key_bits(c, row);
        }
        /* home slot: the HIGH bits of a remix. Every row of a shuffled partition shares
         * h % P_total, so low bits of h would pile the partition onto a few slots */
        uint32_t s = (uint32_t)(dd_mix64(h) >> (64 - lg));
        uint32_t found = F_EMPTY;
        for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
            uint32_t *t = table + ((size_t)base + s);
            /* a slot goes EMPTY -> row id once and never changes again: a non-EMPTY read
             * is final, an EMPTY read is settled by the CAS */
            uint32_t cur = __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == F_EMPTY) {
                cur = atomicCAS(t, F_EMPTY, (uint32_t)row);
                if (cur == F_EMPTY) { /* this row represents the group */
                    found = base + s;
                    break;
                }
            }
            if (f_same_group(a, nk, (int64_t)cur, kb, knull)) {
                found = base + s;
                break;
            }
        }
        if (found == F_EMPTY) atomicOr(err, 1u); /* unreachable at load <= 0.5 */
        row_slot[row] = found;
    }
}

extern "C" hipError_t dd_launch_final_claim(const dd_kargs *a, const int64_t *seg_offsets,
                                            const int32_t *seg_part, int32_t n_segs,
                                            const uint32_t *part_base,
                                            const uint32_t *part_log2, uint32_t *table,
                                            uint32_t *row_slot, uint32_t *err,
                                            hipStream_t s) {
    const int64_t nblocks = (a->n_rows + DD_F_BLOCK_ROWS - 1) / DD_F_BLOCK_ROWS;
    if (nblocks == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_final_claim<true>, dim3((unsigned)nblocks), dim3(F_THREADS), 0,
                           s, *a, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           row_slot, err);
    else
        hipLaunchKernelGGL(k_final_claim<false>, dim3((unsigned)nblocks), dim3(F_THREADS), 0,
                           s, *a, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           row_slot, err);
    return hipGetLastError();
}

/* ---------------- group ids: exclusive scan of "occupied" over the table ----------------
 * Three passes, none of which looks back at a running neighbour: per-tile counts, one
 * block that scans the tile counts, per-tile ranks on top of the tile's base. */

/* exclusive scan of c over the block's T threads (T / 64 waves); total = block sum.
 * s_w: T / 64 words of LDS, free on entry */
template <int T>
__device__ __forceinline__ uint32_t f_block_excl(uint32_t c, uint32_t *s_w, uint32_t &total) {
    const int lane = threadIdx.x & (F_WAVE - 1), w = threadIdx.x / F_WAVE;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < F_WAVE; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, F_WAVE);
        if (lane >= off) inc += o;
    }
    if (lane == F_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < T / F_WAVE; i++) {
        const uint32_t v = s_w[i];
        if (i < w) wbase += v;
        total += v;
    }
    return wbase + inc - c;
}

/* the four table entries of this thread (n_slots is a multiple of 4) */
__device__ __forceinline__ uint4 f_tile_load(const uint32_t *table, uint64_t n_slots,
                                             uint64_t i) {
    if (i < n_slots) return *(const uint4 *)(table + i);
    return make_uint4(F_EMPTY, F_EMPTY, F_EMPTY, F_EMPTY);
}

__global__ __launch_bounds__(F_THREADS) void k_final_scan_count(const uint32_t *table,
                                                                uint64_t n_slots,
                                                                uint32_t *block_sums) {
    __shared__ uint32_t s_w[F_THREADS / F_WAVE];
    const uint64_t i = (uint64_t)blockIdx.x * DD_F_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = f_tile_load(table, n_slots, i);
    const uint32_t c = (v.x != F_EMPTY) + (v.y != F_EMPTY) + (v.z != F_EMPTY) + (v.w != F_EMPTY);
    uint32_t total;
    (void)f_block_excl<F_THREADS>(c, s_w, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

#define F_SUMS_THREADS 1024
/* in place: sums[i] = sum of sums[0 .. i), sums[nb] = the total (the group count) */
__global__ __launch_bounds__(F_SUMS_THREADS) void k_final_scan_sums(uint32_t *sums,
                                                                    uint32_t nb) {
    __shared__ uint32_t s_w[F_SUMS_THREADS / F_WAVE];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += F_SUMS_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t c = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = f_block_excl<F_SUMS_THREADS>(c, s_w, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
        __syncthreads(); /* s_w is reused by the next round */
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}

/* slot_gid[s] = occupied slots before s (for an occupied slot: its group id) */
__global__ __launch_bounds__(F_THREADS) void k_final_scan_write(const uint32_t *table,
                                                                uint64_t n_slots,
                                                                const uint32_t *block_sums,
                                                                uint32_t *slot_gid) {
    __shared__ uint32_t s_w[F_THREADS / F_WAVE];
    const uint64_t i = (uint64_t)blockIdx.x * DD_F_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = f_tile_load(table, n_slots, i);
    const uint32_t c0 = v.x != F_EMPTY, c1 = v.y != F_EMPTY, c2 = v.z != F_EMPTY,
                   c3 = v.w != F_EMPTY;
    uint32_t total;
    const uint32_t ex = block_sums[blockIdx.x] + f_block_excl<F_THREADS>(c0 + c1 + c2 + c3,
                                                                        s_w, total);
    if (i < n_slots)
        *(uint4 *)(slot_gid + i) = make_uint4(ex, ex + c0, ex + c0 + c1, ex + c0 + c1 + c2);
}

/* group_offsets[p] = group id of partition p's first slot; [n_parts] = the group count */
__global__ void k_final_group_offsets(const uint32_t *slot_gid, const uint32_t *part_base,
                                      const uint32_t *block_sums, uint32_t nb,
                                      int32_t n_parts, int64_t *group_offsets) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_parts) group_offsets[p] = (int64_t)slot_gid[part_base[p]];
    else if (p == n_parts) group_offsets[p] = (int64_t)block_sums[nb];
}

extern "C" hipError_t dd_launch_final_scan(const uint32_t *table, uint64_t n_slots,
                                           uint32_t *block_sums, uint32_t *slot_gid,
                                           const uint32_t *part_base, int32_t n_parts,
                                           int64_t *group_offsets, hipStream_t s) {
    const uint32_t nb = (uint32_t)((n_slots + DD_F_SCAN_TILE - 1) / DD_F_SCAN_TILE);
    hipLaunchKernelGGL(k_final_scan_count, dim3(nb), dim3(F_THREADS), 0, s, table, n_slots,
                       block_sums);
    hipLaunchKernelGGL(k_final_scan_sums, dim3(1), dim3(F_SUMS_THREADS), 0, s, block_sums, nb);
    hipLaunchKernelGGL(k_final_scan_write, dim3(nb), dim3(F_THREADS), 0, s, table, n_slots,
                       block_sums, slot_gid);
    hipLaunchKernelGGL(k_final_group_offsets, dim3((unsigned)(n_parts / 256 + 1)), dim3(256),
                       0, s, slot_gid, part_base, block_sums, nb, n_parts, group_offsets);
    return hipGetLastError();
}

/* ---------------- merge ---------------- */

__global__ __launch_bounds__(F_THREADS) void k_final_init(dd_final_plan plan, int64_t n_groups,
                                                          uint64_t *out_aggs, uint64_t *out_hi,
                                                          uint64_t *out_nn) {
    const int64_t g = (int64_t)blockIdx.x * F_THREADS + threadIdx.x;
    if (g >= n_groups) return;
    const int na = plan.n_aggs;
#pragma unroll
    for (int j = 0; j < F_MAXA; j++) {
        if (j >= na) break;
        out_aggs[g * na + j] = dd_agg_identity(plan.ops[j]);
        out_hi[g * na + j] = 0;
        out_nn[g * na + j] = 0;
    }
}

__global__ __launch_bounds__(F_THREADS) void k_final_merge(
    dd_kargs a, dd_final_plan plan, const uint32_t *table, const uint32_t *row_slot,
    const uint32_t *slot_gid, uint64_t *out_keys /* [n_groups][n_keys] */,
    uint32_t *out_keynull /* [n_groups] */, uint64_t *out_aggs /* [n_groups][n_aggs] */,
    uint64_t *out_hi, uint64_t *out_nn) {
    const int64_t row = (int64_t)blockIdx.x * F_THREADS + threadIdx.x;
    if (row >= a.n_rows) return;
    const int nk = a.n_keys > F_MAXK ? F_MAXK : a.n_keys;
    const int na = plan.n_aggs;

    /* every load of the row first, the atomics after them */
    const uint32_t slot = row_slot[row];
    uint64_t lo[F_MAXA], hi[F_MAXA], nn[F_MAXA];
#pragma unroll
    for (int j = 0; j < F_MAXA; j++) {
        lo[j] = hi[j] = nn[j] = 0;
        if (j >= na) continue;
        const dd_kcol &c = a.cols[plan.state_cols[j]];
        if (plan.ops[j] == DD_AGG_SUM_DEC128) {
            const dd_u128 v = ((const dd_u128 *)c.data)[row];
            lo[j] = v.x;
            hi[j] = v.y;
        } else {
            lo[j] = ((const uint64_t *)c.data)[row];
        }
        /* COUNT: nn is the merged count itself */
        nn[j] = plan.ops[j] == DD_AGG_COUNT
                    ? lo[j]
                    : ((const uint64_t *)a.cols[plan.nn_cols[j]].data)[row];
    }
    const uint32_t gid = slot_gid[slot];
    const bool rep = table[slot] == (uint32_t)row;
    if (rep) { /* the claim's winner carries the group's identity out */
        uint32_t knull = 0;
#pragma unroll
        for (int k = 0; k < F_MAXK; k++) {
            if (k >= nk) break;
            const dd_kcol &c = a.cols[a.key_idx[k]];
            const bool isnull = c.valid && !c.valid[row];
            if (isnull) knull |= 1u << k;
            out_keys[(size_t)gid * nk + k] = isnull ? 0 : dd_key_bits(c, row);
        }
        out_keynull[gid] = knull;
    }
#pragma unroll
    for (int j = 0; j < F_MAXA; j++) {
        if (j >= na) break;
        if (nn[j] == 0) continue; /* a partial without a non-null input: value never used */
        unsigned long long *p = (unsigned long long *)&out_aggs[(size_t)gid * na + j];
        switch (plan.ops[j]) {
        case DD_AGG_SUM_F64:
            (void)unsafeAtomicAdd((double *)p, __longlong_as_double((long long)lo[j]));
            break;
        case DD_AGG_MIN_F64:
            atomicMin(p, (unsigned long long)dd_f64_key(__longlong_as_double((long long)lo[j])));
            break;
        case DD_AGG_MAX_F64:
            atomicMax(p, (unsigned long long)dd_f64_key(__longlong_as_double((long long)lo[j])));
            break;
        case DD_AGG_MIN_I64:
            atomicMin(p, (unsigned long long)dd_i64_key((int64_t)lo[j]));
            break;
        case DD_AGG_MAX_I64:
            atomicMax(p, (unsigned long long)dd_i64_key((int64_t)lo[j]));
            break;
        case DD_AGG_SUM_DEC128: {
            /* §17.2: the low adds are serialised by the atomic and each carry is a function
             * of its own add's `old`, so (lo, hi) ends as the sum modulo 2^128 */
            const uint64_t old = atomicAdd(p, (unsigned long long)lo[j]);
            const uint64_t up = hi[j] + (uint64_t)((old + lo[j]) < old);
            if (up)
                atomicAdd((unsigned long long *)&out_hi[(size_t)gid * na + j],
                          (unsigned long long)up);
            break;
        }
        case DD_AGG_COUNT: /* its nn is the merged count: k_final_finish copies it over */
            atomicAdd(p, (unsigned long long)lo[j]);
            continue;
        default: /* SUM_I64 */
            atomicAdd(p, (unsigned long long)lo[j]);
        }
        atomicAdd((unsigned long long *)&out_nn[(size_t)gid * na + j],
                  (unsigned long long)nn[j]);
    }
}

/* min / max: order-preserving key -> value bits; COUNT: nn = the merged count */
__global__ __launch_bounds__(F_THREADS) void k_final_finish(dd_final_plan plan,
                                                            int64_t n_groups,
                                                            uint64_t *out_aggs,
                                                            uint64_t *out_nn) {
    const int64_t g = (int64_t)blockIdx.x * F_THREADS + threadIdx.x;
    if (g >= n_groups) return;
    const int na = plan.n_aggs;
#pragma unroll
    for (int j = 0; j < F_MAXA; j++) {
        if (j >= na) break;
        const int op = plan.ops[j];
        if (op == DD_AGG_MIN_F64 || op == DD_AGG_MAX_F64)
            out_aggs[g * na + j] =
                (uint64_t)__double_as_longlong(dd_f64_unkey(out_aggs[g * na + j]));
        else if (op == DD_AGG_MIN_I64 || op == DD_AGG_MAX_I64)
            out_aggs[g * na + j] = (uint64_t)dd_i64_unkey(out_aggs[g * na + j]);
        else if (op == DD_AGG_COUNT)
            out_nn[g * na + j] = out_aggs[g * na + j];
    }
}

extern "C" hipError_t dd_launch_final_merge(const dd_kargs *a, const dd_final_plan *plan,
                                            const uint32_t *table, const uint32_t *row_slot,
                                            const uint32_t *slot_gid, int64_t n_groups,
                                            uint64_t *out_keys, uint32_t *out_keynull,
                                            uint64_t *out_aggs, uint64_t *out_hi,
                                            uint64_t *out_nn, hipStream_t s) {
    if (n_groups == 0) return hipSuccess;
    const unsigned gb = (unsigned)((n_groups + F_THREADS - 1) / F_THREADS);
    const unsigned rb = (unsigned)((a->n_rows + F_THREADS - 1) / F_THREADS);
    hipLaunchKernelGGL(k_final_init, dim3(gb), dim3(F_THREADS), 0, s, *plan, n_groups, out_aggs,
                       out_hi, out_nn);
    hipLaunchKernelGGL(k_final_merge, dim3(rb), dim3(F_THREADS), 0, s, *a, *plan, table,
                       row_slot, slot_gid, out_keys, out_keynull, out_aggs, out_hi, out_nn);
    bool finish = false; /* a plan of sums alone has nothing to map back */
    for (int j = 0; j < plan->n_aggs; j++)
        finish = finish || plan->ops[j] == DD_AGG_COUNT ||
                 (plan->ops[j] >= DD_AGG_MIN_F64 && plan->ops[j] <= DD_AGG_MAX_I64);
    if (finish)
        hipLaunchKernelGGL(k_final_finish, dim3(gb), dim3(F_THREADS), 0, s, *plan, n_groups,
                           out_aggs, out_nn);
    return hipGetLastError();
}

/* ---------------- typed device columns for a further operator ----------
 * The interleaved state of a finished merge, one thread per group, as columns: each key in its
 * input dtype from the canonical key bits (a float key therefore comes out canonicalised: +0.0
 * for -0.0, one quiet NaN) with validity from keynull; one column per aggregate (i64, f64, or
 * dec128 from (lo, hi)) with validity nn != 0; optionally nn itself as i64. */
__global__ __launch_bounds__(F_THREADS) void k_final_columns(
    dd_final_cols c, int64_t n_groups, const uint64_t *keys, const uint32_t *keynull,
    const uint64_t *aggs, const uint64_t *hi, const uint64_t *nn) {
    const int64_t g = (int64_t)blockIdx.x * F_THREADS + threadIdx.x;
    if (g >= n_groups) return;
    const int nk = c.n_keys, na = c.n_aggs;
    const uint32_t knull = keynull[g];
#pragma unroll
    for (int k = 0; k < F_MAXK; k++) {
        if (k >= nk) break;
        const uint64_t b = keys[(size_t)g * nk + k];
        switch (c.key_dtype[k]) { /* wave-uniform */
        case DD_KDT_U8:
        case DD_KDT_BOOL: ((uint8_t *)c.key_data[k])[g] = (uint8_t)b; break;
        case DD_KDT_I16: ((uint16_t *)c.key_data[k])[g] = (uint16_t)b; break;
        case DD_KDT_I32:
        case DD_KDT_F32: ((uint32_t *)c.key_data[k])[g] = (uint32_t)b; break;
        default: ((uint64_t *)c.key_data[k])[g] = b; /* i64, f64 */
        }
        c.key_valid[k][g] = (uint8_t)(((knull >> k) & 1u) == 0);
    }
#pragma unroll
    for (int j = 0; j < F_MAXA; j++) {
        if (j >= na) break;
        const uint64_t lo = aggs[(size_t)g * na + j], cnt = nn[(size_t)g * na + j];
        if (c.ops[j] == DD_AGG_SUM_DEC128)
            ((dd_u128 *)c.agg_data[j])[g] = dd_u128{lo, hi[(size_t)g * na + j]};
        else
            ((uint64_t *)c.agg_data[j])[g] = lo;
        if (c.agg_valid[j]) c.agg_valid[j][g] = (uint8_t)(cnt != 0);
        if (c.nn_data[j]) c.nn_data[j][g] = (int64_t)cnt;
    }
}

extern "C" hipError_t dd_launch_final_columns(const dd_final_cols *c, int64_t n_groups,
                                              const uint64_t *keys, const uint32_t *keynull,
                                              const uint64_t *aggs, const uint64_t *hi,
                                              const uint64_t *nn, hipStream_t s) {
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(k_final_columns, dim3((unsigned)((n_groups + F_THREADS - 1) / F_THREADS)),
                       dim3(F_THREADS), 0, s, *c, n_groups, keys, keynull, aggs, hi, nn);
    return hipGetLastError();
}
