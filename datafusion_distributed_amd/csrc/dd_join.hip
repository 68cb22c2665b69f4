/* dd_join.hip — GPU partitioned hash join above two co-partitioned shuffles.
 *
 * The HashJoinExec mode=Partitioned that sits on two RepartitionExec Hash(keys, P) inputs in
 * the reference's plans (tests/join.rs, tests/tpch_plans_test.rs). Two device batches, each
 * with a segment layout (seg_offsets / seg_part); partition p of the build side joins
 * partition p of the probe side and nothing else.
 *
 * As in dd_final.hip no kernel waits on another lane: the table holds ROW IDS into the
 * immutable build batch, duplicates hang behind the head of their key in `next`, and nobody
 * reads a chain before the kernel that built it has ended.
 *
 *   k_join_build        per build row: segment -> partition -> region; claim the home slot
 *                       chain by CAS, or link behind the resident row of an equal key.
 *   k_join_count        per probe row: probe the now-immutable table with plain loads, walk
 *                       the chain: cnt[row] (inner, right_*) or matched[build row] (left_*).
 *   k_join_left_cnt     left_*: cnt over build rows from matched.
 *   k_join_scan_*       exclusive scan of cnt in place, 64-bit throughout, so the total is
 *                       exact before the host range-checks it.
 *   k_join_seg_out      output seg_offsets = the scan at the emitting side's boundaries.
 *   k_join_emit_*       re-walk and write the pair indices / selected row ids.
 *   k_join_gather       out[c][i] = src[c][idx[i]] for the projected columns + validity.
 *
 * The outer joins (left, right, full) share build, scan and seg_out and add:
 *   k_join_count_outer  per probe row: probe once, keep the chain head in head[row], count
 *                       the chain, mark matched[build row] (left, full).
 *   k_join_build_cnt_outer  left, full: cnt[n_probe + r] = !matched[r], behind the probe rows'
 *                       counts in the one array the scan runs over.
 *   k_join_emit_outer   probe section from head / off / next alone (no re-probe), then the
 *                       unmatched build rows; DD_JOIN_NONE marks the absent side.
 *   k_join_gather_outer k_join_gather that writes zeros and validity 0 on a NONE index. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_agg_device.h"
#include "dd_hash_device.h"
#include "dd_internal.h"

#define J_THREADS DD_F_THREADS
#define J_WAVE 64
#define J_MAXK 4
#define J_EMPTY DD_F_EMPTY

/* ---------------- shared pieces ---------------- */

/* the segment s with seg_offsets[s] <= row < seg_offsets[s + 1] (k_final_claim's search:
 * empty segments are stepped over, seg_offsets[n_segs] == n_rows > row bounds it) */
template <bool STAGED>
__device__ __forceinline__ int j_find_seg(const int64_t *s_off, const int64_t *seg_offsets,
                                          int n_segs, int64_t row) {
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int64_t e = STAGED ? s_off[mid + 1] : seg_offsets[mid + 1];
        if (e > row) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* raw key bits of `row`; false when any component is NULL (the row matches nothing) */
__device__ __forceinline__ bool j_load_key(const dd_kargs &a, int nk, int64_t row,
                                           uint64_t (&kb)[J_MAXK]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < J_MAXK; k++) {
        kb[k] = 0;
        if (k >= nk) continue;
        const dd_kcol &c = a.cols[a.key_idx[k]];
        if (c.valid && !c.valid[row]) ok = false;
        else kb[k] = dd_key_bits(c, row);
    }
    return ok;
}

/* does build row `other` (never a NULL-key row: those are not inserted) carry kb? */
__device__ __forceinline__ bool j_same_key(const dd_kargs &b, int nk, int64_t other,
                                           const uint64_t (&kb)[J_MAXK]) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < J_MAXK; k++) {
        if (k >= nk) break;
        eq = eq && dd_key_bits(b.cols[b.key_idx[k]], other) == kb[k];
    }
    return eq;
}

/* ---------------- build ---------------- */

template <bool STAGED>
__global__ __launch_bounds__(J_THREADS) void k_join_build(
    dd_kargs b, const int64_t *seg_offsets, const int32_t *seg_part, int32_t n_segs,
    const uint32_t *part_base, const uint32_t *part_log2, uint32_t *table,
    uint32_t *next /* [build rows], EMPTY */, uint32_t *err) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    if (STAGED) {
        for (int i = threadIdx.x; i <= n_segs; i += J_THREADS) s_off[i] = seg_offsets[i];
        __syncthreads();
    }
    const int nk = b.n_keys > J_MAXK ? J_MAXK : b.n_keys;
    const int64_t start = (int64_t)blockIdx.x * DD_F_BLOCK_ROWS;
    const int64_t end = start + DD_F_BLOCK_ROWS < b.n_rows ? start + DD_F_BLOCK_ROWS : b.n_rows;

    for (int64_t row = start + threadIdx.x; row < end; row += J_THREADS) {
        uint64_t kb[J_MAXK];
        if (!j_load_key(b, nk, row, kb)) continue; /* NULL key: not inserted */
        const int32_t p = seg_part[j_find_seg<STAGED>(s_off, seg_offsets, n_segs, row)];
        const uint32_t base = part_base[p];
        const uint32_t lg = part_log2[p];
        const uint32_t mask = (1u << lg) - 1u;
        const uint64_t h = dd_row_hash<false>(b, row);
        uint32_t s = (uint32_t)(dd_mix64(h) >> (64 - lg));
        bool done = false;
        for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
            uint32_t *t = table + ((size_t)base + s);
            /* EMPTY -> row id once and never again: a non-EMPTY read is final */
            uint32_t cur = __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == J_EMPTY) {
                cur = atomicCAS(t, J_EMPTY, (uint32_t)row);
                if (cur == J_EMPTY) { /* this row heads its key */
                    done = true;
                    break;
                }
            }
            if (j_same_key(b, nk, (int64_t)cur, kb)) {
                /* link behind the head. Only a head's entry is ever exchanged and this row
                 * is no head, so next[row] is this lane's alone; chains are read by the
                 * next kernel only */
                const uint32_t old = atomicExch(&next[cur], (uint32_t)row);
                next[row] = old;
                done = true;
                break;
            }
        }
        if (!done) atomicOr(err, 1u); /* unreachable at load <= 0.5 */
    }
}

extern "C" hipError_t dd_launch_join_build(const dd_kargs *b, const int64_t *seg_offsets,
                                           const int32_t *seg_part, int32_t n_segs,
                                           const uint32_t *part_base,
                                           const uint32_t *part_log2, uint32_t *table,
                                           uint32_t *next, uint32_t *err, hipStream_t s) {
    const int64_t nblocks = (b->n_rows + DD_F_BLOCK_ROWS - 1) / DD_F_BLOCK_ROWS;
    if (nblocks == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_join_build<true>, dim3((unsigned)nblocks), dim3(J_THREADS), 0, s,
                           *b, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           next, err);
    else
        hipLaunchKernelGGL(k_join_build<false>, dim3((unsigned)nblocks), dim3(J_THREADS), 0, s,
                           *b, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           next, err);
    return hipGetLastError();
}

/* ---------------- probe: count and emit ---------------- */

/* head of the build chain whose key equals probe row `row`'s, or EMPTY. The table is
 * immutable by now: plain loads */
template <bool STAGED>
__device__ __forceinline__ uint32_t j_probe(const dd_kargs &b, const dd_kargs &p, int nk,
                                            int64_t row, const int64_t *s_off,
                                            const int64_t *seg_offsets,
                                            const int32_t *seg_part, int32_t n_segs,
                                            const uint32_t *part_base,
                                            const uint32_t *part_log2,
                                            const uint32_t *table) {
    uint64_t kb[J_MAXK];
    if (!j_load_key(p, nk, row, kb)) return J_EMPTY;
    const int32_t part = seg_part[j_find_seg<STAGED>(s_off, seg_offsets, n_segs, row)];
    const uint32_t base = part_base[part];
    const uint32_t lg = part_log2[part];
    const uint32_t mask = (1u << lg) - 1u;
    /* same dtypes on both sides: the probe row's hash is the build rows' of that key */
    const uint64_t h = dd_row_hash<false>(p, row);
    uint32_t s = (uint32_t)(dd_mix64(h) >> (64 - lg));
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
        const uint32_t cur = table[(size_t)base + s];
        if (cur == J_EMPTY) return J_EMPTY;
        if (j_same_key(b, nk, (int64_t)cur, kb)) return cur;
    }
    return J_EMPTY;
}

template <bool STAGED>
__global__ __launch_bounds__(J_THREADS) void k_join_count(
    dd_kargs b, dd_kargs p, const int64_t *seg_offsets, const int32_t *seg_part,
    int32_t n_segs, const uint32_t *part_base, const uint32_t *part_log2,
    const uint32_t *table, const uint32_t *next, int32_t join_type,
    uint32_t *cnt /* [probe rows]; unused for left_* */,
    uint8_t *matched /* [build rows]; left_* only */) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    if (STAGED) {
        for (int i = threadIdx.x; i <= n_segs; i += J_THREADS) s_off[i] = seg_offsets[i];
        __syncthreads();
    }
    const int nk = p.n_keys > J_MAXK ? J_MAXK : p.n_keys;
    const int64_t start = (int64_t)blockIdx.x * DD_F_BLOCK_ROWS;
    const int64_t end = start + DD_F_BLOCK_ROWS < p.n_rows ? start + DD_F_BLOCK_ROWS : p.n_rows;
    const uint32_t max_steps = (uint32_t)b.n_rows; /* a chain is no longer than the side */

    for (int64_t row = start + threadIdx.x; row < end; row += J_THREADS) {
        const uint32_t head = j_probe<STAGED>(b, p, nk, row, s_off, seg_offsets, seg_part,
                                              n_segs, part_base, part_log2, table);
        if (join_type == DD_JOIN_INNER) {
            uint32_t c = 0;
            for (uint32_t r = head; r != J_EMPTY && c < max_steps; r = next[r]) c++;
            cnt[row] = c;
        } else if (join_type == DD_JOIN_RIGHT_SEMI) {
            cnt[row] = head != J_EMPTY;
        } else if (join_type == DD_JOIN_RIGHT_ANTI) {
            cnt[row] = head == J_EMPTY;
        } else if (head != J_EMPTY && !matched[head]) {
            /* left_*: idempotent byte stores over the whole chain, head first. A lane that
             * finds the head marked skips the walk: whoever marked it finishes the chain
             * before this kernel ends, and nobody reads `matched` until then */
            uint32_t c = 0;
            for (uint32_t r = head; r != J_EMPTY && c < max_steps; r = next[r], c++)
                matched[r] = 1;
        }
    }
}

extern "C" hipError_t dd_launch_join_count(const dd_kargs *b, const dd_kargs *p,
                                           const int64_t *seg_offsets,
                                           const int32_t *seg_part, int32_t n_segs,
                                           const uint32_t *part_base,
                                           const uint32_t *part_log2, const uint32_t *table,
                                           const uint32_t *next, int32_t join_type,
                                           uint32_t *cnt, uint8_t *matched, hipStream_t s) {
    const int64_t nblocks = (p->n_rows + DD_F_BLOCK_ROWS - 1) / DD_F_BLOCK_ROWS;
    if (nblocks == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_join_count<true>, dim3((unsigned)nblocks), dim3(J_THREADS), 0, s,
                           *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           next, join_type, cnt, matched);
    else
        hipLaunchKernelGGL(k_join_count<false>, dim3((unsigned)nblocks), dim3(J_THREADS), 0, s,
                           *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2, table,
                           next, join_type, cnt, matched);
    return hipGetLastError();
}

/* left_semi / left_anti: cnt[build row] = matched ^ anti */
__global__ __launch_bounds__(J_THREADS) void k_join_left_cnt(const uint8_t *matched,
                                                             int64_t n, uint32_t anti,
                                                             uint32_t *cnt) {
    const int64_t r = (int64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (r < n) cnt[r] = (uint32_t)(matched[r] != 0) ^ anti;
}

extern "C" hipError_t dd_launch_join_left_cnt(const uint8_t *matched, int64_t n, int anti,
                                              uint32_t *cnt, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_left_cnt, dim3((unsigned)((n + J_THREADS - 1) / J_THREADS)),
                       dim3(J_THREADS), 0, s, matched, n, (uint32_t)(anti != 0), cnt);
    return hipGetLastError();
}

/* inner / right_*: one probe row per thread re-walks its matches and writes them at
 * off[row] + k */
template <bool STAGED>
__global__ __launch_bounds__(J_THREADS) void k_join_emit_probe(
    dd_kargs b, dd_kargs p, const int64_t *seg_offsets, const int32_t *seg_part,
    int32_t n_segs, const uint32_t *part_base, const uint32_t *part_log2,
    const uint32_t *table, const uint32_t *next, int32_t join_type,
    const uint32_t *off /* [probe rows] exclusive scan of cnt */, uint32_t n_out,
    uint32_t *build_idx, uint32_t *probe_idx) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    if (STAGED) {
        for (int i = threadIdx.x; i <= n_segs; i += J_THREADS) s_off[i] = seg_offsets[i];
        __syncthreads();
    }
    const int nk = p.n_keys > J_MAXK ? J_MAXK : p.n_keys;
    const int64_t start = (int64_t)blockIdx.x * DD_F_BLOCK_ROWS;
    const int64_t end = start + DD_F_BLOCK_ROWS < p.n_rows ? start + DD_F_BLOCK_ROWS : p.n_rows;

    for (int64_t row = start + threadIdx.x; row < end; row += J_THREADS) {
        const uint32_t head = j_probe<STAGED>(b, p, nk, row, s_off, seg_offsets, seg_part,
                                              n_segs, part_base, part_log2, table);
        uint32_t o = off[row];
        if (join_type == DD_JOIN_INNER) {
            /* o < n_out bounds the walk by what the count pass found */
            for (uint32_t r = head; r != J_EMPTY && o < n_out; r = next[r], o++) {
                build_idx[o] = r;
                probe_idx[o] = (uint32_t)row;
            }
        } else if ((head != J_EMPTY) == (join_type == DD_JOIN_RIGHT_SEMI) && o < n_out) {
            probe_idx[o] = (uint32_t)row;
        }
    }
}

extern "C" hipError_t dd_launch_join_emit_probe(
    const dd_kargs *b, const dd_kargs *p, const int64_t *seg_offsets, const int32_t *seg_part,
    int32_t n_segs, const uint32_t *part_base, const uint32_t *part_log2,
    const uint32_t *table, const uint32_t *next, int32_t join_type, const uint32_t *off,
    uint32_t n_out, uint32_t *build_idx, uint32_t *probe_idx, hipStream_t s) {
    const int64_t nblocks = (p->n_rows + DD_F_BLOCK_ROWS - 1) / DD_F_BLOCK_ROWS;
    if (nblocks == 0 || n_out == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_join_emit_probe<true>, dim3((unsigned)nblocks), dim3(J_THREADS),
                           0, s, *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2,
                           table, next, join_type, off, n_out, build_idx, probe_idx);
    else
        hipLaunchKernelGGL(k_join_emit_probe<false>, dim3((unsigned)nblocks), dim3(J_THREADS),
                           0, s, *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2,
                           table, next, join_type, off, n_out, build_idx, probe_idx);
    return hipGetLastError();
}

/* left_*: the selected build rows */
__global__ __launch_bounds__(J_THREADS) void k_join_emit_build(const uint8_t *matched,
                                                               int64_t n, uint32_t anti,
                                                               const uint32_t *off,
                                                               uint32_t n_out,
                                                               uint32_t *build_idx) {
    const int64_t r = (int64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (r >= n) return;
    const uint32_t sel = (uint32_t)(matched[r] != 0) ^ anti;
    const uint32_t o = off[r];
    if (sel && o < n_out) build_idx[o] = (uint32_t)r;
}

extern "C" hipError_t dd_launch_join_emit_build(const uint8_t *matched, int64_t n, int anti,
                                                const uint32_t *off, uint32_t n_out,
                                                uint32_t *build_idx, hipStream_t s) {
    if (n == 0 || n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_emit_build, dim3((unsigned)((n + J_THREADS - 1) / J_THREADS)),
                       dim3(J_THREADS), 0, s, matched, n, (uint32_t)(anti != 0), off, n_out,
                       build_idx);
    return hipGetLastError();
}

/* ---------------- scan: exclusive, in place, 64-bit sums ----------------
 * k_final_scan_*'s three passes (per-tile sums, one block over the tile sums, per-tile
 * ranks on the tile's base; none looks back at a running neighbour) with 64-bit sums: a
 * count may be as large as the build side, so 32 bits cannot hold even one tile's sum.
 * The stored offsets are the low 32 bits; the host uses them only when the exact total
 * (sums[nb]) is below 2^31. */

template <int T>
__device__ __forceinline__ uint64_t j_block_excl(uint64_t c, uint64_t *s_w, uint64_t &total) {
    const int lane = threadIdx.x & (J_WAVE - 1), w = threadIdx.x / J_WAVE;
    unsigned long long inc = c;
#pragma unroll
    for (int off = 1; off < J_WAVE; off <<= 1) {
        const unsigned long long o = __shfl_up(inc, off, J_WAVE);
        if (lane >= off) inc += o;
    }
    if (lane == J_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint64_t wbase = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < T / J_WAVE; i++) {
        const uint64_t v = s_w[i];
        if (i < w) wbase += v;
        total += v;
    }
    return wbase + inc - c;
}

/* the four counts of this thread (cnt is padded to a multiple of 4 entries, pad = 0) */
__device__ __forceinline__ uint4 j_tile_load(const uint32_t *cnt, uint64_t n_pad, uint64_t i) {
    if (i < n_pad) return *(const uint4 *)(cnt + i);
    return make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(J_THREADS) void k_join_scan_count(const uint32_t *cnt,
                                                               uint64_t n_pad,
                                                               uint64_t *sums) {
    __shared__ uint64_t s_w[J_THREADS / J_WAVE];
    const uint64_t i = (uint64_t)blockIdx.x * DD_J_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = j_tile_load(cnt, n_pad, i);
    uint64_t total;
    (void)j_block_excl<J_THREADS>((uint64_t)v.x + v.y + v.z + v.w, s_w, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* in place: sums[i] = sum of sums[0 .. i), sums[nb] = the total; DD_J_SUMS_THREADS tile
 * sums per round */
__global__ __launch_bounds__(DD_J_SUMS_THREADS) void k_join_scan_sums(uint64_t *sums,
                                                                      uint32_t nb) {
    __shared__ uint64_t s_w[DD_J_SUMS_THREADS / J_WAVE];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += DD_J_SUMS_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t c = i < nb ? sums[i] : 0u;
        uint64_t total;
        const uint64_t ex = j_block_excl<DD_J_SUMS_THREADS>(c, s_w, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
        __syncthreads(); /* s_w is reused by the next round */
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ __launch_bounds__(J_THREADS) void k_join_scan_write(uint32_t *cnt, uint64_t n_pad,
                                                               const uint64_t *sums) {
    __shared__ uint64_t s_w[J_THREADS / J_WAVE];
    const uint64_t i = (uint64_t)blockIdx.x * DD_J_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = j_tile_load(cnt, n_pad, i);
    uint64_t total;
    const uint64_t ex = sums[blockIdx.x] +
                        j_block_excl<J_THREADS>((uint64_t)v.x + v.y + v.z + v.w, s_w, total);
    if (i < n_pad)
        *(uint4 *)(cnt + i) = make_uint4((uint32_t)ex, (uint32_t)(ex + v.x),
                                         (uint32_t)(ex + v.x + v.y),
                                         (uint32_t)(ex + v.x + v.y + v.z));
}

/* out[s] = output rows before the emitting side's row seg_offsets[s]; out[n_segs + 1] =
 * the exact total once more, for the host's range check */
__global__ void k_join_seg_out(const uint32_t *off, int64_t n, const int64_t *seg_offsets,
                               int32_t n_segs, const uint64_t *sums, uint32_t nb,
                               int64_t *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)sums[nb];
    if (s <= n_segs) {
        const int64_t o = seg_offsets[s];
        out[s] = o < n ? (int64_t)off[o] : total;
    } else if (s == n_segs + 1) {
        out[s] = total;
    }
}

extern "C" hipError_t dd_launch_join_scan(uint32_t *cnt, int64_t n, uint64_t *sums,
                                          const int64_t *seg_offsets, int32_t n_segs,
                                          int64_t *seg_out, hipStream_t s) {
    const uint64_t n_pad = ((uint64_t)n + 3u) & ~(uint64_t)3u;
    const uint32_t nb = (uint32_t)((n_pad + DD_J_SCAN_TILE - 1) / DD_J_SCAN_TILE);
    if (nb) hipLaunchKernelGGL(k_join_scan_count, dim3(nb), dim3(J_THREADS), 0, s, cnt, n_pad,
                               sums);
    hipLaunchKernelGGL(k_join_scan_sums, dim3(1), dim3(DD_J_SUMS_THREADS), 0, s, sums, nb);
    if (nb) hipLaunchKernelGGL(k_join_scan_write, dim3(nb), dim3(J_THREADS), 0, s, cnt, n_pad,
                               sums);
    hipLaunchKernelGGL(k_join_seg_out, dim3((unsigned)((n_segs + 2) / 256 + 1)), dim3(256), 0,
                       s, cnt, n, seg_offsets, n_segs, sums, nb, seg_out);
    return hipGetLastError();
}

/* ---------------- gather ---------------- */

#define J_GATHER_GROUP 4 /* columns whose loads are in flight together */

template <typename T>
__device__ __forceinline__ void j_ld(dd_u128 &v, const void *src, uint32_t i) {
    v.x = (uint64_t)((const T *)src)[i];
}

/* one output row per thread: the index load, then for every group of columns all value and
 * validity loads before the group's stores, each one access of the element's own width */
__global__ __launch_bounds__(J_THREADS) void k_join_gather(dd_join_gather g,
                                                           const uint32_t *idx,
                                                           int64_t n_out) {
    const int64_t i = (int64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (i >= n_out) return;
    const uint32_t src = idx[i];
    for (int c0 = 0; c0 < g.n_cols; c0 += J_GATHER_GROUP) {
        dd_u128 v[J_GATHER_GROUP];
        uint8_t ok[J_GATHER_GROUP];
#pragma unroll
        for (int j = 0; j < J_GATHER_GROUP; j++) {
            const int c = c0 + j;
            v[j] = dd_u128{0, 0};
            ok[j] = 0;
            if (c >= g.n_cols) continue;
            switch (g.elem[c]) { /* wave-uniform */
            case 1: j_ld<uint8_t>(v[j], g.src[c], src); break;
            case 2: j_ld<uint16_t>(v[j], g.src[c], src); break;
            case 4: j_ld<uint32_t>(v[j], g.src[c], src); break;
            case 8: j_ld<uint64_t>(v[j], g.src[c], src); break;
            default: v[j] = ((const dd_u128 *)g.src[c])[src];
            }
            if (g.src_valid[c]) ok[j] = g.src_valid[c][src];
        }
#pragma unroll
        for (int j = 0; j < J_GATHER_GROUP; j++) {
            const int c = c0 + j;
            if (c >= g.n_cols) continue;
            switch (g.elem[c]) {
            case 1: ((uint8_t *)g.dst[c])[i] = (uint8_t)v[j].x; break;
            case 2: ((uint16_t *)g.dst[c])[i] = (uint16_t)v[j].x; break;
            case 4: ((uint32_t *)g.dst[c])[i] = (uint32_t)v[j].x; break;
            case 8: ((uint64_t *)g.dst[c])[i] = v[j].x; break;
            default: ((dd_u128 *)g.dst[c])[i] = v[j];
            }
            if (g.src_valid[c]) g.dst_valid[c][i] = ok[j];
        }
    }
}

extern "C" hipError_t dd_launch_join_gather(const dd_join_gather *g, const uint32_t *idx,
                                            int64_t n_out, hipStream_t s) {
    if (n_out == 0 || g->n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_gather, dim3((unsigned)((n_out + J_THREADS - 1) / J_THREADS)),
                       dim3(J_THREADS), 0, s, *g, idx, n_out);
    return hipGetLastError();
}

/* ---------------- outer joins: left, right, full ----------------
 * Output rows come in two sections over ONE count array cnt[n_probe + n_build]: the probe
 * rows' pairs (right, full: at least one row each), then for left / full the build rows no
 * probe row matched. The build part starts at index n_probe with no alignment padding, so
 * one scan serves both; every index into cnt is 64-bit. */

#define J_NONE 0xffffffffu /* DD_JOIN_NONE: the absent side of an output row */

template <bool STAGED>
__global__ __launch_bounds__(J_THREADS) void k_join_count_outer(
    dd_kargs b, dd_kargs p, const int64_t *seg_offsets, const int32_t *seg_part,
    int32_t n_segs, const uint32_t *part_base, const uint32_t *part_log2,
    const uint32_t *table, const uint32_t *next, uint32_t keep_probe /* right, full */,
    uint32_t *head_out /* [probe rows] */, uint32_t *cnt /* [probe rows] */,
    uint8_t *matched /* [build rows]; left, full only, else null */) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    if (STAGED) {
        for (int i = threadIdx.x; i <= n_segs; i += J_THREADS) s_off[i] = seg_offsets[i];
        __syncthreads();
    }
    const int nk = p.n_keys > J_MAXK ? J_MAXK : p.n_keys;
    const int64_t start = (int64_t)blockIdx.x * DD_F_BLOCK_ROWS;
    const int64_t end = start + DD_F_BLOCK_ROWS < p.n_rows ? start + DD_F_BLOCK_ROWS : p.n_rows;
    const uint32_t max_steps = (uint32_t)b.n_rows; /* a chain is no longer than the side */

    for (int64_t row = start + threadIdx.x; row < end; row += J_THREADS) {
        const uint32_t head = j_probe<STAGED>(b, p, nk, row, s_off, seg_offsets, seg_part,
                                              n_segs, part_base, part_log2, table);
        head_out[row] = head; /* the emit walks from here: it never probes again */
        uint32_t c = 0;
        if (matched) {
            /* idempotent byte stores; unlike left_semi the walk cannot stop at a marked
             * head, the count is needed. Nobody reads `matched` before this kernel ends */
            for (uint32_t r = head; r != J_EMPTY && c < max_steps; r = next[r], c++)
                if (!matched[r]) matched[r] = 1;
        } else {
            for (uint32_t r = head; r != J_EMPTY && c < max_steps; r = next[r]) c++;
        }
        cnt[row] = keep_probe && c == 0 ? 1u : c;
    }
}

extern "C" hipError_t dd_launch_join_count_outer(
    const dd_kargs *b, const dd_kargs *p, const int64_t *seg_offsets, const int32_t *seg_part,
    int32_t n_segs, const uint32_t *part_base, const uint32_t *part_log2,
    const uint32_t *table, const uint32_t *next, int keep_probe, uint32_t *head,
    uint32_t *cnt, uint8_t *matched, hipStream_t s) {
    const int64_t nblocks = (p->n_rows + DD_F_BLOCK_ROWS - 1) / DD_F_BLOCK_ROWS;
    if (nblocks == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_join_count_outer<true>, dim3((unsigned)nblocks), dim3(J_THREADS),
                           0, s, *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2,
                           table, next, (uint32_t)(keep_probe != 0), head, cnt, matched);
    else
        hipLaunchKernelGGL(k_join_count_outer<false>, dim3((unsigned)nblocks), dim3(J_THREADS),
                           0, s, *b, *p, seg_offsets, seg_part, n_segs, part_base, part_log2,
                           table, next, (uint32_t)(keep_probe != 0), head, cnt, matched);
    return hipGetLastError();
}

/* left, full: the build rows' counts, behind the probe rows' in the same array */
__global__ __launch_bounds__(J_THREADS) void k_join_build_cnt_outer(const uint8_t *matched,
                                                                    int64_t n_build,
                                                                    uint64_t n_probe,
                                                                    uint32_t *cnt) {
    const int64_t r = (int64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (r < n_build) cnt[n_probe + (uint64_t)r] = matched[r] == 0;
}

extern "C" hipError_t dd_launch_join_build_cnt_outer(const uint8_t *matched, int64_t n_build,
                                                     int64_t n_probe, uint32_t *cnt,
                                                     hipStream_t s) {
    if (n_build == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_build_cnt_outer,
                       dim3((unsigned)((n_build + J_THREADS - 1) / J_THREADS)), dim3(J_THREADS),
                       0, s, matched, n_build, (uint64_t)n_probe, cnt);
    return hipGetLastError();
}

/* one entry of cnt per thread. Probe section: walk next from the stored head and write the
 * pairs at off[row] + k, or (NONE, row) for a kept row without a match. Build section (n_tail
 * = build rows for left / full, else 0): (r, NONE) for the rows nobody marked. No key loads,
 * no table, no segment search, hence no dd_kargs. Every store is below n_out. */
__global__ __launch_bounds__(J_THREADS) void k_join_emit_outer(
    const uint32_t *head, const uint32_t *next, const uint8_t *matched,
    const uint32_t *off /* [n_probe + n_tail] exclusive scan of cnt */, uint64_t n_probe,
    uint64_t n_tail, uint32_t keep_probe, uint32_t n_out, uint32_t *build_idx,
    uint32_t *probe_idx) {
    const uint64_t i = (uint64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (i >= n_probe + n_tail) return;
    uint32_t o = off[i];
    if (i < n_probe) {
        uint32_t r = head[i];
        if (r == J_EMPTY) {
            if (keep_probe && o < n_out) {
                build_idx[o] = J_NONE;
                probe_idx[o] = (uint32_t)i;
            }
            return;
        }
        /* o < n_out bounds the walk by what the count pass found */
        for (; r != J_EMPTY && o < n_out; r = next[r], o++) {
            build_idx[o] = r;
            probe_idx[o] = (uint32_t)i;
        }
    } else {
        const uint64_t r = i - n_probe;
        if (!matched[r] && o < n_out) {
            build_idx[o] = (uint32_t)r;
            probe_idx[o] = J_NONE;
        }
    }
}

extern "C" hipError_t dd_launch_join_emit_outer(const uint32_t *head, const uint32_t *next,
                                                const uint8_t *matched, const uint32_t *off,
                                                int64_t n_probe, int64_t n_tail,
                                                int keep_probe, uint32_t n_out,
                                                uint32_t *build_idx, uint32_t *probe_idx,
                                                hipStream_t s) {
    const uint64_t n = (uint64_t)n_probe + (uint64_t)n_tail; /* < 2^32: blocks < 2^24 */
    if (n == 0 || n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_emit_outer, dim3((unsigned)((n + J_THREADS - 1) / J_THREADS)),
                       dim3(J_THREADS), 0, s, head, next, matched, off, (uint64_t)n_probe,
                       (uint64_t)n_tail, (uint32_t)(keep_probe != 0), n_out, build_idx,
                       probe_idx);
    return hipGetLastError();
}

/* k_join_gather for a side whose index may be NONE: the source is not read then, the value
 * bytes are zero and the validity byte 0. dst_valid[c] decides whether validity is written:
 * always set on a NULL-extended side (1 on a real row of a source without validity), set
 * exactly where the source has one on the other side, whose index is never NONE */
__global__ __launch_bounds__(J_THREADS) void k_join_gather_outer(dd_join_gather g,
                                                                 const uint32_t *idx,
                                                                 int64_t n_out) {
    const int64_t i = (int64_t)blockIdx.x * J_THREADS + threadIdx.x;
    if (i >= n_out) return;
    const uint32_t src = idx[i];
    const bool real = src != J_NONE;
    for (int c0 = 0; c0 < g.n_cols; c0 += J_GATHER_GROUP) {
        dd_u128 v[J_GATHER_GROUP];
        uint8_t ok[J_GATHER_GROUP];
#pragma unroll
        for (int j = 0; j < J_GATHER_GROUP; j++) {
            const int c = c0 + j;
            v[j] = dd_u128{0, 0};
            ok[j] = 0;
            if (c >= g.n_cols || !real) continue;
            switch (g.elem[c]) { /* wave-uniform */
            case 1: j_ld<uint8_t>(v[j], g.src[c], src); break;
            case 2: j_ld<uint16_t>(v[j], g.src[c], src); break;
            case 4: j_ld<uint32_t>(v[j], g.src[c], src); break;
            case 8: j_ld<uint64_t>(v[j], g.src[c], src); break;
            default: v[j] = ((const dd_u128 *)g.src[c])[src];
            }
            ok[j] = g.src_valid[c] ? g.src_valid[c][src] : (uint8_t)1;
        }
#pragma unroll
        for (int j = 0; j < J_GATHER_GROUP; j++) {
            const int c = c0 + j;
            if (c >= g.n_cols) continue;
            switch (g.elem[c]) {
            case 1: ((uint8_t *)g.dst[c])[i] = (uint8_t)v[j].x; break;
            case 2: ((uint16_t *)g.dst[c])[i] = (uint16_t)v[j].x; break;
            case 4: ((uint32_t *)g.dst[c])[i] = (uint32_t)v[j].x; break;
            case 8: ((uint64_t *)g.dst[c])[i] = v[j].x; break;
            default: ((dd_u128 *)g.dst[c])[i] = v[j];
            }
            if (g.dst_valid[c]) g.dst_valid[c][i] = ok[j];
        }
    }
}

extern "C" hipError_t dd_launch_join_gather_outer(const dd_join_gather *g, const uint32_t *idx,
                                                  int64_t n_out, hipStream_t s) {
    if (n_out == 0 || g->n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(k_join_gather_outer,
                       dim3((unsigned)((n_out + J_THREADS - 1) / J_THREADS)), dim3(J_THREADS),
                       0, s, *g, idx, n_out);
    return hipGetLastError();
}
