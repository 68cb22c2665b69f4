/* dd_sort.hip — GPU SortExec / TopK per partition above the shuffle.
 *
 * The SortExec(preserve_partitioning=[true], fetch) that closes every task of the TPC-H plans
 * in tests/tpch_plans_test.rs: rows of a device batch, routed to partitions by a segment
 * layout, come out partition-major and in key order inside each partition, ties in input
 * order. A stable LSD radix sort over ORDERED WORDS:
 *
 *   k_sort_encode   per row: one unsigned 64-bit word per key (two for dec128) whose unsigned
 *                   order is the key's order, and a META word = partition id << 32 | one byte
 *                   of null rank per key; perm[i] = i; and the DIGIT CENSUS: a 256-bin
 *                   histogram of every byte of every word over all rows (LDS histograms,
 *                   flushed with integer atomics: order-free, deterministic).
 *   (host)          reads the census and drops every pass whose byte is the same in all rows.
 *   per pass        k_sort_hist (256 bins per 2048-row tile, written hist[bin][tile]) ->
 *                   k_sort_scan_* (exclusive scan in bin-major order: count -> sums -> write,
 *                   the shape of k_final_scan_*) -> k_sort_scatter (stable).
 *   k_sort_gather_word  between two words of the plan: cur[i] = word_k[perm[i]].
 *   k_sort_seg_out  the kept rows of every partition (fetch) -> the output's perm.
 *   (k_join_gather) out[c][i] = src[c][perm[i]], through its launch in dd_internal.h.
 *
 * No lane or block waits on another's publication: a pass is three launches, and inside the
 * scatter the only cross-wave hand-off is through __syncthreads. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_agg_device.h"
#include "dd_hash_device.h"
#include "dd_internal.h"

#define S_THREADS DD_S_THREADS
#define S_WAVE 64
#define S_WAVES (S_THREADS / S_WAVE)
#define S_TILE DD_S_TILE
#define S_STEPS (S_TILE / S_THREADS) /* 64-row steps a wave walks in order */
#define S_SIGN64 0x8000000000000000ULL

static_assert(S_TILE == S_WAVES * S_STEPS * S_WAVE, "a tile is waves x steps x 64 rows");
static_assert(S_THREADS == 256, "one thread per bin in the hist / scatter kernels");

/* dd_f64_key's 32-bit twin: totalOrder on the raw f32 bit pattern */
__device__ __forceinline__ uint32_t dd_f32_key(uint32_t b) {
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

/* the ordered value word `part` of key `key` at `row`: unsigned order ==
 * key order; complemented at the dtype's own width when descending; 0 for a NULL, whose
 * value bytes are not read */
__device__ __forceinline__ uint64_t s_value_word(const dd_sort_keys &k, int key, int part,
                                                 int64_t row) {
    const uint8_t *valid = k.valid[key];
    if (valid && !valid[row]) return 0;
    const void *data = k.data[key];
    uint64_t x, m;
    switch (k.dtype[key]) { /* wave-uniform */
    case DD_KDT_U8:
    case DD_KDT_BOOL:
        x = ((const uint8_t *)data)[row];
        m = 0xffULL;
        break;
    case DD_KDT_I16:
        x = (uint64_t)(((const uint16_t *)data)[row] ^ 0x8000u);
        m = 0xffffULL;
        break;
    case DD_KDT_I32:
        x = (uint64_t)(((const uint32_t *)data)[row] ^ 0x80000000u);
        m = 0xffffffffULL;
        break;
    case DD_KDT_F32:
        x = (uint64_t)dd_f32_key(((const uint32_t *)data)[row]);
        m = 0xffffffffULL;
        break;
    case DD_KDT_F64:
        x = dd_f64_key(((const double *)data)[row]);
        m = ~0ULL;
        break;
    case DD_KDT_DEC128: {
        /* signed 128-bit: (hi with the sign flipped, lo); one 16-byte load, the host
         * checks the alignment */
        const dd_u128 v = ((const dd_u128 *)data)[row];
        x = part == 0 ? (v.y ^ S_SIGN64) : v.x;
        m = ~0ULL;
        break;
    }
    default: /* DD_KDT_I64 */
        x = ((const uint64_t *)data)[row] ^ S_SIGN64;
        m = ~0ULL;
    }
    return (k.flags[key] & DD_SORT_DESC) ? (~x & m) : x;
}

/* ---------------- encode + census ---------------- */

template <bool STAGED>
__global__ __launch_bounds__(S_THREADS) void k_sort_encode(
    dd_sort_keys k, int64_t n, const int64_t *seg_offsets /* [n_segs + 1] */,
    const int32_t *seg_part /* [n_segs] */, int32_t n_segs,
    uint64_t *words /* [n_words][n] */, uint32_t *perm /* [n] */,
    uint32_t *census /* [n_words][8][256] */) {
    __shared__ int64_t s_off[STAGED ? DD_F_LDS_SEGS + 1 : 1];
    __shared__ uint32_t s_h[8 * 256];
    if (STAGED)
        for (int i = threadIdx.x; i <= n_segs; i += S_THREADS) s_off[i] = seg_offsets[i];
    const int lane = threadIdx.x & (S_WAVE - 1);
    const int64_t start = (int64_t)blockIdx.x * DD_S_ENC_ROWS;
    const int64_t end = start + DD_S_ENC_ROWS < n ? start + DD_S_ENC_ROWS : n;
    const int meta = k.n_words - 1;

    for (int w = 0; w < k.n_words; w++) { /* block-uniform: one word at a time, 8 KiB of LDS */
        for (int i = threadIdx.x; i < 8 * 256; i += S_THREADS) s_h[i] = 0;
        __syncthreads(); /* also orders s_off's staging before the first search */
        /* block-uniform bounds: every lane stays in the loop, so the wave votes are whole */
        for (int64_t base = start; base < end; base += S_THREADS) {
            const int64_t row = base + threadIdx.x;
            const bool ok = row < end;
            uint64_t x = 0;
            if (ok && w != meta) {
                x = s_value_word(k, k.wkey[w], k.wpart[w], row);
            } else if (ok) {
                /* the segment s with seg_offsets[s] <= row < seg_offsets[s + 1], as in
                 * k_final_claim: the smallest s whose END lies past the row */
                int lo = 0, hi = n_segs - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const int64_t e = STAGED ? s_off[mid + 1] : seg_offsets[mid + 1];
                    if (e > row) hi = mid;
                    else lo = mid + 1;
                }
                x = (uint64_t)(uint32_t)seg_part[lo] << 32;
#pragma unroll
                for (int j = 0; j < DD_S_MAX_KEYS; j++) {
                    if (j >= k.n_keys) break;
                    const bool isnull = k.valid[j] && !k.valid[j][row];
                    /* null rank, 0 sorts first */
                    const bool first = (k.flags[j] & DD_SORT_NULLS_FIRST) != 0;
                    x |= (uint64_t)(isnull != first) << (8 * j);
                }
                perm[row] = (uint32_t)row;
            }
            if (ok) words[(size_t)w * (size_t)n + (size_t)row] = x;
            /* census: valid lanes are a prefix of the wave, so lane 0 speaks for a byte all
             * of them share (the common case for high bytes) with one add */
            const uint64_t act = __ballot(ok);
            if (act == 0) continue;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t d = (uint32_t)(x >> (8 * j)) & 255u;
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                if (__ballot(ok && d != d0) == 0) {
                    if (lane == 0) atomicAdd(&s_h[j * 256 + d0], (uint32_t)__popcll(act));
                } else if (ok) {
                    atomicAdd(&s_h[j * 256 + d], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 8 * 256; i += S_THREADS)
            if (s_h[i]) atomicAdd(&census[w * (8 * 256) + i], s_h[i]);
        __syncthreads(); /* s_h is zeroed again for the next word */
    }
}

extern "C" hipError_t dd_launch_sort_encode(const dd_sort_keys *k, int64_t n,
                                            const int64_t *seg_offsets,
                                            const int32_t *seg_part, int32_t n_segs,
                                            uint64_t *words, uint32_t *perm, uint32_t *census,
                                            hipStream_t s) {
    const int64_t nblocks = (n + DD_S_ENC_ROWS - 1) / DD_S_ENC_ROWS;
    if (nblocks == 0) return hipSuccess;
    if (n_segs <= DD_F_LDS_SEGS)
        hipLaunchKernelGGL(k_sort_encode<true>, dim3((unsigned)nblocks), dim3(S_THREADS), 0, s,
                           *k, n, seg_offsets, seg_part, n_segs, words, perm, census);
    else
        hipLaunchKernelGGL(k_sort_encode<false>, dim3((unsigned)nblocks), dim3(S_THREADS), 0, s,
                           *k, n, seg_offsets, seg_part, n_segs, words, perm, census);
    return hipGetLastError();
}

/* ---------------- one pass: histogram -> scan -> scatter ---------------- */

/* hist[bin * n_tiles + tile] = rows of the tile whose digit is bin */
__global__ __launch_bounds__(S_THREADS) void k_sort_hist(const uint64_t *word, int64_t n,
                                                         int shift, uint32_t n_tiles,
                                                         uint32_t *hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * S_TILE;
    uint64_t x[S_STEPS];
#pragma unroll
    for (int s = 0; s < S_STEPS; s++) { /* every load before the first atomic */
        const int64_t row = base + s * S_THREADS + threadIdx.x;
        x[s] = row < n ? word[row] : 0;
    }
#pragma unroll
    for (int s = 0; s < S_STEPS; s++) {
        const int64_t row = base + s * S_THREADS + threadIdx.x;
        if (row < n) atomicAdd(&s_h[(uint32_t)(x[s] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

/* exclusive scan of c over the block's T threads; total = block sum. s_w: T / 64 words of
 * LDS, free on entry */
template <int T>
__device__ __forceinline__ uint32_t s_block_excl(uint32_t c, uint32_t *s_w, uint32_t &total) {
    const int lane = threadIdx.x & (S_WAVE - 1), w = threadIdx.x / S_WAVE;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < S_WAVE; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, S_WAVE);
        if (lane >= off) inc += o;
    }
    if (lane == S_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < T / S_WAVE; i++) {
        const uint32_t v = s_w[i];
        if (i < w) wbase += v;
        total += v;
    }
    return wbase + inc - c;
}

/* the four counts of this thread (n_h = 256 * n_tiles is a multiple of 4) */
__device__ __forceinline__ uint4 s_tile_load(const uint32_t *hist, uint64_t n_h, uint64_t i) {
    if (i < n_h) return *(const uint4 *)(hist + i);
    return make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(S_THREADS) void k_sort_scan_count(const uint32_t *hist,
                                                               uint64_t n_h, uint32_t *sums) {
    __shared__ uint32_t s_w[S_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * DD_S_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = s_tile_load(hist, n_h, i);
    uint32_t total;
    (void)s_block_excl<S_THREADS>(v.x + v.y + v.z + v.w, s_w, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* in place: sums[i] = sum of sums[0 .. i); DD_S_SUMS_THREADS tile sums per round */
__global__ __launch_bounds__(DD_S_SUMS_THREADS) void k_sort_scan_sums(uint32_t *sums,
                                                                      uint32_t nb) {
    __shared__ uint32_t s_w[DD_S_SUMS_THREADS / S_WAVE];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += DD_S_SUMS_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t c = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = s_block_excl<DD_S_SUMS_THREADS>(c, s_w, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
        __syncthreads(); /* s_w is reused by the next round */
    }
}

/* in place: hist[i] = rows that sort before (bin, tile) i */
__global__ __launch_bounds__(S_THREADS) void k_sort_scan_write(uint32_t *hist, uint64_t n_h,
                                                               const uint32_t *sums) {
    __shared__ uint32_t s_w[S_WAVES];
    const uint64_t i = (uint64_t)blockIdx.x * DD_S_SCAN_TILE + threadIdx.x * 4u;
    const uint4 v = s_tile_load(hist, n_h, i);
    uint32_t total;
    const uint32_t ex = sums[blockIdx.x] +
                        s_block_excl<S_THREADS>(v.x + v.y + v.z + v.w, s_w, total);
    if (i < n_h)
        *(uint4 *)(hist + i) = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
}

/* Stable scatter of one tile. A row's destination is the scanned base of (digit, tile) + the
 * rows with its digit in earlier waves of the tile + in earlier steps of its wave + in lower
 * lanes of its step. A wave walks S_STEPS consecutive 64-row steps in order, so "earlier" is
 * row order. The tile is staged in LDS in digit order (24 KiB) and written out in runs. */
__global__ __launch_bounds__(S_THREADS) void k_sort_scatter(
    const uint64_t *win, const uint32_t *pin, int64_t n, int shift, uint32_t n_tiles,
    const uint32_t *hist /* scanned */, uint64_t *wout, uint32_t *pout) {
    __shared__ uint64_t s_word[S_TILE];
    __shared__ uint32_t s_perm[S_TILE];
    __shared__ uint32_t s_cnt[S_WAVES][256]; /* per wave: counts, then exclusive wave bases */
    __shared__ uint32_t s_lstart[256];       /* first staged position of a digit */
    __shared__ uint32_t s_gbase[256];        /* its first output row */
    __shared__ uint32_t s_w[S_WAVES];
    const int tid = threadIdx.x, lane = tid & (S_WAVE - 1), w = tid / S_WAVE;
    const int64_t tile0 = (int64_t)blockIdx.x * S_TILE;
    const int64_t base = tile0 + (int64_t)w * (S_STEPS * S_WAVE);

#pragma unroll
    for (int i = 0; i < S_WAVES; i++) s_cnt[i][tid] = 0;

    uint64_t x[S_STEPS];
    uint32_t p[S_STEPS], rk[S_STEPS];
#pragma unroll
    for (int s = 0; s < S_STEPS; s++) { /* every load in flight before the first use */
        const int64_t row = base + s * S_WAVE + lane;
        x[s] = row < n ? win[row] : 0;
        p[s] = row < n ? pin[row] : 0;
    }
    __syncthreads();

    const uint64_t below = (1ULL << lane) - 1ULL; /* masks are 64-bit on this target */
#pragma unroll
    for (int s = 0; s < S_STEPS; s++) {
        const bool ok = base + s * S_WAVE + lane < n;
        const uint32_t d = (uint32_t)(x[s] >> shift) & 255u;
        /* wave-wide match: the valid lanes that hold this lane's digit */
        uint64_t mask = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(ok && bit);
            mask &= bit ? bal : ~bal;
        }
        const uint32_t r = (uint32_t)__popcll(mask & below);
        /* the lowest lane of each digit adds the step's count to the wave's row and hands
         * the count of the earlier steps to its peers; s_cnt[w] is this wave's alone */
        uint32_t old = 0;
        if (ok && r == 0) old = atomicAdd(&s_cnt[w][d], (uint32_t)__popcll(mask));
        const int leader = ok ? __ffsll((unsigned long long)mask) - 1 : lane;
        rk[s] = (uint32_t)__shfl((int)old, leader, S_WAVE) + r;
    }
    __syncthreads();

    { /* thread = digit: wave bases, the digit's staged start and its output base */
        uint32_t run = 0;
#pragma unroll
        for (int i = 0; i < S_WAVES; i++) {
            const uint32_t c = s_cnt[i][tid];
            s_cnt[i][tid] = run;
            run += c;
        }
        uint32_t total;
        s_lstart[tid] = s_block_excl<S_THREADS>(run, s_w, total);
        s_gbase[tid] = hist[(size_t)tid * n_tiles + blockIdx.x];
    }
    __syncthreads();

#pragma unroll
    for (int s = 0; s < S_STEPS; s++) {
        if (base + s * S_WAVE + lane < n) {
            const uint32_t d = (uint32_t)(x[s] >> shift) & 255u;
            const uint32_t pos = s_lstart[d] + s_cnt[w][d] + rk[s]; /* < rows of the tile */
            s_word[pos] = x[s];
            s_perm[pos] = p[s];
        }
    }
    __syncthreads();

    const int64_t left = n - tile0;
    const uint32_t rows = left < S_TILE ? (uint32_t)left : (uint32_t)S_TILE;
    for (uint32_t j = tid; j < rows; j += S_THREADS) {
        const uint64_t xw = s_word[j];
        const uint32_t d = (uint32_t)(xw >> shift) & 255u;
        const size_t dst = (size_t)s_gbase[d] + (j - s_lstart[d]);
        wout[dst] = xw;
        pout[dst] = s_perm[j];
    }
}

/* hist: u32[256 * n_tiles], sums: u32[256 * n_tiles / DD_S_SCAN_TILE rounded up] */
extern "C" hipError_t dd_launch_sort_pass(const uint64_t *win, const uint32_t *pin, int64_t n,
                                          int shift, uint32_t *hist, uint32_t *sums,
                                          uint64_t *wout, uint32_t *pout, hipStream_t s) {
    const uint32_t n_tiles = (uint32_t)((n + S_TILE - 1) / S_TILE);
    if (n_tiles == 0) return hipSuccess;
    const uint64_t n_h = (uint64_t)n_tiles * 256u;
    const uint32_t nb = (uint32_t)((n_h + DD_S_SCAN_TILE - 1) / DD_S_SCAN_TILE);
    hipLaunchKernelGGL(k_sort_hist, dim3(n_tiles), dim3(S_THREADS), 0, s, win, n, shift,
                       n_tiles, hist);
    hipLaunchKernelGGL(k_sort_scan_count, dim3(nb), dim3(S_THREADS), 0, s, hist, n_h, sums);
    hipLaunchKernelGGL(k_sort_scan_sums, dim3(1), dim3(DD_S_SUMS_THREADS), 0, s, sums, nb);
    hipLaunchKernelGGL(k_sort_scan_write, dim3(nb), dim3(S_THREADS), 0, s, hist, n_h, sums);
    hipLaunchKernelGGL(k_sort_scatter, dim3(n_tiles), dim3(S_THREADS), 0, s, win, pin, n, shift,
                       n_tiles, hist, wout, pout);
    return hipGetLastError();
}

/* ---------------- between two words; after the passes ---------------- */

__global__ __launch_bounds__(S_THREADS) void k_sort_gather_word(const uint64_t *src,
                                                                const uint32_t *perm,
                                                                int64_t n, uint64_t *out) {
    const int64_t i = (int64_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (i < n) out[i] = src[perm[i]];
}

extern "C" hipError_t dd_launch_sort_gather_word(const uint64_t *src, const uint32_t *perm,
                                                 int64_t n, uint64_t *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_gather_word, dim3((unsigned)((n + S_THREADS - 1) / S_THREADS)),
                       dim3(S_THREADS), 0, s, src, perm, n, out);
    return hipGetLastError();
}

/* Output row i lies in the partition p with out_off[p] <= i < out_off[p + 1] (fetch has cut
 * the counts); its source is sorted row in_off[p] + (i - out_off[p]). */
__global__ __launch_bounds__(S_THREADS) void k_sort_seg_out(const uint32_t *sorted,
                                                            const int64_t *in_off,
                                                            const int64_t *out_off,
                                                            int32_t n_parts, int64_t n_out,
                                                            uint32_t *perm_out) {
    const int64_t i = (int64_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (i >= n_out) return;
    int lo = 0, hi = n_parts - 1; /* out_off[n_parts] == n_out > i bounds the search */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (out_off[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    perm_out[i] = sorted[in_off[lo] + (i - out_off[lo])];
}

extern "C" hipError_t dd_launch_sort_seg_out(const uint32_t *sorted, const int64_t *in_off,
                                             const int64_t *out_off, int32_t n_parts,
                                             int64_t n_out, uint32_t *perm_out, hipStream_t s) {
    if (n_out == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sort_seg_out, dim3((unsigned)((n_out + S_THREADS - 1) / S_THREADS)),
                       dim3(S_THREADS), 0, s, sorted, in_off, out_off, n_parts, n_out,
                       perm_out);
    return hipGetLastError();
}
