/* dd_views.hip — Utf8View / BinaryView columns around the shuffle.
 *
 * The reference garbage-collects view arrays before a batch goes on the wire
 * (garbage_collect_arrays, src/protocol/grpc/worker_service.rs:408-433: StringViewArray::gc
 * / BinaryViewArray::gc keep only the referenced bytes). The device's internal var-width
 * form (dense offsets + bytes) is that form already, so view GC is two gathers:
 *   ingest  views + N data buffers -> dense utf8          (len, scan, add, copy)
 *   emit    partition-major utf8   -> per-window views    (sums, scan, build, copy)
 * Both copy steps gather (src, len) segments into a dense output at scanned offsets and
 * share one tile body (vw_tile_copy): a block owns DD_VW_TILE_ROWS rows whose output range
 * is contiguous. The direct tier (the default: it measured faster) copies
 * each value straight to global memory, by 16-lane groups or, for long values, the whole
 * wave. The LDS-staged tier (DD_VIEW_LDS=1) places the values in an LDS byte image and
 * flushes it with aligned 8-byte stores; a tile whose range is larger than the image
 * copies directly (block-uniform branch).
 * Scans are reduce -> single-block scan of tile sums -> add; no workgroup ever waits for
 * another. Everything is a pure function of the inputs: results are bit-exact. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_internal.h"

#define VW_WAVE 64
#define VW_THREADS DD_VW_THREADS
#define VW_WAVES (VW_THREADS / VW_WAVE)
#define VW_RPT (DD_VW_TILE_ROWS / VW_THREADS) /* rows per thread */
#define VW_SCAN_THREADS 1024

static_assert(DD_VW_TILE_ROWS % VW_THREADS == 0, "tile rows must be a multiple of the block");
static_assert(DD_VW_TILE_ROWS % 4 == 0, "k_vw_add loads the lengths as int4");
static_assert(DD_VW_IMAGE_BYTES % 8 == 0, "the image is flushed in 8-byte words");

/* ---------------- helpers ---------------- */

__device__ __forceinline__ uint64_t vw_shfl_up64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, VW_WAVE);
    const uint32_t hi = __shfl_up((uint32_t)(v >> 32), d, VW_WAVE);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t vw_shfl64(uint64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, VW_WAVE);
    const uint32_t hi = __shfl((uint32_t)(v >> 32), src, VW_WAVE);
    return ((uint64_t)hi << 32) | lo;
}

/* inclusive wave scan */
__device__ __forceinline__ uint64_t vw_wave_incl(uint64_t v) {
    const int lane = threadIdx.x % VW_WAVE;
#pragma unroll
    for (int d = 1; d < VW_WAVE; d <<= 1) {
        const uint64_t o = vw_shfl_up64(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

/* block exclusive scan over NW waves in thread order; sm holds NW entries; *total = sum */
template <int NW>
__device__ __forceinline__ uint64_t vw_block_excl(uint64_t v, uint64_t *total, uint64_t *sm) {
    const int lane = threadIdx.x % VW_WAVE, wid = threadIdx.x / VW_WAVE;
    const uint64_t inc = vw_wave_incl(v);
    if (lane == VW_WAVE - 1) sm[wid] = inc;
    __syncthreads();
    uint64_t before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) {
        const uint64_t s = sm[q];
        if (q < wid) before += s;
        tot += s;
    }
    __syncthreads(); /* sm is reused by the next call */
    *total = tot;
    return before + inc - v;
}

/* LANES lanes (a 16-lane group or the whole wave; `sub` = the lane's index among them)
 * copy n bytes from global src to dst (LDS image or global). dal = the byte address of dst
 * modulo 4: the head runs to dst's next 4-byte boundary, the body moves dst-aligned dwords
 * (the source side is assembled from an unaligned load), the tail is bytes again. */
template <int LANES>
__device__ __forceinline__ void vw_lanes_copy(uint8_t *__restrict__ dst, uint32_t dal,
                                              const uint8_t *__restrict__ src, int32_t n,
                                              int sub) {
    int32_t h = (int32_t)((4u - (dal & 3u)) & 3u);
    if (h > n) h = n;
    if (sub < h) dst[sub] = src[sub];
    const int32_t nw = (n - h) >> 2;
    for (int32_t w = sub; w < nw; w += LANES) {
        uint32_t v;
        __builtin_memcpy(&v, src + h + 4 * w, 4);
        *(uint32_t *)(dst + h + 4 * w) = v;
    }
    const int32_t t0 = h + 4 * nw;
    if (sub < n - t0) dst[t0 + sub] = src[t0 + sub];
}

/* a lane places its own <= 12 inline bytes (registers w[0..2]); fully unrolled so the
 * register array is only ever indexed statically */
__device__ __forceinline__ void vw_place_inline(uint8_t *dst, const uint32_t (&w)[3],
                                                int32_t n) {
#pragma unroll
    for (int j = 0; j < 12; j++)
        if (j < n) dst[j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
}

/* One row of a tile as the copy body sees it: n bytes that land at byte `rel` of the
 * tile's output range, from the lane's registers (inl) or from global memory (src). */
struct vw_seg {
    const uint8_t *src;
    uint32_t w[3];
    int32_t n;
    uint32_t rel;
    bool inl;
};

/* Every wave places its rows at d0 + rel; the address of d0 is congruent to a modulo 4.
 * Inline values go straight from the owning lane's registers. Values from global memory
 * up to VW_GROUP_MAX bytes are copied by 16-lane groups, four values of a wave in flight at
 * once (group q walks the rows held by lanes 16q..16q+15); longer ones by the whole wave. */
#define VW_GRP 16
#define VW_GROUP_MAX 1024
__device__ __forceinline__ void vw_place_rows(uint8_t *d0, uint32_t a,
                                              const vw_seg (&seg)[VW_RPT]) {
    const int lane = threadIdx.x % VW_WAVE;
    const int sub = lane % VW_GRP, g0 = lane - sub;
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const vw_seg &s = seg[j];
        if (s.inl && s.n > 0) vw_place_inline(d0 + s.rel, s.w, s.n);
        const bool glob = !s.inl && s.n > 0;
        const uint64_t ms = __ballot(glob && s.n <= VW_GROUP_MAX);
        uint64_t mb = __ballot(glob && s.n > VW_GROUP_MAX);
        const int32_t gn = (glob && s.n <= VW_GROUP_MAX) ? s.n : 0;
        if (ms) { /* wave-uniform */
            for (int t = 0; t < VW_GRP; t++) {
                /* does any group hold a short global value at its t-th lane? */
                if (!((ms >> t) & 0x0001000100010001ull)) continue; /* wave-uniform */
                const uint8_t *src = (const uint8_t *)vw_shfl64((uint64_t)s.src, g0 + t);
                const int32_t n = __shfl(gn, g0 + t, VW_WAVE);
                const uint32_t rel = __shfl(s.rel, g0 + t, VW_WAVE);
                if (n > 0) vw_lanes_copy<VW_GRP>(d0 + rel, a + rel, src, n, sub);
            }
        }
        while (mb) { /* wave-uniform */
            const int b = __builtin_ctzll(mb);
            mb &= mb - 1;
            const uint8_t *src = (const uint8_t *)vw_shfl64((uint64_t)s.src, b);
            const int32_t n = __shfl(s.n, b, VW_WAVE);
            const uint32_t rel = __shfl(s.rel, b, VW_WAVE);
            vw_lanes_copy<VW_WAVE>(d0 + rel, a + rel, src, n, lane);
        }
    }
}

/* Shared tile body. Lane l of wave v holds rows v*VW_RPT*64 + j*64 + l (j < VW_RPT) of the
 * tile in seg[j]. [base, base + span) is the tile's byte range of `out`. */
template <bool LDS>
__device__ __forceinline__ void vw_tile_copy(uint8_t *out, int64_t base, int64_t span,
                                             const vw_seg (&seg)[VW_RPT], uint8_t *img) {
    const uint32_t a = (uint32_t)(base & 7);
    /* `out` is 8-byte aligned, so out + base and img + a are both congruent to a */
    if (!LDS || span > (int64_t)DD_VW_IMAGE_BYTES) { /* block-uniform */
        vw_place_rows(out + base, a, seg);
        return;
    }
    vw_place_rows(img + a, a, seg);
    __syncthreads();
    /* flush: 8-byte words of the image; the first and last word may be shared with the
     * neighbouring tiles and are written byte by byte */
    const uint32_t total = a + (uint32_t)span;
    const uint32_t nwords = (total + 7) >> 3;
    uint8_t *oal = out + (base - a);
    for (uint32_t k = threadIdx.x; k < nwords; k += VW_THREADS) {
        const uint32_t lo = k * 8, hi = lo + 8;
        if (lo >= a && hi <= total) {
            *(uint64_t *)(oal + lo) = *(const uint64_t *)(img + lo);
        } else {
            const uint32_t b0 = lo > a ? lo : a, b1 = hi < total ? hi : total;
            for (uint32_t x = b0; x < b1; x++) oal[x] = img[x];
        }
    }
}

/* ---------------- ingest ---------------- */

/* (a) length pass: one 16-byte view per lane, validated; lens[] (the offsets buffer, tile
 * padded) gets the row length, tsum[tile] the tile's byte total */
__global__ void __launch_bounds__(VW_THREADS)
k_vw_len(const uint4 *views, const uint8_t *valid, int64_t n_rows, const int64_t *buf_lens,
         int32_t n_bufs, int32_t *lens, uint64_t *tsum, uint32_t *flag) {
    __shared__ uint64_t sm[VW_WAVES];
    const int64_t r0 = (int64_t)blockIdx.x * DD_VW_TILE_ROWS;
    uint64_t mine = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const int64_t r = r0 + j * VW_THREADS + threadIdx.x;
        int32_t len = 0;
        if (r < n_rows && (!valid || valid[r])) {
            const uint4 v = views[r];
            len = (int32_t)v.x;
            if (len < 0) {
                bad = true;
                len = 0;
            } else if (len > 12) {
                const int32_t bi = (int32_t)v.z, off = (int32_t)v.w;
                if (bi < 0 || bi >= n_bufs || off < 0 ||
                    (int64_t)off + (int64_t)len > buf_lens[bi]) {
                    bad = true;
                    len = 0;
                }
            }
        }
        lens[r] = len; /* rows past n_rows inside the padded tile get 0 */
        mine += (uint64_t)len;
    }
    uint64_t tot;
    (void)vw_block_excl<VW_WAVES>(mine, &tot, sm);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
    if (bad) atomicOr(flag, 1u);
}

/* (b) single-block exclusive scan of column blockIdx.x of in[n][nc] into out[n+1][nc];
 * meta[c] = the column total. Column 0 also counts the tiles whose sum exceeds the LDS
 * image (meta[nc]) and, when off_end is given, stores the total there (offsets[n_rows]). */
__global__ void __launch_bounds__(VW_SCAN_THREADS)
k_vw_scan(const uint64_t *in, int64_t n, int32_t nc, uint64_t *out, uint64_t *meta,
          int32_t *off_end) {
    __shared__ uint64_t sm[VW_SCAN_THREADS / VW_WAVE];
    __shared__ uint32_t s_big;
    const int32_t c = blockIdx.x;
    if (threadIdx.x == 0) s_big = 0;
    __syncthreads();
    uint64_t carry = 0;
    uint32_t big = 0;
    for (int64_t b0 = 0; b0 < n; b0 += VW_SCAN_THREADS) {
        const int64_t i = b0 + threadIdx.x;
        const uint64_t v = i < n ? in[i * nc + c] : 0;
        big += v > (uint64_t)DD_VW_IMAGE_BYTES;
        uint64_t tot;
        const uint64_t ex = vw_block_excl<VW_SCAN_THREADS / VW_WAVE>(v, &tot, sm);
        if (i < n) out[i * nc + c] = carry + ex;
        carry += tot;
    }
    if (c == 0 && big) atomicAdd(&s_big, big);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[n * nc + c] = carry;
        meta[c] = carry;
        if (c == 0) {
            meta[nc] = s_big;
            if (off_end) *off_end = (int32_t)carry;
        }
    }
}

/* (b) add: lens -> zero-based exclusive offsets, in place. Thread t owns rows 4t..4t+3 of
 * the tile (one int4). The padded tail of the last tile holds zeros, so offsets[n_rows]
 * comes out as the total. */
__global__ void __launch_bounds__(VW_THREADS)
k_vw_add(int32_t *offs, const uint64_t *tbase) {
    __shared__ uint64_t sm[VW_WAVES];
    int32_t *o = offs + (int64_t)blockIdx.x * DD_VW_TILE_ROWS;
    const uint64_t base = tbase[blockIdx.x];
    const int q = threadIdx.x;
    const bool mine = q < DD_VW_TILE_ROWS / 4; /* every thread joins the block scan */
    int4 l = make_int4(0, 0, 0, 0);
    if (mine) l = ((const int4 *)o)[q];
    uint64_t tot;
    const uint64_t ex =
        base + vw_block_excl<VW_WAVES>((uint64_t)l.x + (uint64_t)l.y + (uint64_t)l.z +
                                           (uint64_t)l.w, &tot, sm);
    if (mine) {
        int4 r;
        r.x = (int32_t)ex;
        r.y = (int32_t)(ex + (uint64_t)l.x);
        r.z = (int32_t)(ex + (uint64_t)l.x + (uint64_t)l.y);
        r.w = (int32_t)(ex + (uint64_t)l.x + (uint64_t)l.y + (uint64_t)l.z);
        ((int4 *)o)[q] = r;
    }
}
static_assert(DD_VW_TILE_ROWS / 4 <= VW_THREADS, "k_vw_add scans one int4 per thread");

/* (c)/(d) copy: a block owns one row tile */
template <bool LDS>
__global__ void __launch_bounds__(VW_THREADS)
k_vw_copy(const uint4 *views, int64_t n_rows, const uint8_t *const *bufs,
          const int32_t *offs, uint8_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t img[LDS ? DD_VW_IMAGE_BYTES + 8 : 8];
    const int lane = threadIdx.x % VW_WAVE, wid = threadIdx.x / VW_WAVE;
    const int64_t r0 = (int64_t)blockIdx.x * DD_VW_TILE_ROWS;
    const int64_t r1 = r0 + DD_VW_TILE_ROWS < n_rows ? r0 + DD_VW_TILE_ROWS : n_rows;
    const int64_t base = offs[r0], span = (int64_t)offs[r1] - base;
    if (span == 0) return; /* block-uniform */
    vw_seg seg[VW_RPT];
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const int64_t r = r0 + (wid * VW_RPT + j) * VW_WAVE + lane;
        vw_seg &s = seg[j];
        s.n = 0;
        s.rel = 0;
        s.inl = true;
        s.src = nullptr;
        s.w[0] = s.w[1] = s.w[2] = 0;
        if (r < r1) {
            const int32_t o0 = offs[r];
            s.n = offs[r + 1] - o0;
            s.rel = (uint32_t)(o0 - base);
            if (s.n > 0) { /* a null (or empty) row's view is never interpreted */
                const uint4 v = views[r];
                if (s.n <= 12) {
                    s.w[0] = v.y;
                    s.w[1] = v.z;
                    s.w[2] = v.w;
                } else {
                    s.inl = false;
                    s.src = bufs[(int32_t)v.z] + (int32_t)v.w;
                }
            }
        }
    }
    vw_tile_copy<LDS>(out, base, span, seg, img);
}

/* ---------------- emit ---------------- */

/* tile sums: column 0 = bytes of every row, column 1 = bytes of valid rows longer than 12 */
__global__ void __launch_bounds__(VW_THREADS)
k_ve_sums(const dd_vw_tile *tiles, const uint32_t *lens, const uint8_t *valid,
          uint64_t *tsum) {
    __shared__ uint64_t sm[VW_WAVES];
    const dd_vw_tile t = tiles[blockIdx.x];
    uint64_t all = 0, lng = 0;
    for (int64_t r = t.row_lo + threadIdx.x; r < t.row_hi; r += VW_THREADS) {
        const uint32_t l = lens[r];
        all += l;
        if (l > 12 && (!valid || valid[r])) lng += l;
    }
    uint64_t ta, tl;
    (void)vw_block_excl<VW_WAVES>(all, &ta, sm);
    (void)vw_block_excl<VW_WAVES>(lng, &tl, sm);
    if (threadIdx.x == 0) {
        tsum[2 * (int64_t)blockIdx.x] = ta;
        tsum[2 * (int64_t)blockIdx.x + 1] = tl;
    }
}

/* Per-row byte start (in the partitioner's byte buffer) and long-byte start (in the
 * emitted buffer) of the tile's rows, in the copy body's row layout: lane l of wave v holds
 * rows v*VW_RPT*64 + j*64 + l. ex_all / ex_lng are exclusive prefixes within the tile. */
struct ve_rows {
    uint32_t len[VW_RPT];
    bool ok[VW_RPT]; /* valid row inside the tile */
    uint64_t ex_all[VW_RPT], ex_lng[VW_RPT];
};

__device__ __forceinline__ void ve_scan_tile(const dd_vw_tile &t, const uint32_t *lens,
                                             const uint8_t *valid, ve_rows &R,
                                             uint64_t *sm /* [2][VW_WAVES * VW_RPT] */) {
    const int lane = threadIdx.x % VW_WAVE, wid = threadIdx.x / VW_WAVE;
    constexpr int NG = VW_WAVES * VW_RPT; /* 64-row groups per tile */
    uint64_t inc_all[VW_RPT], inc_lng[VW_RPT];
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const int64_t r = t.row_lo + (wid * VW_RPT + j) * VW_WAVE + lane;
        const bool in = r < t.row_hi;
        R.len[j] = in ? lens[r] : 0u;
        R.ok[j] = in && (!valid || valid[r]);
        const uint64_t lg = (R.ok[j] && R.len[j] > 12) ? R.len[j] : 0u;
        inc_all[j] = vw_wave_incl(R.len[j]);
        inc_lng[j] = vw_wave_incl(lg);
        R.ex_all[j] = inc_all[j] - R.len[j];
        R.ex_lng[j] = inc_lng[j] - lg;
        if (lane == VW_WAVE - 1) {
            sm[wid * VW_RPT + j] = inc_all[j];
            sm[NG + wid * VW_RPT + j] = inc_lng[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const int g = wid * VW_RPT + j;
        uint64_t ba = 0, bl = 0;
#pragma unroll
        for (int q = 0; q < NG; q++) {
            if (q < g) {
                ba += sm[q];
                bl += sm[NG + q];
            }
        }
        R.ex_all[j] += ba;
        R.ex_lng[j] += bl;
    }
}

/* build: one 16-byte view per row */
__global__ void __launch_bounds__(VW_THREADS)
k_ve_build(const dd_vw_tile *tiles, const uint32_t *lens, const uint8_t *valid,
           const uint8_t *bytes, const uint64_t *part_boff, const uint64_t *S, uint4 *views) {
    __shared__ uint64_t sm[2 * VW_WAVES * VW_RPT];
    const int lane = threadIdx.x % VW_WAVE, wid = threadIdx.x / VW_WAVE;
    const dd_vw_tile t = tiles[blockIdx.x];
    ve_rows R;
    ve_scan_tile(t, lens, valid, R, sm);
    /* S[tile][0] scans bytes over all tiles; a partition's bytes start at part_boff */
    const uint64_t row_base =
        part_boff[t.part] + (S[2 * (int64_t)blockIdx.x] - S[2 * (int64_t)t.part_first]);
    const uint64_t lng_base = S[2 * (int64_t)blockIdx.x + 1] - S[2 * (int64_t)t.win_first + 1];
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        const int64_t r = t.row_lo + (wid * VW_RPT + j) * VW_WAVE + lane;
        if (r >= t.row_hi) continue;
        uint4 v = make_uint4(0u, 0u, 0u, 0u); /* null row: 16 zero bytes */
        if (R.ok[j]) {
            const uint32_t n = R.len[j];
            const uint8_t *src = bytes + row_base + R.ex_all[j];
            uint32_t w[3] = {0u, 0u, 0u};
            const uint32_t take = n > 12 ? 4u : n;
#pragma unroll
            for (int x = 0; x < 12; x++)
                if ((uint32_t)x < take) w[x >> 2] |= (uint32_t)src[x] << ((x & 3) * 8);
            v.x = n;
            v.y = w[0];
            if (n > 12) {
                v.z = 0u; /* buffer_index */
                v.w = (uint32_t)(lng_base + R.ex_lng[j]);
            } else {
                v.z = w[1];
                v.w = w[2];
            }
        }
        views[r] = v;
    }
}

/* copy: the long values of valid rows, tile by tile, into the emitted byte buffer (the
 * windows' buffers are adjacent: window w starts at S[win_first(w)][1]) */
template <bool LDS>
__global__ void __launch_bounds__(VW_THREADS)
k_ve_copy(const dd_vw_tile *tiles, const uint32_t *lens, const uint8_t *valid,
          const uint8_t *bytes, const uint64_t *part_boff, const uint64_t *S, uint8_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t img[LDS ? DD_VW_IMAGE_BYTES + 8 : 8];
    __shared__ uint64_t sm[2 * VW_WAVES * VW_RPT];
    const dd_vw_tile t = tiles[blockIdx.x];
    const int64_t base = (int64_t)S[2 * (int64_t)blockIdx.x + 1];
    const int64_t span = (int64_t)S[2 * (int64_t)blockIdx.x + 3] - base;
    if (span == 0) return; /* block-uniform: no long value in this tile */
    ve_rows R;
    ve_scan_tile(t, lens, valid, R, sm);
    const uint64_t row_base =
        part_boff[t.part] + (S[2 * (int64_t)blockIdx.x] - S[2 * (int64_t)t.part_first]);
    vw_seg seg[VW_RPT];
#pragma unroll
    for (int j = 0; j < VW_RPT; j++) {
        vw_seg &s = seg[j];
        const bool lg = R.ok[j] && R.len[j] > 12;
        s.inl = false;
        s.w[0] = s.w[1] = s.w[2] = 0;
        s.n = lg ? (int32_t)R.len[j] : 0;
        s.rel = (uint32_t)R.ex_lng[j];
        s.src = bytes + row_base + R.ex_all[j];
    }
    vw_tile_copy<LDS>(out, base, span, seg, img);
}

/* ---------------- launchers ---------------- */

extern "C" {

hipError_t dd_launch_vw_len(const void *views, const uint8_t *valid, int64_t n_rows,
                            const int64_t *buf_lens, int32_t n_bufs, int32_t *lens,
                            uint64_t *tsum, uint32_t *flag, hipStream_t s) {
    const int64_t nt = (n_rows + DD_VW_TILE_ROWS - 1) / DD_VW_TILE_ROWS;
    if (nt <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vw_len, dim3((unsigned)nt), dim3(VW_THREADS), 0, s,
                       (const uint4 *)views, valid, n_rows, buf_lens, n_bufs, lens, tsum,
                       flag);
    return hipGetLastError();
}

hipError_t dd_launch_vw_scan(const uint64_t *in, int64_t n, int32_t nc, uint64_t *out,
                             uint64_t *meta, int32_t *off_end, hipStream_t s) {
    hipLaunchKernelGGL(k_vw_scan, dim3((unsigned)nc), dim3(VW_SCAN_THREADS), 0, s, in, n, nc,
                       out, meta, off_end);
    return hipGetLastError();
}

hipError_t dd_launch_vw_add(int32_t *offs, int64_t n_tiles, const uint64_t *tbase,
                            hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vw_add, dim3((unsigned)n_tiles), dim3(VW_THREADS), 0, s, offs, tbase);
    return hipGetLastError();
}

hipError_t dd_launch_vw_copy(const void *views, int64_t n_rows, const uint8_t *const *bufs,
                             const int32_t *offs, uint8_t *out, int lds, hipStream_t s) {
    const int64_t nt = (n_rows + DD_VW_TILE_ROWS - 1) / DD_VW_TILE_ROWS;
    if (nt <= 0) return hipSuccess;
    if (lds)
        hipLaunchKernelGGL(k_vw_copy<true>, dim3((unsigned)nt), dim3(VW_THREADS), 0, s,
                           (const uint4 *)views, n_rows, bufs, offs, out);
    else
        hipLaunchKernelGGL(k_vw_copy<false>, dim3((unsigned)nt), dim3(VW_THREADS), 0, s,
                           (const uint4 *)views, n_rows, bufs, offs, out);
    return hipGetLastError();
}

hipError_t dd_launch_ve_sums(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                             const uint8_t *valid, uint64_t *tsum, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ve_sums, dim3((unsigned)n_tiles), dim3(VW_THREADS), 0, s, tiles, lens,
                       valid, tsum);
    return hipGetLastError();
}

hipError_t dd_launch_ve_build(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                              const uint8_t *valid, const uint8_t *bytes,
                              const uint64_t *part_boff, const uint64_t *S, void *views,
                              hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ve_build, dim3((unsigned)n_tiles), dim3(VW_THREADS), 0, s, tiles,
                       lens, valid, bytes, part_boff, S, (uint4 *)views);
    return hipGetLastError();
}

hipError_t dd_launch_ve_copy(const dd_vw_tile *tiles, int64_t n_tiles, const uint32_t *lens,
                             const uint8_t *valid, const uint8_t *bytes,
                             const uint64_t *part_boff, const uint64_t *S, uint8_t *out,
                             int lds, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (lds)
        hipLaunchKernelGGL(k_ve_copy<true>, dim3((unsigned)n_tiles), dim3(VW_THREADS), 0, s,
                           tiles, lens, valid, bytes, part_boff, S, out);
    else
        hipLaunchKernelGGL(k_ve_copy<false>, dim3((unsigned)n_tiles), dim3(VW_THREADS), 0, s,
                           tiles, lens, valid, bytes, part_boff, S, out);
    return hipGetLastError();
}
}
