/* dd_dictgc.hip — per-window dictionary GC over the partitioner's output.
 *
 * Mirrors what the reference does before a batch goes on the wire
 * (src/protocol/grpc/worker_service.rs:363-433: garbage_collect_arrays compacts each
 * dictionary column to the values the batch references, then resends the dictionary):
 *   mark    row-rate   one workgroup per row tile sets the window's used bitmap
 *   rank    dict-rate  per-window exclusive prefix of word popcounts + value/byte totals
 *   compact dict-rate  lengths at rank -> per-window scan -> byte copy
 *   remap   row-rate   new index = prefix[k>>5] + popc(bits[k>>5] & below(k))
 *   rebase  row-rate   out[i] = in[i] + base[seg(i)] (consumer side of the exchange)
 * No W x dict_n remap table is ever materialised: the bitmap + word prefix IS the table.
 * Everything is a pure function of the inputs (bit OR / popcount / order-preserving
 * filter), so results are bit-exact whatever the scheduling. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_internal.h"

#define GC_WAVE 64
#define GC_SCAN_THREADS 1024

extern __shared__ uint32_t gc_lds[];

/* ---------------- mark ---------------- */

template <bool LDS>
__device__ __forceinline__ void gc_mark_one(uint32_t k, uint32_t dict_n, uint32_t *wbits,
                                            bool &bad) {
    if (k >= dict_n) { /* also catches negative indices */
        bad = true;
        return;
    }
    const uint32_t m = 1u << (k & 31);
    if (LDS) {
        atomicOr(&gc_lds[k >> 5], m);
    } else {
        uint32_t *wd = wbits + (k >> 5);
        /* test first: a stale 0 only costs a redundant OR */
        if (!(__atomic_load_n(wd, __ATOMIC_RELAXED) & m)) atomicOr(wd, m);
    }
}

template <bool LDS>
__global__ void k_gc_mark(const dd_gc_tile *tiles, const int32_t *idx, const uint8_t *valid,
                          uint32_t dict_n, uint32_t nw, uint32_t *bits, uint32_t *flag) {
    const dd_gc_tile t = tiles[blockIdx.x];
    uint32_t *wbits = bits + (size_t)t.window * nw;
    const int64_t bd = blockDim.x;
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < nw; j += blockDim.x) gc_lds[j] = 0;
        __syncthreads();
    }
    bool bad = false;
    int64_t i = t.row_lo + threadIdx.x;
    /* 4 independent loads in flight per thread before the (LDS/global) atomics */
    for (; i + 3 * bd < t.row_hi; i += 4 * bd) {
        uint32_t k[4];
        uint8_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            k[u] = (uint32_t)idx[i + u * bd];
            v[u] = valid ? valid[i + u * bd] : (uint8_t)1;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (v[u]) gc_mark_one<LDS>(k[u], dict_n, wbits, bad);
    }
    for (; i < t.row_hi; i += bd) {
        if (valid && !valid[i]) continue;
        gc_mark_one<LDS>((uint32_t)idx[i], dict_n, wbits, bad);
    }
    if (bad) atomicOr(flag, 1u);
    if (LDS) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nw; j += blockDim.x) {
            const uint32_t v = gc_lds[j];
            if (v) atomicOr(&wbits[j], v);
        }
    }
}

/* ---------------- block scan helper (GC_SCAN_THREADS threads) ---------------- */

__device__ __forceinline__ uint32_t gc_block_excl_scan(uint32_t v, uint32_t *total,
                                                       uint32_t *sm) {
    const int lane = threadIdx.x % GC_WAVE, wid = threadIdx.x / GC_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < GC_WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, GC_WAVE);
        if (lane >= d) inc += o;
    }
    if (lane == GC_WAVE - 1) sm[wid] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < GC_SCAN_THREADS / GC_WAVE; q++) {
        const uint32_t s = sm[q];
        if (q < wid) before += s;
        tot += s;
    }
    __syncthreads(); /* sm is reused by the next call */
    *total = tot;
    return before + inc - v;
}

/* ---------------- rank: one workgroup per window ---------------- */

__global__ void k_gc_rank(const uint32_t *bits, uint32_t nw, const int32_t *dict_offsets,
                          uint32_t *prefix, uint32_t *nvals, unsigned long long *nbytes) {
    __shared__ uint32_t sm[GC_SCAN_THREADS / GC_WAVE];
    __shared__ unsigned long long sbytes;
    const uint32_t w = blockIdx.x;
    const uint32_t *wb = bits + (size_t)w * nw;
    uint32_t *wp = prefix + (size_t)w * nw;
    if (threadIdx.x == 0) sbytes = 0;
    __syncthreads();
    uint32_t carry = 0;
    unsigned long long local = 0;
    for (uint32_t b0 = 0; b0 < nw; b0 += GC_SCAN_THREADS) {
        const uint32_t j = b0 + threadIdx.x;
        uint32_t word = j < nw ? wb[j] : 0u;
        uint32_t tot;
        const uint32_t ex = gc_block_excl_scan(__popc(word), &tot, sm);
        if (j < nw) wp[j] = carry + ex;
        carry += tot;
        while (word) {
            const uint32_t k = j * 32u + (uint32_t)__builtin_ctz(word);
            word &= word - 1;
            local += (unsigned long long)(uint32_t)(dict_offsets[k + 1] - dict_offsets[k]);
        }
    }
    if (local) atomicAdd(&sbytes, local);
    __syncthreads();
    if (threadIdx.x == 0) {
        nvals[w] = carry;
        nbytes[w] = sbytes;
    }
}

/* ---------------- compact ---------------- */

/* surviving value lengths at their rank: offs[w][1 + rank] = len */
__global__ void k_gc_lens(const uint32_t *bits, const uint32_t *prefix, uint32_t nw,
                          uint64_t total_words, const int32_t *dict_offsets,
                          const int64_t *val_off, int32_t *offs) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total_words) return;
    uint32_t word = bits[g];
    if (!word) return;
    const uint64_t w = g / nw;
    const uint32_t j = (uint32_t)(g % nw);
    int32_t *o = offs + val_off[w] + (int64_t)w + 1 + prefix[g];
    while (word) {
        const uint32_t k = j * 32u + (uint32_t)__builtin_ctz(word);
        word &= word - 1;
        *o++ = dict_offsets[k + 1] - dict_offsets[k];
    }
}

/* per-window in-place scan: offs[w] = {0, inclusive scan of the lengths} */
__global__ void k_gc_scan_offs(const int64_t *val_off, int32_t *offs) {
    __shared__ uint32_t sm[GC_SCAN_THREADS / GC_WAVE];
    const int64_t w = blockIdx.x;
    int32_t *o = offs + val_off[w] + w;
    const int64_t nv = val_off[w + 1] - val_off[w];
    if (threadIdx.x == 0) o[0] = 0;
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < nv; b0 += GC_SCAN_THREADS) {
        const int64_t r = b0 + threadIdx.x;
        const uint32_t v = r < nv ? (uint32_t)o[1 + r] : 0u;
        uint32_t tot;
        const uint32_t ex = gc_block_excl_scan(v, &tot, sm);
        if (r < nv) o[1 + r] = (int32_t)(carry + ex + v);
        carry += tot;
    }
}

/* byte copy: one wave per bitmap word. Lane b < 32 loads value b's source offset, length
 * and destination offset (independent loads, no serial chain); then the whole wave copies
 * each surviving value (ascending indices are adjacent in source and destination) */
__global__ void k_gc_copy(const uint32_t *bits, const uint32_t *prefix, uint32_t nw,
                          uint64_t total_words, const int32_t *dict_offsets,
                          const uint8_t *dict_bytes, const int64_t *val_off,
                          const int64_t *byte_off, const int32_t *offs, uint8_t *out_bytes) {
    const int lane = threadIdx.x % GC_WAVE;
    const uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / GC_WAVE;
    if (g >= total_words) return; /* wave-uniform */
    const uint32_t word = __builtin_amdgcn_readfirstlane(bits[g]);
    if (!word) return;
    const uint64_t w = g / nw;
    const uint32_t j = (uint32_t)(g % nw);
    const int32_t *ow = offs + val_off[w] + (int64_t)w + prefix[g];
    uint8_t *dst = out_bytes + byte_off[w];
    int32_t s0 = 0, len = 0, d0 = 0;
    if (lane < 32 && ((word >> lane) & 1u)) {
        const uint32_t k = j * 32u + (uint32_t)lane;
        s0 = dict_offsets[k];
        len = dict_offsets[k + 1] - s0;
        d0 = ow[__popc(word & ((1u << lane) - 1u))];
    }
    uint32_t m = word;
    while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        const int32_t bs0 = __shfl(s0, b, GC_WAVE);
        const int32_t blen = __shfl(len, b, GC_WAVE);
        const int32_t bd0 = __shfl(d0, b, GC_WAVE);
        for (int32_t x = lane; x < blen; x += GC_WAVE) dst[bd0 + x] = dict_bytes[bs0 + x];
    }
}

/* ---------------- remap ---------------- */

template <bool LDS>
__global__ void k_gc_remap(const dd_gc_tile *tiles, const int32_t *idx, const uint8_t *valid,
                           uint32_t dict_n, uint32_t nw, const uint32_t *bits,
                           const uint32_t *prefix, int32_t *out) {
    const dd_gc_tile t = tiles[blockIdx.x];
    const uint32_t *wb = bits + (size_t)t.window * nw;
    const uint32_t *wp = prefix + (size_t)t.window * nw;
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < nw; j += blockDim.x) {
            gc_lds[j] = wb[j];
            gc_lds[nw + j] = wp[j];
        }
        __syncthreads();
    }
    for (int64_t i = t.row_lo + threadIdx.x; i < t.row_hi; i += blockDim.x) {
        const uint32_t k = (uint32_t)idx[i];
        int32_t r = 0;
        if ((!valid || valid[i]) && k < dict_n) {
            const uint32_t b = LDS ? gc_lds[k >> 5] : wb[k >> 5];
            const uint32_t p = LDS ? gc_lds[nw + (k >> 5)] : wp[k >> 5];
            r = (int32_t)(p + __popc(b & ((1u << (k & 31)) - 1u)));
        }
        out[i] = r;
    }
}

/* ---------------- rebase ---------------- */

/* out[i] = in[i + seg(i) * skew] + bases[seg(i)], seg_off[s] <= i < seg_off[s+1].
 * skew = 1 splices per-producer offsets arrays (n_s + 1 entries each) into one. */
__global__ void k_gc_rebase(const int32_t *in, int64_t n, const int64_t *seg_off,
                            const int32_t *bases, int32_t n_seg, int32_t skew, int32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    /* s = number of boundaries seg_off[1..n_seg-1] that are <= i */
    int32_t lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) / 2;
        if (seg_off[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    out[i] = in[i + (int64_t)lo * skew] + bases[lo];
}

/* ---------------- launchers ---------------- */

extern "C" {

hipError_t dd_launch_gc_mark(const dd_gc_tile *tiles, int64_t n_tiles, const int32_t *idx,
                             const uint8_t *valid, uint32_t dict_n, uint32_t nw, int lds,
                             uint32_t *bits, uint32_t *flag, hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (lds)
        hipLaunchKernelGGL(k_gc_mark<true>, dim3((unsigned)n_tiles), dim3(DD_GC_LDS_THREADS),
                           (size_t)nw * 4, s, tiles, idx, valid, dict_n, nw, bits, flag);
    else
        hipLaunchKernelGGL(k_gc_mark<false>, dim3((unsigned)n_tiles), dim3(DD_GC_GLB_THREADS),
                           0, s, tiles, idx, valid, dict_n, nw, bits, flag);
    return hipGetLastError();
}

hipError_t dd_launch_gc_rank(const uint32_t *bits, uint32_t n_windows, uint32_t nw,
                             const int32_t *dict_offsets, uint32_t *prefix, uint32_t *nvals,
                             uint64_t *nbytes, hipStream_t s) {
    hipLaunchKernelGGL(k_gc_rank, dim3(n_windows), dim3(GC_SCAN_THREADS), 0, s, bits, nw,
                       dict_offsets, prefix, nvals, (unsigned long long *)nbytes);
    return hipGetLastError();
}

hipError_t dd_launch_gc_compact(const uint32_t *bits, const uint32_t *prefix,
                                uint32_t n_windows, uint32_t nw, const int32_t *dict_offsets,
                                const uint8_t *dict_bytes, const int64_t *val_off,
                                const int64_t *byte_off, int32_t *offs, uint8_t *out_bytes,
                                hipStream_t s) {
    const uint64_t total_words = (uint64_t)n_windows * nw;
    if (total_words) {
        const unsigned blocks = (unsigned)((total_words + 255) / 256);
        hipLaunchKernelGGL(k_gc_lens, dim3(blocks), dim3(256), 0, s, bits, prefix, nw,
                           total_words, dict_offsets, val_off, offs);
    }
    hipLaunchKernelGGL(k_gc_scan_offs, dim3(n_windows), dim3(GC_SCAN_THREADS), 0, s, val_off,
                       offs);
    if (total_words) {
        const unsigned blocks = (unsigned)((total_words + 3) / 4); /* a wave per word */
        hipLaunchKernelGGL(k_gc_copy, dim3(blocks), dim3(4 * GC_WAVE), 0, s, bits, prefix, nw,
                           total_words, dict_offsets, dict_bytes, val_off, byte_off, offs,
                           out_bytes);
    }
    return hipGetLastError();
}

hipError_t dd_launch_gc_remap(const dd_gc_tile *tiles, int64_t n_tiles, const int32_t *idx,
                              const uint8_t *valid, uint32_t dict_n, uint32_t nw, int lds,
                              const uint32_t *bits, const uint32_t *prefix, int32_t *out,
                              hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (lds) {
        const size_t lds_bytes = (size_t)nw * 8;
        if (lds_bytes > 65536) {
            hipError_t e = hipFuncSetAttribute((const void *)k_gc_remap<true>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds_bytes);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_gc_remap<true>, dim3((unsigned)n_tiles), dim3(DD_GC_LDS_THREADS),
                           lds_bytes, s, tiles, idx, valid, dict_n, nw, bits, prefix, out);
    } else {
        hipLaunchKernelGGL(k_gc_remap<false>, dim3((unsigned)n_tiles),
                           dim3(DD_GC_GLB_THREADS), 0, s, tiles, idx, valid, dict_n, nw, bits,
                           prefix, out);
    }
    return hipGetLastError();
}

hipError_t dd_launch_gc_rebase(const int32_t *in, int64_t n, const int64_t *seg_off,
                               const int32_t *bases, int32_t n_seg, int32_t skew,
                               int32_t *out, hipStream_t s) {
    if (n <= 0 || n_seg <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_gc_rebase, dim3(blocks), dim3(256), 0, s, in, n, seg_off, bases,
                       n_seg, skew, out);
    return hipGetLastError();
}
}
