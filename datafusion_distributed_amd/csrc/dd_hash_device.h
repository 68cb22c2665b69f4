/* dd_hash_device.h — device-side normative hash, shared by the shuffle
 * kernels (dd_kernels.hip) and the partial-reduce kernel (dd_reduce.hip). Must match
 * oracle/dd_oracle.c bit-exactly. */

#ifndef DD_HASH_DEVICE_H
#define DD_HASH_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_internal.h"

/* ---------------- normative hash (must match oracle/dd_oracle.c bit-exactly) ------------ */

__device__ __forceinline__ uint64_t dd_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint64_t dd_hash_bytes_dev(const uint8_t *p, int64_t len) {
    uint64_t h = 0x9e3779b97f4a7c15ULL ^ ((uint64_t)len * 0xff51afd7ed558ccdULL);
    int64_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t c;
        /* gfx950 supports unaligned wide loads: this lowers to global_load_dwordx2 */
        __builtin_memcpy(&c, p + i, 8);
        h = dd_mix64(h ^ c);
    }
    if (i < len) {
        uint64_t c = 0;
        for (int64_t b = 0; b < len - i; b++) c |= (uint64_t)p[i + b] << (8 * b);
        h = dd_mix64(h ^ c);
    }
    return h;
}

__device__ __forceinline__ uint64_t dd_canon_f64_dev(double v) {
    if (v == 0.0) v = 0.0;
    uint64_t b = __double_as_longlong(v);
    if (v != v) b = 0x7ff8000000000000ULL;
    return b;
}

__device__ __forceinline__ uint64_t dd_canon_f32_dev(float v) {
    if (v == 0.0f) v = 0.0f;
    uint32_t b = __float_as_uint(v);
    if (v != v) b = 0x7fc00000u;
    return (uint64_t)b;
}

/* value hash of a valid row (column described by a dd_kcol) */
__device__ __forceinline__ uint64_t dd_value_hash_dev(const dd_kcol &c, int64_t i) {
    switch (c.dtype) {
    case DD_KDT_U8:
    case DD_KDT_BOOL: /* unpacked u8 0/1 hashes like u8 (oracle dd_value_hash) */
        return dd_mix64((uint64_t)((const uint8_t *)c.data)[i]);
    case DD_KDT_I16:
        return dd_mix64((uint64_t)((const uint16_t *)c.data)[i]);
    case DD_KDT_I32:
        return dd_mix64((uint64_t)((const uint32_t *)c.data)[i]);
    case DD_KDT_I64:
        return dd_mix64(((const uint64_t *)c.data)[i]);
    case DD_KDT_F32:
        return dd_mix64(dd_canon_f32_dev(((const float *)c.data)[i]));
    case DD_KDT_F64:
        return dd_mix64(dd_canon_f64_dev(((const double *)c.data)[i]));
    case DD_KDT_UTF8: {
        int32_t o0 = c.offsets[i], o1 = c.offsets[i + 1];
        return dd_hash_bytes_dev((const uint8_t *)c.data + o0, (int64_t)(o1 - o0));
    }
    case DD_KDT_DICT32: {
        int32_t k = ((const int32_t *)c.data)[i];
        return c.dict_hashes[k]; /* precomputed by k_dict_hashes */
    }
    default:
        return 0;
    }
}


/* one 16-byte value (dec128 and its layout kin): x = lo = bytes 0..7, y = hi = bytes
 * 8..15. A native vector, so a load or store of it is one 128-bit access */
typedef uint64_t dd_u128 __attribute__((ext_vector_type(2)));

/* §3.1's comb */
__device__ __forceinline__ uint64_t dd_hash_comb(uint64_t h, uint64_t vh) {
    return h ^ (vh + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2));
}

/* row hash over the key columns; create_hashes restatement.
 * DEC128 = false: for callers whose host gate admits no dec128 key (the pre-path K1 kernels,
 * the partial reduce); they compile to what they were before the dtype existed. */
template <bool DEC128 = true>
__device__ __forceinline__ uint64_t dd_row_hash(const dd_kargs &a, int64_t i) {
    uint64_t h = 0;
    for (int k = 0; k < a.n_keys; k++) {
        const dd_kcol &c = a.cols[a.key_idx[k]];
        if (c.valid && !c.valid[i]) continue;
        if (DEC128 && c.dtype == DD_KDT_DEC128) {
            /* §16: hashes as the two i64 keys (lo, hi) in that order; one 16-byte load
             * (the host checks the alignment) */
            const dd_u128 v = ((const dd_u128 *)c.data)[i];
            h = dd_hash_comb(h, dd_mix64(v.x));
            h = dd_hash_comb(h, dd_mix64(v.y));
            continue;
        }
        uint64_t vh = dd_value_hash_dev(c, i);
        h = dd_hash_comb(h, vh);
    }
    return h;
}

/* ---------------- K1 with a compile-time key signature ----------------
 * dd_row_hash walks a.n_keys at run time and switches on the dtype per row, so a K1 loop
 * "unrolled over G row groups" compiles to G copies of load -> wait -> hash -> store: one
 * key load in flight per lane. With the signature (the kinds of one or two NON-NULLABLE
 * fixed-width key columns) known at compile time the body is straight-line code and every
 * key load of every group issues before the first wait. The host picks the signature once
 * (dd_partitioner_create; dd_partitioner_k1_spec reports it); everything it does not
 * whitelist keeps dd_row_hash. Kinds and codes: DD_KK_* / DD_K1_CODE in dd_internal.h. */

template <int K> struct dd_kk_raw { using T = uint8_t; };
template <> struct dd_kk_raw<DD_KK_B2> { using T = uint16_t; };
template <> struct dd_kk_raw<DD_KK_B4> { using T = uint32_t; };
template <> struct dd_kk_raw<DD_KK_B8> { using T = uint64_t; };
template <> struct dd_kk_raw<DD_KK_F32> { using T = float; };
template <> struct dd_kk_raw<DD_KK_F64> { using T = double; };
template <> struct dd_kk_raw<DD_KK_DICT32> { using T = int32_t; };

/* value hash of a loaded key element (dict32: v is the index, gathered by the caller) */
template <int K>
__device__ __forceinline__ uint64_t dd_kk_hash(typename dd_kk_raw<K>::T v) {
    if constexpr (K == DD_KK_F32) return dd_mix64(dd_canon_f32_dev(v));
    else if constexpr (K == DD_KK_F64) return dd_mix64(dd_canon_f64_dev(v));
    else return dd_mix64((uint64_t)v); /* unsigned raw types: zero-extended, as the oracle */
}

/* K1 work of G row groups: rows row0 + g * stride, g < G, those below `end` active
 * (end > 0; at least the caller's first row is below it). Order: clamp -> all key loads ->
 * dict32 gathers -> hashes -> pid rule -> pid stores -> LDS counts. An inactive lane
 * loads row end - 1 (as k_scatter_pre::preload clamps), so no load sits under a branch. */
template <int K0, int K1, int G>
__device__ __forceinline__ void dd_k1_spec_groups(const dd_kargs &a, int64_t row0,
                                                  int64_t stride, int64_t end,
                                                  uint32_t *pid_out, uint32_t *hist) {
    using T0 = typename dd_kk_raw<K0>::T;
    using T1 = typename dd_kk_raw<K1>::T;
    constexpr bool TWO = K1 != DD_KK_NONE;
    const dd_kcol &c0 = a.cols[a.key_idx[0]];
    const dd_kcol &c1 = a.cols[a.key_idx[TWO ? 1 : 0]];
    const T0 *__restrict__ d0 = (const T0 *)c0.data;
    const T1 *__restrict__ d1 = (const T1 *)c1.data;

    int64_t row[G], crow[G];
    bool act[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        row[g] = row0 + g * stride;
        act[g] = row[g] < end;
        crow[g] = act[g] ? row[g] : end - 1;
    }
    T0 r0[G];
    T1 r1[G];
#pragma unroll
    for (int g = 0; g < G; g++) r0[g] = d0[crow[g]];
    if constexpr (TWO) {
#pragma unroll
        for (int g = 0; g < G; g++) r1[g] = d1[crow[g]];
    }
    /* nothing moves across: left alone, the scheduler hoists the first group's hash (and
     * with it a wait) above the later groups' loads */
    __builtin_amdgcn_sched_barrier(0);
    uint64_t v0[G], v1[G];
    if constexpr (K0 == DD_KK_DICT32) {
        const uint64_t *__restrict__ dh = c0.dict_hashes;
#pragma unroll
        for (int g = 0; g < G; g++) v0[g] = dh[r0[g]];
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (int g = 0; g < G; g++) v0[g] = dd_kk_hash<K0>(r0[g]);
    }
    if constexpr (TWO) {
        static_assert(K1 != DD_KK_DICT32, "dict32 is instantiated as a single key only");
#pragma unroll
        for (int g = 0; g < G; g++) v1[g] = dd_kk_hash<K1>(r1[g]);
    }
    /* dd_row_hash's combine; its first step from h = 0 is vh + golden */
    uint64_t h[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        h[g] = v0[g] + 0x9e3779b97f4a7c15ULL;
        if constexpr (TWO)
            h[g] = h[g] ^ (v1[g] + 0x9e3779b97f4a7c15ULL + (h[g] << 6) + (h[g] >> 2));
    }
    /* pid = (h % pid_total) >> pid_shift */
    const uint32_t tot = a.pid_total;
    uint32_t pid[G];
    if ((tot & (tot - 1)) == 0) {
#pragma unroll
        for (int g = 0; g < G; g++) pid[g] = (uint32_t)(h[g] & (uint64_t)(tot - 1));
    } else {
#pragma unroll
        for (int g = 0; g < G; g++) pid[g] = (uint32_t)(h[g] % (uint64_t)tot);
    }
#pragma unroll
    for (int g = 0; g < G; g++) pid[g] >>= a.pid_shift;
    if (a.pid8) {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (act[g]) ((uint8_t *)pid_out)[row[g]] = (uint8_t)pid[g];
    } else {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (act[g]) pid_out[row[g]] = pid[g];
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (act[g]) atomicAdd(&hist[pid[g]], 1u);
}

/* one K1 iteration of a wave segment or block tile: 4 groups, or 2 where no more than two
 * groups' worth of rows is left (the SEG = 128 tiers; a short tail) */
template <int K0, int K1>
__device__ __forceinline__ void dd_k1_spec_iter(const dd_kargs &a, int64_t base, int lane,
                                                int64_t stride, int64_t end,
                                                uint32_t *pid_out, uint32_t *hist) {
    /* wave-uniform in every caller; said so, the choice is a scalar branch */
    if (__builtin_amdgcn_readfirstlane((int)(end - base <= 2 * stride)))
        dd_k1_spec_groups<K0, K1, 2>(a, base + lane, stride, end, pid_out, hist);
    else
        dd_k1_spec_groups<K0, K1, 4>(a, base + lane, stride, end, pid_out, hist);
}

/* ballot-multisplit: lanes with equal pid (among `act`); returns the equal-mask */
__device__ __forceinline__ uint64_t dd_eq_mask(uint32_t pid, uint64_t act, int nbits) {
    uint64_t eq = act;
    for (int b = 0; b < nbits; b++) {
        uint64_t bal = __ballot((pid >> b) & 1u);
        eq &= ((pid >> b) & 1u) ? bal : ~bal;
    }
    return eq;
}


#endif /* DD_HASH_DEVICE_H */
