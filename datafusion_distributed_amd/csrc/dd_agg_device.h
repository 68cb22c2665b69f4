/* dd_agg_device.h — device helpers shared by the partial aggregate (dd_reduce.hip) and the
 * final merge above the shuffle (dd_final.hip): the order-preserving u64 keys behind
 * min / max, the op identities and the canonical key bits of a group identity. */

#ifndef DD_AGG_DEVICE_H
#define DD_AGG_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dd_internal.h"

/* order-preserving f64 <-> u64 map (IEEE-754 totalOrder on the bit pattern: a sign-clear
 * NaN sorts above +inf, a sign-set NaN below -inf): sign clear -> bits | sign,
 * sign set -> ~bits */
__device__ __forceinline__ uint64_t dd_f64_key(double v) {
    uint64_t b = __double_as_longlong(v);
    return (b & 0x8000000000000000ULL) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double dd_f64_unkey(uint64_t k) {
    uint64_t b = (k & 0x8000000000000000ULL) ? (k & 0x7fffffffffffffffULL) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ uint64_t dd_i64_key(int64_t v) {
    return (uint64_t)v ^ 0x8000000000000000ULL; /* order-preserving signed -> unsigned */
}
__device__ __forceinline__ int64_t dd_i64_unkey(uint64_t k) {
    return (int64_t)(k ^ 0x8000000000000000ULL);
}

__device__ __forceinline__ unsigned long long dd_agg_identity(int op) {
    switch (op) {
    case DD_AGG_SUM_F64: return (unsigned long long)__double_as_longlong(0.0);
    case DD_AGG_MIN_F64:
    case DD_AGG_MIN_I64: return ~0ULL; /* min over mapped-u64 keys */
    case DD_AGG_MAX_F64:
    case DD_AGG_MAX_I64: return 0ULL;
    default: return 0ULL; /* COUNT / SUM_I64 */
    }
}

/* canonical 64-bit key bits (zero-extended; floats canonicalized like the hash) */
__device__ __forceinline__ uint64_t dd_key_bits(const dd_kcol &c, int64_t i) {
    switch (c.dtype) {
    case DD_KDT_U8:
    case DD_KDT_BOOL:
        return (uint64_t)((const uint8_t *)c.data)[i];
    case DD_KDT_I16:
        return (uint64_t)((const uint16_t *)c.data)[i];
    case DD_KDT_I32:
        return (uint64_t)((const uint32_t *)c.data)[i];
    case DD_KDT_I64:
        return ((const uint64_t *)c.data)[i];
    case DD_KDT_F32: {
        float v = ((const float *)c.data)[i];
        if (v == 0.0f) v = 0.0f;
        uint32_t b = __float_as_uint(v);
        if (v != v) b = 0x7fc00000u;
        return (uint64_t)b;
    }
    case DD_KDT_F64: {
        double v = ((const double *)c.data)[i];
        if (v == 0.0) v = 0.0;
        uint64_t b = __double_as_longlong(v);
        if (v != v) b = 0x7ff8000000000000ULL;
        return b;
    }
    case DD_KDT_DICT32:
        /* group by dictionary INDEX: within one batch the dict is shared, so equal
         * indices == equal values; duplicate values under different indices would only
         * split a group, which partial aggregation permits (merged downstream by value) */
        return (uint64_t)(uint32_t)((const int32_t *)c.data)[i];
    default:
        return 0;
    }
}

#endif /* DD_AGG_DEVICE_H */
