// qc_pk_ops.h — two codewords per register as an fp16 pair: the packed idioms shared by the quantized min-sum
// kernels (qc_pk.hip flooding, qc_lay_pk.hip layered).  Every value is a small integer, so fp16 arithmetic on them
// is exact (the argument at the head of qc_pk.hip).
#pragma once
#include "qc_common.h"

#include <cstdint>

namespace ldpc {

using h2 = _Float16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 as_h2(uint32_t x) { return __builtin_bit_cast(h2, x); }
__device__ __forceinline__ uint32_t as_u(h2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t pmin(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_h2(a), as_h2(b))); }
__device__ __forceinline__ uint32_t pmax(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_h2(a), as_h2(b))); }
__device__ __forceinline__ uint32_t padd(uint32_t a, uint32_t b) { return as_u(as_h2(a) + as_h2(b)); }
__device__ __forceinline__ uint32_t psub(uint32_t a, uint32_t b) { return as_u(as_h2(a) - as_h2(b)); }
__device__ __forceinline__ uint32_t pbperm(int addr, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v); }
__device__ __forceinline__ uint32_t pk2(float lo, float hi) { return as_u(h2{(_Float16)lo, (_Float16)hi}); }
constexpr uint32_t kSign2 = 0x80008000u, kMag2 = 0x7fff7fffu;

// three-input packed minimum (v_pk_minimum3_f16, gfx950): IEEE minimum, the same as min on these operands
// (no NaN; magnitudes carry +0 only)
__device__ __forceinline__ uint32_t pmin3(uint32_t a, uint32_t b, uint32_t c) {
    return as_u(__builtin_elementwise_minimum(__builtin_elementwise_minimum(as_h2(a), as_h2(b)), as_h2(c)));
}
// the two smallest of D packed non-negative magnitudes (each result is one of the inputs, bit for bit), over edge
// pairs with v_pk_minimum3_f16 (5 VALU per 2 edges instead of 6): per pair (x, y) with lo/hi = min/max(x, y): the new second minimum of {mn1 <= mn2, x, y} is
// min(mn2, hi, max(mn1, lo)) (lo < mn1: min(mn1, hi); else min(mn2, lo)), the new minimum min(mn1, lo).
template <int D>
__device__ __forceinline__ void two_min_pk(const uint32_t (&a)[D], uint32_t& mn1, uint32_t& mn2) {
    static_assert(D >= 2, "packed min-sum: check degree >= 2");
    mn1 = pmin(a[0], a[1]);
    mn2 = pmax(a[0], a[1]);
    static_for<0, (D - 2) / 2>([&](auto pp) __attribute__((always_inline)) {
        constexpr int t = 2 + 2 * decltype(pp)::value;
        const uint32_t lo = pmin(a[t], a[t + 1]), hi = pmax(a[t], a[t + 1]);
        mn2 = pmin3(mn2, hi, pmax(mn1, lo));
        mn1 = pmin(mn1, lo);
    });
    if constexpr (D % 2 == 1) {
        mn2 = pmin(mn2, pmax(mn1, a[D - 1]));
        mn1 = pmin(mn1, a[D - 1]);
    }
}

template <int D>
__device__ __forceinline__ uint32_t xor_all_u(const uint32_t (&v)[D]) {
    uint32_t t = v[0];
    static_for<0, (D - 1) / 2>([&](auto pp) __attribute__((always_inline)) {
        constexpr int k = 1 + 2 * decltype(pp)::value;
        t = __builtin_amdgcn_bitop3_b32(t, v[k], v[k + 1], 0x96);
    });
    if constexpr ((D - 1) % 2) t ^= v[D - 1];
    return t;
}

}  // namespace ldpc
