// Device helpers shared by the R1CS check (check.hip) and the QAP witness map (qap.hip): witness gathers and the
// linear combinations <L, w> over the loader's factor stream (r1cs_internal.hpp).  A general factor is one Montgomery
// product with its coefficient c * R, so the sum is c * w for a canonical row and c * w * R for a Montgomery row.
#pragma once
#include <hip/hip_runtime.h>

#include "r1cs_internal.hpp"

namespace cwc_r1cs {

using cwc::Fr;

__device__ __forceinline__ Fr load_elem(const uint8_t* row, uint32_t wire) {
    const uint4* p = reinterpret_cast<const uint4*>(row + (size_t)wire * 32);
    const uint4 lo = p[0], hi = p[1];
    return Fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}

// w mod r for any w < 2^256 (rare: rows from the witness calculator are already below r)
__device__ __forceinline__ Fr reduce_any(Fr w) {
    if (!cwc::u256_lt(w, cwc::fr_p())) {
        const Fr one{{1, 0, 0, 0, 0, 0, 0, 0}};
        w = cwc::fr_mul(cwc::fr_mul(w, cwc::fr_r2()), one);  // (w R) / R
    }
    return w;
}

__device__ __forceinline__ Fr accumulate(const Fr& acc, Fr w, uint32_t kind, const Fr* __restrict__ coef, uint32_t ci) {
    if (kind == KIND_GENERAL) return cwc::fr_add(acc, cwc::fr_mul(w, coef[ci]));  // w may be any value below 2^256 as the first operand
    w = reduce_any(w);
    return kind == KIND_PLUS ? cwc::fr_add(acc, w) : cwc::fr_sub(acc, w);
}

// Four factors at a time: their four witness gathers are in flight together before the arithmetic that needs the first.
__device__ __forceinline__ Fr lin_comb(const uint32_t* __restrict__ fac, const uint32_t* __restrict__ cidx, const Fr* __restrict__ coef,
                                       uint32_t k, uint32_t end, const uint8_t* row) {
    constexpr int U = 4;
    Fr acc = cwc::fr_zero();
    for (; k + U <= end; k += U) {
        uint32_t f[U];
        Fr w[U];
#pragma unroll
        for (int i = 0; i < U; ++i) f[i] = fac[k + i];
#pragma unroll
        for (int i = 0; i < U; ++i) w[i] = load_elem(row, f[i] & WIRE_MASK);
#pragma unroll
        for (int i = 0; i < U; ++i) acc = accumulate(acc, w[i], f[i] >> 30, coef, cidx[k + i]);
    }
    for (; k < end; ++k) {
        const uint32_t f = fac[k];
        acc = accumulate(acc, load_elem(row, f & WIRE_MASK), f >> 30, coef, cidx[k]);
    }
    return acc;
}

}  // namespace cwc_r1cs
