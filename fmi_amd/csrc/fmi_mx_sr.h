// fmi_mx_sr.h — stochastic rounding for the MX calls (fmi_dev_reduce_tree_mx_sr, fmi_dev_mx_quantize_sr,
// fmi_host_mx_quantize_sr; include/fmi_dev.h): the random bits and the rounding, one __host__ __device__ function each,
// shared by the fused kernels (fmi_mx_impl.h, fmi_mxfp4_impl.h), the quantize kernels (fmi_mx.hip) and the host call
// (fmi_mx_sr.hip). Plain C++: no conversion instruction of the target is used.
//
//   element i of a call has the stream position j = first + i; q = j >> 3
//   W = Philox4x32-10(counter (q lo, q hi, 0, 0), key (seed lo, seed hi));  r = 16 bits of W[(j & 7) >> 1], the low half
//   for an even j, the high half for an odd one: one Philox call serves 8 consecutive elements
//   narrow_sr(y, r): lo <= |y| < hi neighbours on the type's grid, T = 65536 (|y| - lo) / (hi - lo);
//                    the magnitude is hi if r + 0.5 < T, else lo; a grid value is never moved; the sign is y's
// The rounding, for finite |y| at most the largest finite element (what the MX scale rule guarantees), in f32
// operations every one of which is exact. With the type's (M, EMIN) and e the exponent of |y|, the grid step around |y|
// is 2^(max(e, EMIN) - M), a power of two:
//   t = |y| / step        one multiply by a power of two; 0 <= t < 2^(M + 1), and below EMIN t < 2^M
//   k = floor(t);  frac = t - k           lo = k * step;  T = 65536 * frac
//   up = (r + 0.5) * 2^-16 < frac         one fma on a 17-bit integer: r + 0.5 < T
// k + up is the result's significand at the exponent max(e, EMIN), and the magnitude code is
// ((max(e, EMIN) - EMIN) << M) + k + up: the implicit bit of a normal k carries the exponent field's 1, a carry out of it
// the next exponent, and below EMIN k is the subnormal code itself. tests/_mx_sr.py restates the same in integers (d =
// 23 - M + max(EMIN - e, 0); D = sig mod 2^d; up = ((2 r + 1) << (d - 17)) < D) and both against the exact form.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "fmi_kernels.h"

namespace fmi::dev {

struct Philox4 {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint64_t q, uint64_t seed) {
    uint32_t c0 = static_cast<uint32_t>(q), c1 = static_cast<uint32_t>(q >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1), c3 = static_cast<uint32_t>(p0), c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// r of the element at stream position j, from the Philox output of q = j >> 3.
__host__ __device__ __forceinline__ uint32_t sr_bits(const Philox4& W, uint64_t j) {
    const uint32_t k = static_cast<uint32_t>(j) & 7u;
    return (W.w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
}

// The magnitude code of narrow_sr(y, r) on the grid with M mantissa bits and the smallest normal exponent EMIN; r < 65536.
template <int M, int EMIN>
__host__ __device__ __forceinline__ uint32_t sr_magnitude(float y, uint32_t r) {
    constexpr uint32_t kMinExp = static_cast<uint32_t>(EMIN + 127) << 23;
    const uint32_t a = __builtin_bit_cast(uint32_t, y) & 0x7FFFFFFFu;
    const uint32_t eb = (a & 0x7F800000u) > kMinExp ? (a & 0x7F800000u) : kMinExp;  // 2^max(e, EMIN), as f32 bits
    const float t = __builtin_bit_cast(float, a) * __builtin_bit_cast(float, (static_cast<uint32_t>(254 + M) << 23) - eb);
    const float k = __builtin_floorf(t);
    const float frac = t - k;
    const float at = __builtin_fmaf(static_cast<float>(r), 0x1p-16f, 0x1p-17f);
    return (((eb - kMinExp) >> 23) << M) + static_cast<uint32_t>(k) + (at < frac ? 1u : 0u);
}

// The three element types: the code with y's sign bit (-0 included). E2M1: a nibble, sign in bit 3.
__host__ __device__ __forceinline__ uint32_t fp4_narrow_sr(float y, uint32_t r) {
    return sr_magnitude<1, 0>(y, r) | ((__builtin_bit_cast(uint32_t, y) >> 28) & 8u);
}
__host__ __device__ __forceinline__ uint32_t e4m3_narrow_sr(float y, uint32_t r) {
    return sr_magnitude<3, -6>(y, r) | ((__builtin_bit_cast(uint32_t, y) >> 24) & 0x80u);
}
__host__ __device__ __forceinline__ uint32_t e5m2_narrow_sr(float y, uint32_t r) {
    return sr_magnitude<2, -14>(y, r) | ((__builtin_bit_cast(uint32_t, y) >> 24) & 0x80u);
}

// The two 8-bit floats by their storage type (fmi_kernels.h).
template <class T>
__host__ __device__ __forceinline__ uint32_t fp8_narrow_sr(float y, uint32_t r) {
    static_assert(is_fp8_v<T>, "fp8_narrow_sr: f8e4m3 or f8e5m2");
    if constexpr (std::is_same_v<T, f8e5m2>)
        return e5m2_narrow_sr(y, r);
    else
        return e4m3_narrow_sr(y, r);
}

}  // namespace fmi::dev
