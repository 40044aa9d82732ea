// The kernels of the MX calls beside the fused ones (include/fmi_dev.h): fmi_dev_mx_quantize and fmi_dev_mx_dequantize,
// which are also what a fmi_dev_reduce_tree_mx call beyond the fused kernels (P = 1, P > 16, unaligned buckets) runs
// around the library's own FMI_F32 program.
//   dequantize   dst[i] = narrow_dst(fl32(widen(src[i]) * scale32(scales[i / 32])))
//   quantize     per block of 32: A = umax bits(|S|), e_out = mx_scale_byte(A), out = narrow(fl32(S * 2^(127 - e_out)))
// Any alignment: one element per thread and step, grid-stride; a block of 32 elements is one half of a wave, so its
// amax is five shuffles inside the half. The waves' loops are uniform (a wave leaves only when all its elements are
// beyond n), so every shuffle has all its lanes. These are the fallback's passes, not a hot path.
// FMI_F4E2M1 (two elements to a byte): one BYTE per thread and step, so nothing needs sub-byte addressing or atomics;
// a block of 32 elements is 16 threads, a quarter of a wave, and its amax four shuffles inside the quarter. Table
// widening and the integer-code narrowing of fmi_mxfp4_impl.h.
// fmi_dev_mx_quantize_sr, which is also what a fmi_dev_reduce_tree_mx_sr call beyond the fused kernels ends with, is the
// quantize kernels' SR instantiation: out = narrow_sr(fl32(S * 2^(127 - e_out)), r) (fmi_mx_sr.h).
// FMI_F6E2M3 / FMI_F6E3M2 (four elements to three bytes): FOUR elements, three whole bytes, per thread and step; a block
// of 32 elements is 8 threads and its amax three shuffles. The integer-code widening and narrowing of fmi_mxfp6_impl.h.
#include "fmi_mxfp4_impl.h"
#include "fmi_mxfp6_impl.h"

namespace fmi::dev {
namespace {

constexpr unsigned kBlock = 256;  // a multiple of 64: waves start on block boundaries
constexpr size_t kGridCap = size_t(1) << 20;

// T: the 8-bit storage type; D: float, _Float16 or __bf16.
template <class T, class D>
__global__ void __launch_bounds__(kBlock) mx_dequantize_kernel(D* dst, const T* src, const uint8_t* scales, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        Lanes<float, 1> v;
        v.v[0] = fp8_widen(src[i]) * mx_scale32(scales[i / 32]);
        dst[i] = to_storage<D>(v).v[0];
    }
}

// What a stochastic-rounding quantize kernel takes beside the round-to-nearest one's arguments: the device word that
// holds the Philox key and the stream position of element 0. The kernels take it as a parameter pack SR..., empty for
// round to nearest (an unused argument, even an empty struct, would move that kernel's hidden arguments).
struct SrStream {
    const uint64_t* seed;
    uint64_t first;
};

// SR: narrow_sr (fmi_mx_sr.h) where the round-to-nearest kernel narrows. A thread runs the Philox call of its element's
// group of 8 and keeps 16 bits of it.
template <class T, class S, class... SR>
__global__ void __launch_bounds__(kBlock) mx_quantize_kernel(T* out, uint8_t* out_scales, const S* src, size_t n, SR... sr) {
    constexpr bool kSr = sizeof...(SR) != 0;
    const SrStream stream{sr...};
    uint64_t seed = 0;
    if constexpr (kSr) seed = *stream.seed;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const unsigned lane = threadIdx.x % 64;
    // `wave0`: the first element of this wave's 64 (two blocks); the loop's condition is the wave's, not the lane's
    for (size_t wave0 = static_cast<size_t>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); wave0 < n; wave0 += stride) {
        const size_t i = wave0 + lane;
        const bool have = i < n;
        float x = 0.0f;
        if (have) {
            Lanes<S, 1> raw;
            raw.v[0] = src[i];
            x = to_value<float>(raw).v[0];
        }
        uint32_t A = mx_abs_bits(x);  // 0 beyond the bucket
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
        const uint32_t e_out = mx_scale_byte<T>(A);
        const float y = x * mx_inv_scale(e_out);
        if (have) {
            if constexpr (kSr) {
                const uint64_t j = stream.first + i;
                const uint32_t code = fp8_narrow_sr<T>(y, sr_bits(philox4x32_10(j >> 3, seed), j));
                out[i] = T{static_cast<uint8_t>(e_out == 255u ? 0x7Fu : code)};
            } else {
                out[i] = e_out == 255u ? T{0x7F} : fp8_narrow<T>(y);
            }
            if (lane % 32 == 0) out_scales[i / 32] = static_cast<uint8_t>(e_out);
        }
    }
}

// n: elements; the bucket is n / 2 + n % 2 bytes, and the last byte's high nibble is not an element when n is odd.
template <class D>
__global__ void __launch_bounds__(kBlock) mxfp4_dequantize_kernel(D* dst, const uint8_t* src, const uint8_t* scales, size_t n) {
    const size_t nbytes = n / 2 + n % 2;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nbytes; i += stride) {
        const uint32_t b = src[i];
        const float sc = mx_scale32(scales[i / 16]);
        Lanes<float, 1> v;
        v.v[0] = fp4_widen_sw(b) * sc;
        dst[2 * i] = to_storage<D>(v).v[0];
        if (2 * i + 1 < n) {
            v.v[0] = fp4_widen_sw(b >> 4) * sc;
            dst[2 * i + 1] = to_storage<D>(v).v[0];
        }
    }
}

// SR: as mx_quantize_kernel's; a byte's elements 2 i and 2 i + 1 lie in one Philox group because `first` is even.
template <class S, class... SR>
__global__ void __launch_bounds__(kBlock) mxfp4_quantize_kernel(uint8_t* out, uint8_t* out_scales, const S* src, size_t n, SR... sr) {
    constexpr bool kSr = sizeof...(SR) != 0;
    const SrStream stream{sr...};
    uint64_t seed = 0;
    if constexpr (kSr) seed = *stream.seed;
    const size_t nbytes = n / 2 + n % 2;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const unsigned lane = threadIdx.x % 64;
    // `wave0`: the first byte of this wave's 64 (four blocks); the loop's condition is the wave's, not the lane's
    for (size_t wave0 = static_cast<size_t>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); wave0 < nbytes; wave0 += stride) {
        const size_t i = wave0 + lane;
        float x[2] = {0.0f, 0.0f};  // beyond the bucket: +0, whose code 0 is what an odd bucket's last high nibble takes
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (2 * i + k < n) {
                Lanes<S, 1> raw;
                raw.v[0] = src[2 * i + k];
                x[k] = to_value<float>(raw).v[0];
            }
        uint32_t A = max(mx_abs_bits(x[0]), mx_abs_bits(x[1]));
#pragma unroll
        for (int d = 8; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
        const uint32_t e_out = mxfp4_scale_byte(A);
        const float inv = mx_inv_scale(e_out);
        if (i < nbytes) {
            uint32_t b;
            if constexpr (kSr) {
                const uint64_t j = stream.first + 2 * i;  // even: j and j + 1 share the word (j & 7) >> 1 of one Philox group
                const uint32_t w = philox4x32_10(j >> 3, seed).w[(static_cast<uint32_t>(j) & 7u) >> 1];
                const uint32_t hi = 2 * i + 1 < n ? fp4_narrow_sr(x[1] * inv, w >> 16) : 0u;  // an odd bucket's last high nibble: 0
                b = e_out == 255u ? 0u : fp4_narrow_sr(x[0] * inv, w & 0xFFFFu) | (hi << 4);
            } else {
                b = e_out == 255u ? 0u : fp4_narrow_sw(x[0] * inv) | (fp4_narrow_sw(x[1] * inv) << 4);
            }
            out[i] = static_cast<uint8_t>(b);
            if (lane % 16 == 0) out_scales[i / 16] = static_cast<uint8_t>(e_out);
        }
    }
}

// The 6-bit floats, M as in fmi_mxfp6_impl.h. n: elements; the bucket is ceil(3 n / 4) bytes. A thread takes FOUR
// elements, three whole bytes, so nothing is sub-byte shared; the last thread of a ragged bucket reads and writes only
// the bytes the bucket has, and the bits of the last byte beyond element n - 1 are ignored.
template <int M, class D>
__global__ void __launch_bounds__(kBlock) mxfp6_dequantize_kernel(D* dst, const uint8_t* src, const uint8_t* scales, size_t n) {
    const size_t nquad = n / 4 + (n % 4 != 0), nbytes = n / 4 * 3 + (n % 4 * 3 + 3) / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nquad; i += stride) {
        uint32_t three = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (3 * i + k < nbytes) three |= static_cast<uint32_t>(src[3 * i + k]) << (8 * k);
        const float sc = mx_scale32(scales[i / 8]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * i + k < n) {
                Lanes<float, 1> v;
                v.v[0] = fp6_widen_sw<M>(three >> (6 * k)) * sc;
                dst[4 * i + k] = to_storage<D>(v).v[0];
            }
    }
}

// SR: as mx_quantize_kernel's; a thread's elements 4 i .. 4 i + 3 lie in one Philox group because `first` is a multiple of 4.
template <int M, class S, class... SR>
__global__ void __launch_bounds__(kBlock) mxfp6_quantize_kernel(uint8_t* out, uint8_t* out_scales, const S* src, size_t n, SR... sr) {
    constexpr bool kSr = sizeof...(SR) != 0;
    const SrStream stream{sr...};
    uint64_t seed = 0;
    if constexpr (kSr) seed = *stream.seed;
    const size_t nquad = n / 4 + (n % 4 != 0), nbytes = n / 4 * 3 + (n % 4 * 3 + 3) / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const unsigned lane = threadIdx.x % 64;
    // `wave0`: the first quad of this wave's 64 (eight blocks); the loop's condition is the wave's, not the lane's
    for (size_t wave0 = static_cast<size_t>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); wave0 < nquad; wave0 += stride) {
        const size_t i = wave0 + lane;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // beyond the bucket: +0, whose code 0 is what the last byte's unused bits take
        uint32_t A = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (4 * i + k < n) {
                Lanes<S, 1> raw;
                raw.v[0] = src[4 * i + k];
                x[k] = to_value<float>(raw).v[0];
            }
            A = max(A, mx_abs_bits(x[k]));
        }
#pragma unroll
        for (int d = 4; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
        const uint32_t e_out = mxfp6_scale_byte<M>(A);
        const float inv = mx_inv_scale(e_out);
        if (i < nquad) {
            uint32_t c[4];
            Philox4 W{};
            if constexpr (kSr) W = philox4x32_10((stream.first + 4 * i) >> 3, seed);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (kSr)
                    c[k] = 4 * i + k < n ? fp6_narrow_sr<M>(x[k] * inv, sr_bits(W, stream.first + 4 * i + k)) : 0u;
                else
                    c[k] = fp6_narrow_sw<M>(x[k] * inv);
            }
            const uint32_t three = e_out == 255u ? 0u : fp6_pack4(c[0], c[1], c[2], c[3]);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (3 * i + k < nbytes) out[3 * i + k] = static_cast<uint8_t>(three >> (8 * k));
            if (lane % 8 == 0) out_scales[i / 8] = static_cast<uint8_t>(e_out);
        }
    }
}

unsigned grid_of(size_t n) { return static_cast<unsigned>(std::min(grid_for(n, kBlock), kGridCap)); }

// f.template operator()<D>() for the non-MX side of a conversion: FMI_F32, FMI_F16 or FMI_BF16.
template <class F>
int with_wide_dtype(const char* who, const char* what, int dtype, F&& f) {
    switch (dtype) {
        case FMI_F32: return f.template operator()<float>();
        case FMI_F16: return f.template operator()<_Float16>();
        case FMI_BF16: return f.template operator()<__bf16>();
        default:
            return fail(FMI_ERR_INVALID, std::string(who) + ": " + what + " " + std::to_string(dtype) + " must be FMI_F32, FMI_F16 or FMI_BF16");
    }
}

// fmi_dev_mx_quantize (no sr) and fmi_dev_mx_quantize_sr (one SrStream), `who` in their messages.
template <class... SR>
int quantize(const char* who, int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, hipStream_t s, SR... sr) {
    constexpr bool kSr = sizeof...(SR) != 0;
    if (n == 0) return FMI_OK;
    if (is_fp6_dtype(dtype))
        return with_wide_dtype(who, "src_dtype", src_dtype, [&]<class S>() -> int {
            const unsigned grid = grid_of(n / 4 + (n % 4 != 0));
            if (dtype == FMI_F6E2M3)
                mxfp6_quantize_kernel<3><<<grid, kBlock, 0, s>>>(static_cast<uint8_t*>(out), out_scales, static_cast<const S*>(src), n, sr...);
            else
                mxfp6_quantize_kernel<2><<<grid, kBlock, 0, s>>>(static_cast<uint8_t*>(out), out_scales, static_cast<const S*>(src), n, sr...);
            return check_launch(kSr ? "MXFP6 stochastic-rounding quantize kernel launch" : "MXFP6 quantize kernel launch");
        });
    if (dtype == FMI_F4E2M1)
        return with_wide_dtype(who, "src_dtype", src_dtype, [&]<class S>() -> int {
            mxfp4_quantize_kernel<<<grid_of(n / 2 + n % 2), kBlock, 0, s>>>(static_cast<uint8_t*>(out), out_scales, static_cast<const S*>(src), n,
                                                                           sr...);
            return check_launch(kSr ? "MXFP4 stochastic-rounding quantize kernel launch" : "MXFP4 quantize kernel launch");
        });
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        return with_wide_dtype(who, "src_dtype", src_dtype, [&]<class S>() -> int {
            mx_quantize_kernel<<<grid_of(n), kBlock, 0, s>>>(static_cast<T*>(out), out_scales, static_cast<const S*>(src), n, sr...);
            return check_launch(kSr ? "MX stochastic-rounding quantize kernel launch" : "MX quantize kernel launch");
        });
    });
}

}  // namespace

int launch_mx_dequantize(int dst_dtype, void* dst, int dtype, const void* src, const uint8_t* scales, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    if (is_fp6_dtype(dtype))
        return with_wide_dtype("fmi_dev_mx_dequantize", "dst_dtype", dst_dtype, [&]<class D>() -> int {
            const unsigned grid = grid_of(n / 4 + (n % 4 != 0));
            if (dtype == FMI_F6E2M3)
                mxfp6_dequantize_kernel<3, D><<<grid, kBlock, 0, s>>>(static_cast<D*>(dst), static_cast<const uint8_t*>(src), scales, n);
            else
                mxfp6_dequantize_kernel<2, D><<<grid, kBlock, 0, s>>>(static_cast<D*>(dst), static_cast<const uint8_t*>(src), scales, n);
            return check_launch("MXFP6 dequantize kernel launch");
        });
    if (dtype == FMI_F4E2M1)
        return with_wide_dtype("fmi_dev_mx_dequantize", "dst_dtype", dst_dtype, [&]<class D>() -> int {
            mxfp4_dequantize_kernel<D><<<grid_of(n / 2 + n % 2), kBlock, 0, s>>>(static_cast<D*>(dst), static_cast<const uint8_t*>(src), scales, n);
            return check_launch("MXFP4 dequantize kernel launch");
        });
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        return with_wide_dtype("fmi_dev_mx_dequantize", "dst_dtype", dst_dtype, [&]<class D>() -> int {
            mx_dequantize_kernel<T, D><<<grid_of(n), kBlock, 0, s>>>(static_cast<D*>(dst), static_cast<const T*>(src), scales, n);
            return check_launch("MX dequantize kernel launch");
        });
    });
}

int launch_mx_quantize(int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, hipStream_t s) {
    return quantize("fmi_dev_mx_quantize", dtype, out, out_scales, src_dtype, src, n, s);
}

int launch_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, const uint64_t* seed,
                          uint64_t first, hipStream_t s) {
    return quantize("fmi_dev_mx_quantize_sr", dtype, out, out_scales, src_dtype, src, n, s, SrStream{seed, first});
}

}  // namespace fmi::dev
