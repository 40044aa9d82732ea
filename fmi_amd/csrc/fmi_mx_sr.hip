// The stochastic-rounding MX calls beside the fused kernels (include/fmi_dev.h): fmi_dev_mx_quantize_sr's kernels, which
// are also what a fmi_dev_reduce_tree_mx_sr call beyond the fused kernels (P = 1, P > 16, unaligned buckets) ends with,
// and fmi_host_mx_quantize_sr, the same quantization on host memory.
//   per block of 32: A = umax bits(|S|), e_out = the block's scale byte, out = narrow_sr(fl32(S * 2^(127 - e_out)), r)
// The kernels are mx_quantize_kernel and mxfp4_quantize_kernel (fmi_mx.hip) with narrow_sr (fmi_mx_sr.h): one element
// (E2M1: one byte, two elements) per thread and step, the amax by shuffles inside a half (quarter) of a wave. A thread
// runs the Philox call of its element's group of 8 and keeps 16 (32) bits of it: these are the fallback's passes, not a
// hot path. An E2M1 byte's elements 2 i and 2 i + 1 lie in one group because `first` is even.
#include "fmi_mxfp4_impl.h"
#include "fmi_mx_sr.h"

namespace fmi::dev {
namespace {

constexpr unsigned kBlock = 256;  // a multiple of 64: waves start on block boundaries
constexpr size_t kGridCap = size_t(1) << 20;

template <class T, class S>
__global__ void __launch_bounds__(kBlock) mx_quantize_sr_kernel(T* out, uint8_t* out_scales, const S* src, size_t n, const uint64_t* seed_ptr,
                                                                uint64_t first) {
    const uint64_t seed = *seed_ptr;
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
            const uint64_t j = first + i;
            const uint32_t code = fp8_narrow_sr<T>(y, sr_bits(philox4x32_10(j >> 3, seed), j));
            out[i] = T{static_cast<uint8_t>(e_out == 255u ? 0x7Fu : code)};
            if (lane % 32 == 0) out_scales[i / 32] = static_cast<uint8_t>(e_out);
        }
    }
}

// n: elements; the bucket is n / 2 + n % 2 bytes, and the last byte's high nibble is not an element when n is odd.
template <class S>
__global__ void __launch_bounds__(kBlock) mxfp4_quantize_sr_kernel(uint8_t* out, uint8_t* out_scales, const S* src, size_t n,
                                                                   const uint64_t* seed_ptr, uint64_t first) {
    const uint64_t seed = *seed_ptr;
    const size_t nbytes = n / 2 + n % 2;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const unsigned lane = threadIdx.x % 64;
    // `wave0`: the first byte of this wave's 64 (four blocks); the loop's condition is the wave's, not the lane's
    for (size_t wave0 = static_cast<size_t>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); wave0 < nbytes; wave0 += stride) {
        const size_t i = wave0 + lane;
        float x[2] = {0.0f, 0.0f};  // beyond the bucket: +0; an odd bucket's last high nibble is written 0 below
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
            const uint64_t j = first + 2 * i;  // even: j and j + 1 share the word (j & 7) >> 1 of one Philox group
            const uint32_t w = philox4x32_10(j >> 3, seed).w[(static_cast<uint32_t>(j) & 7u) >> 1];
            const uint32_t hi = 2 * i + 1 < n ? fp4_narrow_sr(x[1] * inv, w >> 16) : 0u;
            const uint32_t b = e_out == 255u ? 0u : fp4_narrow_sr(x[0] * inv, w & 0xFFFFu) | (hi << 4);
            out[i] = static_cast<uint8_t>(b);
            if (lane % 16 == 0) out_scales[i / 16] = static_cast<uint8_t>(e_out);
        }
    }
}

unsigned grid_of(size_t n) { return static_cast<unsigned>(std::min(grid_for(n, kBlock), kGridCap)); }

// f.template operator()<S>() for the source of a quantization: FMI_F32, FMI_F16 or FMI_BF16.
template <class F>
int with_src_dtype(int dtype, F&& f) {
    switch (dtype) {
        case FMI_F32: return f.template operator()<float>();
        case FMI_F16: return f.template operator()<_Float16>();
        case FMI_BF16: return f.template operator()<__bf16>();
        default:
            return fail(FMI_ERR_INVALID, "fmi_dev_mx_quantize_sr: src_dtype " + std::to_string(dtype) + " must be FMI_F32, FMI_F16 or FMI_BF16");
    }
}

// One block of 32 (or fewer) host elements; i0: the block's first element in the call. scale_byte: the kernels' own
// mx_scale_byte<T> or mxfp4_scale_byte.
template <class ScaleByte, class Narrow, class Store>
void host_block(const float* src, size_t i0, size_t len, uint8_t* scale, uint64_t seed, uint64_t first, ScaleByte&& scale_byte, Narrow&& narrow,
                Store&& store) {
    uint32_t A = 0;
    for (size_t k = 0; k < len; ++k) A = std::max(A, __builtin_bit_cast(uint32_t, src[i0 + k]) & 0x7FFFFFFFu);
    const uint32_t e_out = scale_byte(A);
    *scale = static_cast<uint8_t>(e_out);
    const float inv = __builtin_bit_cast(float, (254u - (e_out == 255u ? 254u : e_out)) << 23);
    Philox4 W{};
    for (size_t k = 0; k < len; ++k) {
        const uint64_t j = first + i0 + k;
        if (k == 0 || (j & 7u) == 0u) W = philox4x32_10(j >> 3, seed);
        const volatile float y = src[i0 + k] * inv;  // one IEEE f32 multiply, kept out of any wider evaluation
        store(i0 + k, e_out == 255u ? ~0u : narrow(y, sr_bits(W, j)));
    }
}

}  // namespace

int launch_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, const uint64_t* seed,
                          uint64_t first, hipStream_t s) {
    if (n == 0) return FMI_OK;
    if (dtype == FMI_F4E2M1)
        return with_src_dtype(src_dtype, [&]<class S>() -> int {
            mxfp4_quantize_sr_kernel<S><<<grid_of(n / 2 + n % 2), kBlock, 0, s>>>(static_cast<uint8_t*>(out), out_scales, static_cast<const S*>(src),
                                                                                 n, seed, first);
            return check_launch("MXFP4 stochastic-rounding quantize kernel launch");
        });
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        return with_src_dtype(src_dtype, [&]<class S>() -> int {
            mx_quantize_sr_kernel<T, S><<<grid_of(n), kBlock, 0, s>>>(static_cast<T*>(out), out_scales, static_cast<const S*>(src), n, seed, first);
            return check_launch("MX stochastic-rounding quantize kernel launch");
        });
    });
}

// fmi_host_mx_quantize_sr after its checks. A NaN block (~0u from host_block): 0x7F bytes, zero nibbles.
int host_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, const float* src, size_t n, uint64_t seed, uint64_t first) {
    uint8_t* o = static_cast<uint8_t*>(out);
    for (size_t i0 = 0; i0 < n; i0 += 32) {
        const size_t len = std::min<size_t>(32, n - i0);
        uint8_t* scale = out_scales + i0 / 32;
        const auto fp8_store = [&](size_t i, uint32_t c) { o[i] = static_cast<uint8_t>(c == ~0u ? 0x7Fu : c); };
        if (dtype == FMI_F4E2M1) {
            for (size_t k = i0 / 2; k < (i0 + len + 1) / 2; ++k) o[k] = 0;  // i0 is even: whole bytes, the odd last high nibble 0
            host_block(src, i0, len, scale, seed, first, [](uint32_t A) { return mxfp4_scale_byte(A); },
                       [](float y, uint32_t r) { return fp4_narrow_sr(y, r); },
                       [&](size_t i, uint32_t c) { o[i / 2] = static_cast<uint8_t>(o[i / 2] | ((c == ~0u ? 0u : c) << (4 * (i % 2)))); });
        } else if (dtype == FMI_F8E4M3) {
            host_block(src, i0, len, scale, seed, first, [](uint32_t A) { return mx_scale_byte<f8e4m3>(A); },
                       [](float y, uint32_t r) { return fp8_narrow_sr<f8e4m3>(y, r); }, fp8_store);
        } else {
            host_block(src, i0, len, scale, seed, first, [](uint32_t A) { return mx_scale_byte<f8e5m2>(A); },
                       [](float y, uint32_t r) { return fp8_narrow_sr<f8e5m2>(y, r); }, fp8_store);
        }
    }
    return FMI_OK;
}

}  // namespace fmi::dev
