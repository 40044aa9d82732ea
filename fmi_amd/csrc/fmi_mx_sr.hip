// fmi_host_mx_quantize_sr (include/fmi_dev.h): fmi_dev_mx_quantize_sr's quantization on host memory, from the functions
// the kernels use (fmi_mx_sr.h, and the scale-byte rules of fmi_mx_impl.h / fmi_mxfp4_impl.h / fmi_mxfp6_impl.h). Host code only: the
// kernels of the device call are the quantize kernels' SR instantiations (fmi_mx.hip).
//   per block of 32: A = umax bits(|S|), e_out = the block's scale byte, out = narrow_sr(fl32(S * 2^(127 - e_out)), r)
#include "fmi_mxfp4_impl.h"
#include "fmi_mxfp6_impl.h"

namespace fmi::dev {
namespace {

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

// fmi_host_mx_quantize_sr after its checks. A NaN block (~0u from host_block): 0x7F bytes, zero nibbles.
int host_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, const float* src, size_t n, uint64_t seed, uint64_t first) {
    uint8_t* o = static_cast<uint8_t*>(out);
    for (size_t i0 = 0; i0 < n; i0 += 32) {
        const size_t len = std::min<size_t>(32, n - i0);
        uint8_t* scale = out_scales + i0 / 32;
        const auto fp8_store = [&](size_t i, uint32_t c) { o[i] = static_cast<uint8_t>(c == ~0u ? 0x7Fu : c); };
        if (is_fp6_dtype(dtype)) {
            // i0 is a multiple of 4: whole bytes from 3 i0 / 4 on; zeroed first, so the last byte's unused bits stay 0
            for (size_t k = i0 / 4 * 3; k < mx_elem_bytes(dtype, i0 + len); ++k) o[k] = 0;
            const auto fp6_store = [&](size_t i, uint32_t c) {
                const uint32_t v = (c == ~0u ? 0u : c) << (6 * i % 8);  // up to 12 bits over two bytes
                o[6 * i / 8] = static_cast<uint8_t>(o[6 * i / 8] | v);
                if (v >> 8) o[6 * i / 8 + 1] = static_cast<uint8_t>(o[6 * i / 8 + 1] | (v >> 8));
            };
            if (dtype == FMI_F6E2M3)
                host_block(src, i0, len, scale, seed, first, [](uint32_t A) { return mxfp6_scale_byte<3>(A); },
                           [](float y, uint32_t r) { return fp6_narrow_sr<3>(y, r); }, fp6_store);
            else
                host_block(src, i0, len, scale, seed, first, [](uint32_t A) { return mxfp6_scale_byte<2>(A); },
                           [](float y, uint32_t r) { return fp6_narrow_sr<2>(y, r); }, fp6_store);
        } else if (dtype == FMI_F4E2M1) {
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
