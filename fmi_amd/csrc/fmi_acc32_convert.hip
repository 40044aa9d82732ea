// The streaming conversions of FMI_ACC_F32's fallback (P > 16 or unaligned buckets: widen every input to an f32
// temporary, run the library's own FMI_F32 program, narrow every stored output): 8 elements per thread through one
// 16-B access on the 16-bit side and two on the f32 side where both pointers allow it, one element per thread
// otherwise (any alignment), like pair_tile / pair_scalar. Widening is exact; narrowing is to_storage's rounding
// (round-to-nearest-even, subnormals kept, NaN stays NaN), the same code the fused acc32 kernels store through.
#include "fmi_fused_impl.h"

namespace fmi::dev {
namespace {

constexpr unsigned kConvBlock = 256;
constexpr size_t kConvGridCap = size_t(1) << 20;

template <class T>
__global__ void __launch_bounds__(kConvBlock) widen_kernel(float* dst, const T* src, size_t n, bool vec) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (vec) {
        const size_t nvec = n / 8;
        for (size_t g = first; g < nvec; g += stride) {
            const Lanes<float, 8> v = to_value<float>(load_lanes<true, T, 8>(src + g * 8));
            Lanes<float, 4> lo, hi;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo.v[k] = v.v[k];
                hi.v[k] = v.v[4 + k];
            }
            store_lanes<false, float, 4>(dst + g * 8, lo);  // read again at once by the f32 program
            store_lanes<false, float, 4>(dst + g * 8 + 4, hi);
        }
        const size_t i = nvec * 8 + threadIdx.x;
        if (blockIdx.x == 0 && i < n) dst[i] = static_cast<float>(src[i]);
    } else {
        for (size_t i = first; i < n; i += stride) dst[i] = static_cast<float>(src[i]);
    }
}

template <class T>
__global__ void __launch_bounds__(kConvBlock) narrow_kernel(T* dst, const float* src, size_t n, bool vec) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (vec) {
        const size_t nvec = n / 8;
        for (size_t g = first; g < nvec; g += stride) {
            const Lanes<float, 4> lo = load_lanes<true, float, 4>(src + g * 8), hi = load_lanes<true, float, 4>(src + g * 8 + 4);
            Lanes<float, 8> v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v.v[k] = lo.v[k];
                v.v[4 + k] = hi.v[k];
            }
            store_lanes<true, T, 8>(dst + g * 8, to_storage<T>(v));
        }
        const size_t i = nvec * 8 + threadIdx.x;
        if (blockIdx.x == 0 && i < n) {
            Lanes<float, 1> x;
            x.v[0] = src[i];
            dst[i] = to_storage<T>(x).v[0];
        }
    } else {
        for (size_t i = first; i < n; i += stride) {
            Lanes<float, 1> x;
            x.v[0] = src[i];
            dst[i] = to_storage<T>(x).v[0];
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int launch_widen_f32(int dtype, float* dst, const void* src, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    const bool vec = aligned16(dst) && aligned16(src);
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / 8 : n, kConvBlock), kConvGridCap));
    return with_dtype<kTierHalf>(dtype, [&]<class T>() -> int {
        widen_kernel<T><<<grid, kConvBlock, 0, s>>>(dst, static_cast<const T*>(src), n, vec);
        return check_launch("f32 widen kernel launch");
    });
}

int launch_narrow_f32(int dtype, void* dst, const float* src, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    const bool vec = aligned16(dst) && aligned16(src);
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / 8 : n, kConvBlock), kConvGridCap));
    return with_dtype<kTierHalf>(dtype, [&]<class T>() -> int {
        narrow_kernel<T><<<grid, kConvBlock, 0, s>>>(static_cast<T*>(dst), src, n, vec);
        return check_launch("f32 narrow kernel launch");
    });
}

}  // namespace fmi::dev
