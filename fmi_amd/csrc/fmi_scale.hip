// The scale kernel of FMI_OP_AVG (fmi_dev_mean_scale, and every mean call beyond the fused kernels: P > 16 or
// unaligned buckets run the unchanged SUM program and then this on its result): in place,
//   inout[i] = store(fl_V(value(inout[i]) * r)),  r = fl_V(1 / P) computed on the host,
// V = f32 for f32 / f16 / bf16 / E4M3 / E5M2 and f64 for f64: one IEEE multiply and, for the 8- and 16-bit floats, the narrowing
// Op::apply ends with (to_storage), from an opaque register so that multiply and narrowing are not fused into
// v_fma_mixlo_f16 x, y, +0 (-0 would come out as +0). One 16-B nontemporal load and store per thread and step on an
// aligned bucket, its < 16-B remainder by the first threads of workgroup 0; one element per thread on an unaligned
// one, like pair_tile / pair_scalar. Algorithmic HBM bytes: 2 x bytes.
#include "fmi_fused_impl.h"

namespace fmi::dev {
namespace {

constexpr unsigned kScaleBlock = 256;
constexpr size_t kScaleGridCap = size_t(1) << 20;

template <class T>
using ScaleValue = std::conditional_t<std::is_same_v<T, double>, double, float>;

template <class T, int W>
__device__ __forceinline__ Lanes<T, W> scale_lanes(const Lanes<T, W>& x, ScaleValue<T> r) {
    if constexpr (is_narrow_float_v<T>) {
        Lanes<float, W> f = to_value<float>(x);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float y = f.v[k] * r;
            asm("" : "+v"(y));
            f.v[k] = y;
        }
        return to_storage<T>(f);
    } else {
        Lanes<T, W> y;
#pragma unroll
        for (int k = 0; k < W; ++k) y.v[k] = x.v[k] * r;
        return y;
    }
}

template <class T>
__global__ void __launch_bounds__(kScaleBlock) scale_kernel(T* inout, size_t n, ScaleValue<T> r, bool vec) {
    constexpr int W = kVecLanes<T>;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (vec) {
        const size_t nvec = n / W;
        for (size_t g = first; g < nvec; g += stride)
            store_lanes<true, T, W>(inout + g * W, scale_lanes<T, W>(load_lanes<true, T, W>(inout + g * W), r));
        const size_t i = nvec * W + threadIdx.x;
        if (blockIdx.x == 0 && i < n) {
            Lanes<T, 1> x;
            x.v[0] = inout[i];
            inout[i] = scale_lanes<T, 1>(x, r).v[0];
        }
    } else {
        for (size_t i = first; i < n; i += stride) {
            Lanes<T, 1> x;
            x.v[0] = inout[i];
            inout[i] = scale_lanes<T, 1>(x, r).v[0];
        }
    }
}

template <class T>
int launch(void* inout, size_t n, int P, hipStream_t s) {
    using V = ScaleValue<T>;
    const V r = static_cast<V>(1) / static_cast<V>(P);  // correctly rounded: one IEEE division on the host
    const bool vec = (reinterpret_cast<uintptr_t>(inout) & 15u) == 0;
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / kVecLanes<T> : n, kScaleBlock), kScaleGridCap));
    scale_kernel<T><<<grid, kScaleBlock, 0, s>>>(static_cast<T*>(inout), n, r, vec);
    return check_launch("mean scale kernel launch");
}

}  // namespace

int launch_mean_scale(int dtype, void* inout, size_t n, int P, hipStream_t s) {
    if (n == 0 || P == 1) return FMI_OK;  // r = 1: the bits unchanged (a NaN's payload too)
    switch (dtype) {
        case FMI_F32: return launch<float>(inout, n, P, s);
        case FMI_F64: return launch<double>(inout, n, P, s);
        case FMI_F16: return launch<_Float16>(inout, n, P, s);
        case FMI_BF16: return launch<__bf16>(inout, n, P, s);
        case FMI_F8E4M3: return launch<f8e4m3>(inout, n, P, s);
        case FMI_F8E5M2: return launch<f8e5m2>(inout, n, P, s);
        default: return fail(FMI_ERR_INVALID, "FMI_OP_AVG: dtype " + std::to_string(dtype) + " is not a float dtype");
    }
}

}  // namespace fmi::dev
