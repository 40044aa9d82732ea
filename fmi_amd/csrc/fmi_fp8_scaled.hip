// The kernels of fmi_dev_reduce_tree_scaled beside the fused ones (include/fmi_dev.h): what a call beyond them (P = 1,
// P > 16, unaligned buckets) runs around the library's own FMI_F32 program, and the amax fold of
// fmi_comm_allreduce_scaled.
//   widen_scale   dst[i] = fl32(widen(src[i]) * s)                                 one per input bucket
//   finish        amax <- umax bits(|S[i]|);  out[i] = narrow(fl32(S[i] * t)) or fl32(S[i] * t)
//   amax_fold     *amax = umax(bits(*amax), words[0 .. count))                     one thread
// Each multiply is one IEEE f32 multiply (-ffp-contract=off; nothing fuses one into the 8-bit narrowing). Any
// alignment: one element per thread and step, grid-stride. These are the fallback's passes, not a hot path: the
// f32 temporaries they stream cost 4 bytes per element each way whatever the access width.
#include "fmi_fp8_scaled_impl.h"

namespace fmi::dev {
namespace {

constexpr unsigned kBlock = 256;
constexpr size_t kGridCap = size_t(1) << 20;

template <class T>
__global__ void __launch_bounds__(kBlock) widen_scale_kernel(float* dst, const T* src, const float* scale, size_t n) {
    const float s = *scale;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = fp8_widen(src[i]) * s;
}

// T: the 8-bit storage type of the call; OUT32: out is f32.
template <class T, bool OUT32>
__global__ void __launch_bounds__(kBlock) finish_kernel(void* out, const float* S, const float* out_scale, float* amax, size_t n) {
    const float t = out_scale ? *out_scale : 1.0f;
    const bool want_amax = amax != nullptr;
    uint32_t m = 0;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = S[i];
        if (want_amax) m = max(m, abs_bits(v));
        const float y = v * t;
        if constexpr (OUT32)
            static_cast<float*>(out)[i] = y;
        else
            static_cast<T*>(out)[i] = fp8_narrow<T>(y);
    }
    if (want_amax) amax_commit(amax, m);
}

__global__ void amax_fold_kernel(float* amax, const uint32_t* words, int count) {
    uint32_t m = *reinterpret_cast<const uint32_t*>(amax);
    for (int k = 0; k < count; ++k) m = max(m, words[k]);
    *reinterpret_cast<uint32_t*>(amax) = m;
}

unsigned grid_of(size_t n) { return static_cast<unsigned>(std::min(grid_for(n, kBlock), kGridCap)); }

}  // namespace

int launch_widen_scale_f32(int dtype, float* dst, const void* src, const float* scale, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        widen_scale_kernel<T><<<grid_of(n), kBlock, 0, s>>>(dst, static_cast<const T*>(src), scale, n);
        return check_launch("scaled widen kernel launch");
    });
}

int launch_scaled_finish(int dtype, int out_dtype, void* out, const float* S, const float* out_scale, float* amax, size_t n,
                         hipStream_t s) {
    if (n == 0) return FMI_OK;
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        if (out_dtype == FMI_F32)
            finish_kernel<T, true><<<grid_of(n), kBlock, 0, s>>>(out, S, out_scale, amax, n);
        else
            finish_kernel<T, false><<<grid_of(n), kBlock, 0, s>>>(out, S, out_scale, amax, n);
        return check_launch("scaled finishing kernel launch");
    });
}

int launch_amax_fold(float* amax, const uint32_t* words, int count, hipStream_t s) {
    amax_fold_kernel<<<1, 1, 0, s>>>(amax, words, count);
    return check_launch("amax fold kernel launch");
}

}  // namespace fmi::dev
