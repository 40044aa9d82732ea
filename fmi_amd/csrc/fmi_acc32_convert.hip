// fmi_dev_convert (launch_convert, below) and the streaming conversions of FMI_ACC_F32's fallback (P > 16 or unaligned buckets: widen every input to an f32
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

// The general conversion (fmi_dev_convert, and the fallback's 8-bit float side): dst[i] = narrow_D(widen_S(src[i])), the
// value through f32, so one rounding in all; S == D copies the bits. G elements per thread and step: 16 B of the
// narrower side, but at most 32 B (two 16-B accesses, 32 B apart) of the wider one, so f32 <-> 8-bit moves 8 elements
// through two 16-B accesses and one of 8 B: every wave access then uses at least half of each cache line it touches.
// Nontemporal accesses where both pointers are 16-B aligned, one element per thread otherwise. A thread loads its
// whole group before it stores, so dst == src is safe at equal element size.
// NTS: nontemporal stores (off where the library's own f32 program reads dst at once).
template <class D, class S>
__device__ __forceinline__ D convert_one(S x) {
    if constexpr (std::is_same_v<D, S>) {
        return x;
    } else {
        Lanes<S, 1> a;
        a.v[0] = x;
        return to_storage<D>(to_value<float>(a)).v[0];
    }
}

using u32x2 = unsigned int __attribute__((ext_vector_type(2)));

template <class T, int W>
__device__ __forceinline__ Lanes<T, W> load_chunk(const T* p) {
    if constexpr (sizeof(T) * W == 8)
        return __builtin_bit_cast(Lanes<T, W>, __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)));
    else
        return load_lanes<true, T, W>(p);
}

template <bool NTS, class T, int W>
__device__ __forceinline__ void store_chunk(T* p, const Lanes<T, W>& x) {
    if constexpr (NTS && sizeof(T) * W == 8)
        __builtin_nontemporal_store(__builtin_bit_cast(u32x2, x), reinterpret_cast<u32x2*>(p));
    else
        store_lanes<NTS, T, W>(p, x);
}

template <class D, class S>
inline constexpr int kConvGroup = std::min(16 / static_cast<int>(std::min(sizeof(S), sizeof(D))),
                                           32 / static_cast<int>(std::max(sizeof(S), sizeof(D))));

template <class D, class S, bool NTS>
__global__ void __launch_bounds__(kConvBlock) convert_kernel(D* dst, const S* src, size_t n, bool vec) {
    constexpr int G = kConvGroup<D, S>;
    constexpr int CS = std::min(G, 16 / static_cast<int>(sizeof(S))), CD = std::min(G, 16 / static_cast<int>(sizeof(D)));  // lanes per access
    static_assert(G % CS == 0 && G % CD == 0 && sizeof(S) * CS >= 8 && sizeof(D) * CD >= 8, "accesses of 8 or 16 B");
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (vec) {
        const size_t nvec = n / G;
        for (size_t g = first; g < nvec; g += stride) {
            if constexpr (std::is_same_v<D, S>) {
                store_chunk<NTS, D, CD>(dst + g * G, load_chunk<S, CS>(src + g * G));
            } else {
                Lanes<float, G> v;
#pragma unroll
                for (int c = 0; c < G / CS; ++c) {
                    const Lanes<float, CS> part = to_value<float>(load_chunk<S, CS>(src + g * G + c * CS));
#pragma unroll
                    for (int k = 0; k < CS; ++k) v.v[c * CS + k] = part.v[k];
                }
#pragma unroll
                for (int c = 0; c < G / CD; ++c) {
                    Lanes<float, CD> part;
#pragma unroll
                    for (int k = 0; k < CD; ++k) part.v[k] = v.v[c * CD + k];
                    store_chunk<NTS, D, CD>(dst + g * G + c * CD, to_storage<D>(part));
                }
            }
        }
        const size_t i = nvec * G + threadIdx.x;
        if (blockIdx.x == 0 && i < n) dst[i] = convert_one<D>(src[i]);
    } else {
        for (size_t i = first; i < n; i += stride) dst[i] = convert_one<D>(src[i]);
    }
}

template <class D, class S, bool NTS = true>
int launch_convert_kernel(void* dst, const void* src, size_t n, hipStream_t s) {
    constexpr size_t G = kConvGroup<D, S>;
    const bool vec = aligned16(dst) && aligned16(src);
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / G : n, kConvBlock), kConvGridCap));
    convert_kernel<D, S, NTS><<<grid, kConvBlock, 0, s>>>(static_cast<D*>(dst), static_cast<const S*>(src), n, vec);
    return check_launch("conversion kernel launch");
}

// f.template operator()<T>() for one of the five dtypes of fmi_dev_convert (checked by the caller)
template <class F>
int with_convert_dtype(int dtype, F&& f) {
    switch (dtype) {
        case FMI_F32: return f.template operator()<float>();
        case FMI_F16: return f.template operator()<_Float16>();
        case FMI_BF16: return f.template operator()<__bf16>();
        case FMI_F8E4M3: return f.template operator()<f8e4m3>();
        case FMI_F8E5M2: return f.template operator()<f8e5m2>();
        default: return fail(FMI_ERR_INVALID, "conversion: dtype " + std::to_string(dtype) + " is not a float dtype of at most 32 bits");
    }
}

}  // namespace

int launch_convert(int dst_dtype, void* dst, int src_dtype, const void* src, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    if (dst_dtype == src_dtype && dst == src) return FMI_OK;
    return with_convert_dtype(dst_dtype, [&]<class D>() -> int {
        return with_convert_dtype(src_dtype, [&]<class S>() -> int { return launch_convert_kernel<D, S>(dst, src, n, s); });
    });
}

int launch_widen_f32(int dtype, float* dst, const void* src, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    if (is_fp8_dtype(dtype))  // plain stores: the f32 program reads dst at once
        return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int { return launch_convert_kernel<float, T, false>(dst, src, n, s); });
    const bool vec = aligned16(dst) && aligned16(src);
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / 8 : n, kConvBlock), kConvGridCap));
    return with_dtype<kTierHalf>(dtype, [&]<class T>() -> int {
        widen_kernel<T><<<grid, kConvBlock, 0, s>>>(dst, static_cast<const T*>(src), n, vec);
        return check_launch("f32 widen kernel launch");
    });
}

int launch_narrow_f32(int dtype, void* dst, const float* src, size_t n, hipStream_t s) {
    if (n == 0) return FMI_OK;
    if (is_fp8_dtype(dtype)) return launch_convert(dtype, dst, FMI_F32, src, n, s);
    const bool vec = aligned16(dst) && aligned16(src);
    const unsigned grid = static_cast<unsigned>(std::min(grid_for(vec ? n / 8 : n, kConvBlock), kConvGridCap));
    return with_dtype<kTierHalf>(dtype, [&]<class T>() -> int {
        narrow_kernel<T><<<grid, kConvBlock, 0, s>>>(static_cast<T*>(dst), src, n, vec);
        return check_launch("f32 narrow kernel launch");
    });
}

}  // namespace fmi::dev
