// fmi_fp8_scaled_impl.h — the kernels of fmi_dev_reduce_tree_scaled (include/fmi_dev.h): the scaled sum of 8-bit float
// buckets, included by the fmi_fused_fp8_scaled_*.hip translation units and fmi_fp8_scaled.hip alone.
//
//   v_p = fl32(widen(x_p) * s_p);  S = F32_program(v);  amax = umax bits(|S|);  out = narrow(fl32(S * t)) or fl32(S * t)
//
// The fused kernel has the shape of fp8_acc_kernel (fmi_fp8_impl.h): a thread keeps the P raw 16-B words it loaded and
// evaluates the program twice over 8 f32 lanes (four 2-lane vectors: v_cvt_pk_f32_fp8 / _bf8, v_pk_mul_f32 by the
// peer's scale, v_pk_add_f32 steps, v_pk_mul_f32 by t, v_cvt_pk_fp8_f32 / _bf8_f32). The library is built with
// -ffp-contract=off and no instruction fuses an f32 multiply into the 8-bit narrowing, so every multiply stands alone.
// The P scales and t are uniform: read once per thread from device memory into scalar registers. An f32 output is 64 B
// per lane group, four 16-B stores; its tile addressing is its own (4x the input's bytes). amax: a running
// max of |S|'s bits per thread, then per wave (shuffles), then per workgroup through 64 B of LDS, then at most one
// atomic max on the 32-bit word by thread 0; `amax == nullptr` is a uniform branch around all of it. The < 16-element
// tail of a bucket goes to workgroup 0, one element per thread, through run_steps on one f32 lane.
#pragma once

#include "fmi_fp8_impl.h"

namespace fmi::dev {

// The scale of input slot I: the caller's in_scales[(I + rot) % P] (rot < P).
template <int P>
__device__ __forceinline__ float scaled_in_scale(const ScaledArgs& sc, int I) {
    int j = I + sc.rot;
    j -= j >= P ? P : 0;
    return sc.in_scales[j];
}

__device__ __forceinline__ uint32_t abs_bits(float f) { return __builtin_bit_cast(uint32_t, f) & 0x7FFFFFFFu; }

// The workgroup's maximum into *amax: all threads of the workgroup call it (uniform control flow), blockDim.x <= 1024.
__device__ __forceinline__ void amax_commit(float* amax, uint32_t m) {
    constexpr unsigned kWave = 64;  // gfx950
    __shared__ uint32_t wave_max[1024 / kWave];
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), d, kWave)));
    const unsigned wave = threadIdx.x / kWave, nwaves = (blockDim.x + kWave - 1) / kWave;
    if (threadIdx.x % kWave == 0) wave_max[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < nwaves; ++w) m = max(m, wave_max[w]);
        // *amax holds a non-negative float or a NaN and only grows while calls fold into it, so a workgroup whose
        // maximum is not above a value read now has nothing to add, and a stale read costs no more than the atomic.
        // Without the read every workgroup's atomic goes to the one word (65,536 of them at 256 MiB per peer) and the
        // kernel waits for them: 0.35 of 8 TB/s against 0.57 with amax == nullptr.
        unsigned int* word = reinterpret_cast<unsigned int*>(amax);
        if (m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, m);
    }
}

// One half of a lane group's 16 elements: widen and scale every peer, run the program, fold |S| into m, scale by t.
template <class T, int ALG, int P, int H>
__device__ __forceinline__ Fp8Half scaled_half(const Fp8Words* raw, const float* s, float t, bool want_amax, uint32_t& m) {
    Fp8Half v[P + kNumSteps<ALG, P>];
    [&]<size_t... I>(std::index_sequence<I...>) {
        ((v[I] = fp8_widen_half<T, H>(raw[I])), ...);
    }(std::make_index_sequence<P>{});
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p].p[k] = v[p].p[k] * s[p];
    fp8_run_steps<OpSum, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    Fp8Half r = v[kOut<ALG, P, 0>];
    if (want_amax) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m = max(m, max(abs_bits(r.p[k].x), abs_bits(r.p[k].y)));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r.p[k] = r.p[k] * t;
    return r;
}

// POL: buffer accesses through tile descriptors or global accesses, as Fp8Access. g: the lane group's index in the
// bucket (POL = false), tile / lane: the tile's first lane group and the lane's index in it (POL = true).
template <class T, int ALG, int P, bool OUT32, bool POL>
__device__ __forceinline__ void scaled_group(const PeerPtrs& ptrs, size_t group0, unsigned lane, const float* s, float t,
                                             bool want_amax, uint32_t& m) {
    const Fp8Access<POL, kTreeStoreAux, T> acc{POL ? group0 * 16 : (group0 + lane) * 16, POL ? lane * 16u : 0u};
    Fp8Words raw[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    const Fp8Half lo = scaled_half<T, ALG, P, 0>(raw, s, t, want_amax, m);
    const Fp8Half hi = scaled_half<T, ALG, P, 1>(raw, s, t, want_amax, m);
    if constexpr (OUT32) {
        fp8_store_f32<POL>(ptrs.out[0], group0, lane, lo, hi);
    } else {
        Fp8Words out;
        fp8_narrow_half<T, 0>(out, lo);
        fp8_narrow_half<T, 1>(out, hi);
        acc.store(ptrs.out[0], out);
    }
}

// The grid of tree_kernel (fmi_kernels.h): one thread per 16-B input lane group up to kFusedGridCap workgroups,
// striding beyond; workgroup 0 takes the tail.
template <class T, int ALG, int P, bool OUT32>
__global__ void __launch_bounds__(256) fp8_scaled_kernel(PeerPtrs ptrs, ScaledArgs sc, size_t n, int pol) {
    float s[P];
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] = scaled_in_scale<P>(sc, p);
    const float t = sc.out_scale ? *sc.out_scale : 1.0f;
    const bool want_amax = sc.amax != nullptr;
    uint32_t m = 0;
    const size_t nvec = n / 16;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec) scaled_group<T, ALG, P, OUT32, true>(ptrs, tile * B, threadIdx.x, s, t, want_amax, m);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            scaled_group<T, ALG, P, OUT32, false>(ptrs, g, 0u, s, t, want_amax, m);
    }
    const size_t i = nvec * 16 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
        Lanes<float, 1> v[P + kNumSteps<ALG, P>];
        [&]<size_t... I>(std::index_sequence<I...>) {
            ((v[I].v[0] = fp8_widen(static_cast<const T*>(ptrs.in[I])[i]) * s[I]), ...);
        }(std::make_index_sequence<P>{});
        run_steps<OpSum, float, 1, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
        const float S = v[kOut<ALG, P, 0>].v[0];
        if (want_amax) m = max(m, abs_bits(S));
        const float y = S * t;
        if constexpr (OUT32)
            static_cast<float*>(ptrs.out[0])[i] = y;
        else
            static_cast<T*>(ptrs.out[0])[i] = fp8_narrow<T>(y);
    }
    if (want_amax) amax_commit(sc.amax, m);
}

template <class T, int ALG, bool OUT32, int P>
void scaled_one(const PeerPtrs& ptrs, const ScaledArgs& sc, size_t n, hipStream_t s) {
    const size_t nvec = n / 16;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    // Twice the workgroups per CU the plain fused kernels' in-flight budget allows (the reservation of half the bytes
    // per workgroup): these kernels carry ~200 VALU instructions per lane group at P = 8 against the unscaled 8-bit
    // kernel's ~130, and at its 2 workgroups per CU a wave's arithmetic is not hidden behind another wave's loads:
    // 0.57 of 8 TB/s at the plain budget, 0.79 at twice. amax_commit's static 64 B come on top of the
    // reservation, so it is one allocation granule smaller.
    size_t lds = fused_lds_bytes(P, kFusedBlock * 8);
    if (lds >= 512) lds -= 256;
    fp8_scaled_kernel<T, ALG, P, OUT32><<<grid, kFusedBlock, lds, s>>>(ptrs, sc, n, fused_policy(false, P));
}

using ScaledFn = void (*)(const PeerPtrs&, const ScaledArgs&, size_t, hipStream_t);
template <class T, int ALG, bool OUT32, int... I>
constexpr std::array<ScaledFn, sizeof...(I)> scaled_table(std::integer_sequence<int, I...>) {
    return {&scaled_one<T, ALG, OUT32, I + 2>...};
}

template <int ALG>
int scaled_unit(int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const ScaledArgs& sc, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "fused scaled kernel needs 2 <= P <= " + std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        constexpr auto seq = std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{};
        static constexpr auto same = scaled_table<T, ALG, false>(seq);
        static constexpr auto wide = scaled_table<T, ALG, true>(seq);
        (out_dtype == FMI_F32 ? wide : same)[P - 2](ptrs, sc, n, s);
        return check_launch("fused scaled P-way kernel launch");
    });
}

}  // namespace fmi::dev
