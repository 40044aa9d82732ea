// fmi_mx_sr_impl.h — the fused kernels of fmi_dev_reduce_tree_mx_sr at the two 8-bit floats (include/fmi_dev.h):
// fp8_mx_kernel's 8-bit-output branch (fmi_mx_impl.h) with narrow_sr (fmi_mx_sr.h) where that one narrows. Included by
// the fmi_fused_mx_sr_*.hip translation units alone. Loads, the program, the block's amax and scale byte, both access
// policies, the grid and the in-flight budget are fp8_mx_kernel's, through its own device functions (mx_half); the
// scale bytes are therefore the round-to-nearest call's.
//
// The random bits belong to the element, not to the thread: lane group g holds the elements 16 g .. 16 g + 15 of the
// call, whose stream positions first + 16 g + k are two whole Philox groups (first is a multiple of 32), q =
// (first >> 3) + 2 g + h for half h; word k of that group's output holds r of the half's elements 2 k (low 16 bits) and
// 2 k + 1 (high 16 bits), which are the two lanes of Fp8Half::p[k]. The ragged block runs one element per lane and takes
// its element's 16 bits of its element's group. The seed is one u64 the thread loads once.
#pragma once

#include "fmi_mx_impl.h"
#include "fmi_mx_sr.h"

namespace fmi::dev {

// Words 2 H and 2 H + 1 of a lane group's output from half H and the Philox output of its 8 elements.
template <class T, int H>
__device__ __forceinline__ void fp8_narrow_sr_half(Fp8Words& out, const Fp8Half& v, const Philox4& W) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
        out.w[2 * H + k] = fp8_narrow_sr<T>(v.p[2 * k].x, W.w[2 * k] & 0xFFFFu) | (fp8_narrow_sr<T>(v.p[2 * k].y, W.w[2 * k] >> 16) << 8) |
                           (fp8_narrow_sr<T>(v.p[2 * k + 1].x, W.w[2 * k + 1] & 0xFFFFu) << 16) |
                           (fp8_narrow_sr<T>(v.p[2 * k + 1].y, W.w[2 * k + 1] >> 16) << 24);
}

// mx_group's 8-bit output with narrow_sr. q0: first >> 3, the Philox group of the call's element 0.
template <class T, int ALG, int P, bool POL>
__device__ __forceinline__ void mx_sr_group(const PeerPtrs& ptrs, const MxArgs& mx, uint64_t seed, uint64_t q0, size_t group0, unsigned lane) {
    const size_t g = group0 + lane;
    const Fp8Access<POL, kTreeStoreAux, T> acc{POL ? group0 * 16 : g * 16, POL ? lane * 16u : 0u};
    Fp8Words raw[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    float s[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((s[I] = mx_scale32(mx.in_scales[I][g / 2])), ...); }(std::make_index_sequence<P>{});
    uint32_t A = 0;
    Fp8Half lo = mx_half<T, ALG, P, 0>(raw, s, mx.r, A);
    Fp8Half hi = mx_half<T, ALG, P, 1>(raw, s, mx.r, A);
    A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), 1)));
    const uint32_t e_out = mx_scale_byte<T>(A);
    const float inv = mx_inv_scale(e_out);
#pragma unroll
    for (int k = 0; k < 4; ++k) lo.p[k] = lo.p[k] * inv, hi.p[k] = hi.p[k] * inv;
    Fp8Words out;
    fp8_narrow_sr_half<T, 0>(out, lo, philox4x32_10(q0 + 2 * g, seed));
    fp8_narrow_sr_half<T, 1>(out, hi, philox4x32_10(q0 + 2 * g + 1, seed));
    if (e_out == 255u) out = Fp8Words{{0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu}};  // the whole block is NaN
    acc.store(ptrs.out[0], out);
    if ((g & 1) == 0) mx.out_scales[g / 2] = static_cast<uint8_t>(e_out);
}

// fp8_mx_kernel's grid and ragged block.
template <class T, int ALG, int P>
__global__ void __launch_bounds__(256) fp8_mx_sr_kernel(PeerPtrs ptrs, MxArgs mx, size_t n, int pol) {
    const uint64_t seed = *mx.seed;
    const uint64_t q0 = mx.first >> 3;
    const size_t nblk = n / 32, nvec = 2 * nblk;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec) mx_sr_group<T, ALG, P, true>(ptrs, mx, seed, q0, tile * B, threadIdx.x);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            mx_sr_group<T, ALG, P, false>(ptrs, mx, seed, q0, g, 0u);
    }
    const size_t first = nblk * 32;
    if (blockIdx.x == 0 && threadIdx.x < 64 && first < n) {  // one whole wave: uniform for the reduction below
        const size_t i = first + threadIdx.x;
        const bool have = i < n;  // 1..31 lanes
        float S = 0.0f;
        if (have) {
            Lanes<float, 1> v[P + kNumSteps<ALG, P>];
            [&]<size_t... I>(std::index_sequence<I...>) {
                ((v[I].v[0] = fp8_widen(static_cast<const T*>(ptrs.in[I])[i]) * mx_scale32(mx.in_scales[I][nblk])), ...);
            }(std::make_index_sequence<P>{});
            run_steps<OpSum, float, 1, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
            S = v[kOut<ALG, P, 0>].v[0] * mx.r;
        }
        uint32_t A = mx_abs_bits(S);  // 0 on the lanes beyond the block
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
        const uint32_t e_out = mx_scale_byte<T>(A);
        const float y = S * mx_inv_scale(e_out);
        const uint64_t j = mx.first + i;
        const uint32_t code = fp8_narrow_sr<T>(y, sr_bits(philox4x32_10(j >> 3, seed), j));
        if (have) static_cast<T*>(ptrs.out[0])[i] = T{static_cast<uint8_t>(e_out == 255u ? 0x7Fu : code)};
        if (threadIdx.x == 0) mx.out_scales[nblk] = static_cast<uint8_t>(e_out);
    }
}

template <class T, int ALG, int P>
void mx_sr_one(const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const size_t nvec = 2 * (n / 32);
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 8);  // mx_one's in-flight budget
    fp8_mx_sr_kernel<T, ALG, P><<<grid, kFusedBlock, lds, s>>>(ptrs, mx, n, fused_policy(false, P));
}

template <class T, int ALG, int... I>
constexpr std::array<MxFn, sizeof...(I)> mx_sr_table(std::integer_sequence<int, I...>) {
    return {&mx_sr_one<T, ALG, I + 2>...};
}

template <int ALG>
int mx_sr_unit(int dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "fused MX stochastic-rounding kernel needs 2 <= P <= " + std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        static constexpr auto table = mx_sr_table<T, ALG>(std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{});
        table[P - 2](ptrs, mx, n, s);
        return check_launch("fused MX stochastic-rounding P-way kernel launch");
    });
}

}  // namespace fmi::dev
