// fmi_mx_impl.h — the kernels of fmi_dev_reduce_tree_mx (include/fmi_dev.h): the sum or mean of block-scaled (MX) 8-bit
// float buckets, one E8M0 scale byte per 32 elements, and of fmi_dev_reduce_tree_mx_sr. Included by the
// fmi_fused_mx_*.hip translation units, fmi_mx.hip and fmi_mx_sr.hip alone.
//
//   v_p = fl32(widen(x_p) * scale32(e_p[b]));  S = F32_program(v);  S = fl32(S * r)      (r = fl32(1 / P) or 1)
//   f32 output:   out = S
//   8-bit output: per block b  A = umax bits(|S|);  e_out = mx_scale_byte(A);  out = narrow(fl32(S * 2^(127 - e_out)))
//
// The fused kernel has the shape of fp8_scaled_kernel (fmi_fp8_scaled_impl.h): a thread keeps the P raw 16-B words it
// loaded and evaluates the program twice over 8 f32 lanes. What differs:
//   - a block is TWO adjacent lanes' groups. The vector path covers whole blocks only (2 * (n / 32) lane groups: an even
//     count, and tiles and grid strides are even, so a lane and its partner lane ^ 1 are active together) and the block's
//     amax takes one exchange with the partner (__shfl_xor by 1: a DPP quad permute, no LDS);
//   - every lane loads its block's P scale bytes (a byte load per peer: the lanes of a wave read 32 consecutive bytes
//     per peer, one request) and the even lane of a pair stores the block's output byte;
//   - the ragged last block (n % 32 elements) goes to the first wave of workgroup 0, one element per lane, its amax
//     through a wave reduction. Nothing of it enters the vector path, so no block is split between the two;
//   - the mean's r is a kernel argument (1.0f for a sum: x * 1.0f is x, bit for bit) so that sum and mean share kernels.
// The multiply by the inverse scale is one IEEE f32 multiply by a normal power of two (e_out <= 247), the narrowing the
// library's non-saturating one: by the round-up rule of mx_scale_byte no element of a finite block can overflow it.
//
// Stochastic rounding (fmi_dev_reduce_tree_mx_sr; the template flag SR, 8-bit output only) is the same kernel with
// narrow_sr (fmi_mx_sr.h) where the round-to-nearest one narrows: loads, the program, the block's amax and scale byte
// are shared, so the scale bytes are the round-to-nearest call's. The random bits belong to the element, not to the
// thread: lane group g holds the elements 16 g .. 16 g + 15 of the call, whose stream positions first + 16 g + k are two
// whole Philox groups (first is a multiple of 32), q = (first >> 3) + 2 g + h for half h; word k of that group's output
// holds r of the half's elements 2 k (low 16 bits) and 2 k + 1 (high 16 bits), which are the two lanes of Fp8Half::p[k].
// The ragged block runs one element per lane and takes its element's 16 bits of its element's group. The seed is one
// u64 the thread loads once.
#pragma once

#include "fmi_fp8_impl.h"
#include "fmi_mx_sr.h"

namespace fmi::dev {

// scale32(e): the f32 value of an E8M0 scale byte. 1..254: 2^(e - 127); 0: 2^-127 (an f32 subnormal); 255: NaN.
__device__ __forceinline__ float mx_scale32(uint32_t e) {
    uint32_t b = e << 23;
    b = e == 0u ? 0x00400000u : b;
    b = e == 255u ? 0x7FC00000u : b;
    return __builtin_bit_cast(float, b);
}

__device__ __forceinline__ uint32_t mx_abs_bits(float f) { return __builtin_bit_cast(uint32_t, f) & 0x7FFFFFFFu; }

// The scale byte of a block whose largest |S| has the bits A: 255 where the block holds an inf or a NaN; otherwise the
// smallest power of two that brings A to at most the largest finite element, 1.75 * 2^EMAX (mantissa bits 0x600000).
template <class T>
__host__ __device__ __forceinline__ uint32_t mx_scale_byte(uint32_t A) {
    constexpr int kEmax = std::is_same_v<T, f8e5m2> ? 15 : 8;
    const int f = static_cast<int>(A >> 23);
    const int e = f - kEmax + ((A & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return f == 255 ? 255u : static_cast<uint32_t>(e < 0 ? 0 : e);
}

// 2^(127 - e_out) for e_out <= 254: what brings a block under its scale. A normal f32 for every e_out a finite block has.
__device__ __forceinline__ float mx_inv_scale(uint32_t e_out) { return __builtin_bit_cast(float, (254u - e_out) << 23); }

// One half of a lane group's 16 elements: widen and scale every peer, run the program, times r, fold |S| into A.
template <class T, int ALG, int P, int H>
__device__ __forceinline__ Fp8Half mx_half(const Fp8Words* raw, const float* s, float r, uint32_t& A) {
    Fp8Half v[P + kNumSteps<ALG, P>];
    [&]<size_t... I>(std::index_sequence<I...>) {
        ((v[I] = fp8_widen_half<T, H>(raw[I])), ...);
    }(std::make_index_sequence<P>{});
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p].p[k] = v[p].p[k] * s[p];
    fp8_run_steps<OpSum, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    Fp8Half S = v[kOut<ALG, P, 0>];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        S.p[k] = S.p[k] * r;
        A = max(A, max(mx_abs_bits(S.p[k].x), mx_abs_bits(S.p[k].y)));
    }
    return S;
}

// Words 2 H and 2 H + 1 of a lane group's output from half H and the Philox output of its 8 elements.
template <class T, int H>
__device__ __forceinline__ void fp8_narrow_sr_half(Fp8Words& out, const Fp8Half& v, const Philox4& W) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
        out.w[2 * H + k] = fp8_narrow_sr<T>(v.p[2 * k].x, W.w[2 * k] & 0xFFFFu) | (fp8_narrow_sr<T>(v.p[2 * k].y, W.w[2 * k] >> 16) << 8) |
                           (fp8_narrow_sr<T>(v.p[2 * k + 1].x, W.w[2 * k + 1] & 0xFFFFu) << 16) |
                           (fp8_narrow_sr<T>(v.p[2 * k + 1].y, W.w[2 * k + 1] >> 16) << 24);
}

// POL, group0, lane: as scaled_group. g: the lane group's index in the bucket; its block is g / 2. Called by both lanes
// of a pair together. seed, q0: the Philox key and first >> 3, the group of the call's element 0 (SR alone).
template <class T, int ALG, int P, bool OUT32, bool SR, bool POL>
__device__ __forceinline__ void mx_group(const PeerPtrs& ptrs, const MxArgs& mx, uint64_t seed, uint64_t q0, size_t group0, unsigned lane) {
    const size_t g = group0 + lane;
    const Fp8Access<POL, kTreeStoreAux, T> acc{POL ? group0 * 16 : g * 16, POL ? lane * 16u : 0u};
    Fp8Words raw[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    float s[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((s[I] = mx_scale32(mx.in_scales[I][g / 2])), ...); }(std::make_index_sequence<P>{});
    uint32_t A = 0;
    Fp8Half lo = mx_half<T, ALG, P, 0>(raw, s, mx.r, A);
    Fp8Half hi = mx_half<T, ALG, P, 1>(raw, s, mx.r, A);
    if constexpr (OUT32) {
        fp8_store_f32<POL>(ptrs.out[0], group0, lane, lo, hi);
    } else {
        // the block's amax: this lane's 16 elements and the partner lane's
        A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), 1)));
        const uint32_t e_out = mx_scale_byte<T>(A);
        const float inv = mx_inv_scale(e_out);
#pragma unroll
        for (int k = 0; k < 4; ++k) lo.p[k] = lo.p[k] * inv, hi.p[k] = hi.p[k] * inv;
        Fp8Words out;
        if constexpr (SR) {
            fp8_narrow_sr_half<T, 0>(out, lo, philox4x32_10(q0 + 2 * g, seed));
            fp8_narrow_sr_half<T, 1>(out, hi, philox4x32_10(q0 + 2 * g + 1, seed));
        } else {
            fp8_narrow_half<T, 0>(out, lo);
            fp8_narrow_half<T, 1>(out, hi);
        }
        if (e_out == 255u) out = Fp8Words{{0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu}};  // the whole block is NaN
        acc.store(ptrs.out[0], out);
        if ((g & 1) == 0) mx.out_scales[g / 2] = static_cast<uint8_t>(e_out);
    }
}

// The grid of fp8_scaled_kernel over the 2 * (n / 32) lane groups of the whole blocks; the first wave of workgroup 0
// takes the ragged last block.
template <class T, int ALG, int P, bool OUT32, bool SR>
__global__ void __launch_bounds__(256) fp8_mx_kernel(PeerPtrs ptrs, MxArgs mx, size_t n, int pol) {
    static_assert(!(SR && OUT32), "stochastic rounding exists only with the element type's own output");
    uint64_t seed = 0, q0 = 0;  // a round-to-nearest kernel reads neither
    if constexpr (SR) seed = *mx.seed, q0 = mx.first >> 3;
    const size_t nblk = n / 32, nvec = 2 * nblk;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec) mx_group<T, ALG, P, OUT32, SR, true>(ptrs, mx, seed, q0, tile * B, threadIdx.x);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            mx_group<T, ALG, P, OUT32, SR, false>(ptrs, mx, seed, q0, g, 0u);
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
        if constexpr (OUT32) {
            if (have) static_cast<float*>(ptrs.out[0])[i] = S;
        } else {
            uint32_t A = mx_abs_bits(S);  // 0 on the lanes beyond the block
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
            const uint32_t e_out = mx_scale_byte<T>(A);
            const float y = S * mx_inv_scale(e_out);
            if constexpr (SR) {
                const uint64_t j = mx.first + i;
                const uint32_t code = fp8_narrow_sr<T>(y, sr_bits(philox4x32_10(j >> 3, seed), j));
                if (have) static_cast<T*>(ptrs.out[0])[i] = T{static_cast<uint8_t>(e_out == 255u ? 0x7Fu : code)};
            } else {
                if (have) static_cast<T*>(ptrs.out[0])[i] = e_out == 255u ? T{0x7F} : fp8_narrow<T>(y);
            }
            if (threadIdx.x == 0) mx.out_scales[nblk] = static_cast<uint8_t>(e_out);
        }
    }
}

template <class T, int ALG, bool OUT32, bool SR, int P>
void mx_one(const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const size_t nvec = 2 * (n / 32);
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    // The scaled kernels' in-flight budget (scaled_one, fmi_fp8_scaled_impl.h): twice the resident workgroups of the
    // plain fused kernels, for the same reason; these kernels use no static LDS.
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 8);
    fp8_mx_kernel<T, ALG, P, OUT32, SR><<<grid, kFusedBlock, lds, s>>>(ptrs, mx, n, fused_policy(false, P));
}

using MxFn = void (*)(const PeerPtrs&, const MxArgs&, size_t, hipStream_t);
template <class T, int ALG, bool OUT32, bool SR, int... I>
constexpr std::array<MxFn, sizeof...(I)> mx_table(std::integer_sequence<int, I...>) {
    return {&mx_one<T, ALG, OUT32, SR, I + 2>...};
}

// SR: the caller (launch_fused_mx) has checked out_dtype == dtype; an SR unit holds no f32-output kernel.
template <int ALG, bool SR>
int mx_unit(int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, std::string(SR ? "fused MX stochastic-rounding" : "fused MX") + " kernel needs 2 <= P <= " +
                                         std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    return with_dtype<kTierFp8>(dtype, [&]<class T>() -> int {
        constexpr auto seq = std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{};
        static constexpr auto same = mx_table<T, ALG, false, SR>(seq);
        if constexpr (SR) {
            same[P - 2](ptrs, mx, n, s);
        } else {
            static constexpr auto wide = mx_table<T, ALG, true, false>(seq);
            (out_dtype == FMI_F32 ? wide : same)[P - 2](ptrs, mx, n, s);
        }
        return check_launch(SR ? "fused MX stochastic-rounding P-way kernel launch" : "fused MX P-way kernel launch");
    });
}

}  // namespace fmi::dev
