// fmi_mxfp4_sr_impl.h — the fused kernels of fmi_dev_reduce_tree_mx_sr at FMI_F4E2M1 (include/fmi_dev.h): mxfp4_kernel's
// E2M1-output branch (fmi_mxfp4_impl.h) with narrow_sr (fmi_mx_sr.h) where that one narrows. Included by the
// fmi_fused_mxfp4_sr_*.hip translation units alone. Loads, the program, the block's amax and scale byte, both access
// policies, the grid and the in-flight budget are mxfp4_kernel's, through its own device functions (mxfp4_piece).
//
// One lane is one block b of 32 elements at the stream positions first + 32 b + k: four whole Philox groups,
// q = (first >> 3) + 4 b + K for piece K, whose output word k holds r of the piece's elements 2 k and 2 k + 1, the two
// lanes of Fp8Half::p[k] and the two nibbles of byte k of output word K. A group's four words are dead once its piece is
// narrowed, so one Philox state is live at a time beside the 32 results. The narrowing is a few exact f32 operations
// per element (fmi_mx_sr.h), not the packed conversion instruction: that one rounds to nearest, and its stochastic form
// was not shown to follow this definition.
#pragma once

#include "fmi_mxfp4_impl.h"
#include "fmi_mx_sr.h"

namespace fmi::dev {

// The 8 nibbles of one piece.
__device__ __forceinline__ uint32_t fp4_narrow_sr_word(const Fp8Half& v, const Philox4& W) {
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w |= (fp4_narrow_sr(v.p[k].x, W.w[k] & 0xFFFFu) | (fp4_narrow_sr(v.p[k].y, W.w[k] >> 16) << 4)) << (8 * k);
    return w;
}

// mxfp4_block's E2M1 output with narrow_sr. q0: first >> 3.
template <int ALG, int P, bool POL>
__device__ __forceinline__ void mxfp4_sr_block(const PeerPtrs& ptrs, const MxArgs& mx, uint64_t seed, uint64_t q0, size_t group0, unsigned lane) {
    const size_t b = group0 + lane;
    const Fp8Access<POL, kTreeStoreAux, uint8_t> acc{POL ? group0 * 16 : b * 16, POL ? lane * 16u : 0u};
    Fp8Words raw[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    float s[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((s[I] = mx_scale32(mx.in_scales[I][b])), ...); }(std::make_index_sequence<P>{});
    uint32_t A = 0;
    Fp8Half S[4];
    S[0] = mxfp4_piece<ALG, P, 0>(raw, s, mx.r, A);
    S[1] = mxfp4_piece<ALG, P, 1>(raw, s, mx.r, A);
    S[2] = mxfp4_piece<ALG, P, 2>(raw, s, mx.r, A);
    S[3] = mxfp4_piece<ALG, P, 3>(raw, s, mx.r, A);
    const uint32_t e_out = mxfp4_scale_byte(A);
    const float inv = mx_inv_scale(e_out);
    Fp8Words out;
#pragma unroll
    for (int K = 0; K < 4; ++K) {
#pragma unroll
        for (int k = 0; k < 4; ++k) S[K].p[k] = S[K].p[k] * inv;
        const uint32_t w = fp4_narrow_sr_word(S[K], philox4x32_10(q0 + 4 * b + K, seed));
        out.w[K] = e_out == 255u ? 0u : w;  // a NaN block: scale byte 255, every nibble 0
    }
    acc.store(ptrs.out[0], out);
    mx.out_scales[b] = static_cast<uint8_t>(e_out);
}

// mxfp4_kernel's grid and ragged block.
template <int ALG, int P>
__global__ void __launch_bounds__(256) mxfp4_sr_kernel(PeerPtrs ptrs, MxArgs mx, size_t n, int pol) {
    const uint64_t seed = *mx.seed;
    const uint64_t q0 = mx.first >> 3;
    const size_t nblk = n / 32;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nblk; tile += gridDim.x)
            if (tile * B + threadIdx.x < nblk) mxfp4_sr_block<ALG, P, true>(ptrs, mx, seed, q0, tile * B, threadIdx.x);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t b = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; b < nblk; b += stride)
            mxfp4_sr_block<ALG, P, false>(ptrs, mx, seed, q0, b, 0u);
    }
    const size_t first = nblk * 32;
    if (blockIdx.x == 0 && threadIdx.x < 64 && first < n) {  // one whole wave: uniform for the exchanges below
        const size_t i = first + threadIdx.x;  // first is even: lanes 2j and 2j + 1 share byte first / 2 + j
        const bool have = i < n;               // 1..31 lanes
        const unsigned shift = (threadIdx.x & 1u) * 4u;
        float S = 0.0f;
        if (have) {
            Lanes<float, 1> v[P + kNumSteps<ALG, P>];
            [&]<size_t... I>(std::index_sequence<I...>) {
                ((v[I].v[0] = fp4_widen_sw(static_cast<uint32_t>(static_cast<const uint8_t*>(ptrs.in[I])[i / 2]) >> shift) *
                              mx_scale32(mx.in_scales[I][nblk])),
                 ...);
            }(std::make_index_sequence<P>{});
            run_steps<OpSum, float, 1, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
            S = v[kOut<ALG, P, 0>].v[0] * mx.r;
        }
        uint32_t A = mx_abs_bits(S);  // 0 on the lanes beyond the block
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
        const uint32_t e_out = mxfp4_scale_byte(A);
        const uint64_t j = mx.first + i;
        const uint32_t sr = fp4_narrow_sr(S * mx_inv_scale(e_out), sr_bits(philox4x32_10(j >> 3, seed), j));
        // beyond the block: code 0, which is what an odd bucket's last high nibble takes
        const uint32_t code = have && e_out != 255u ? sr : 0u;
        const uint32_t next = static_cast<uint32_t>(__shfl_xor(static_cast<int>(code), 1, 64));
        if (have && shift == 0u) static_cast<uint8_t*>(ptrs.out[0])[i / 2] = static_cast<uint8_t>(code | (next << 4));
        if (threadIdx.x == 0) mx.out_scales[nblk] = static_cast<uint8_t>(e_out);
    }
}

template <int ALG, int P>
void mxfp4_sr_one(const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(n / 32, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 8);  // mxfp4_one's in-flight budget
    mxfp4_sr_kernel<ALG, P><<<grid, kFusedBlock, lds, s>>>(ptrs, mx, n, fused_policy(false, P));
}

template <int ALG, int... I>
constexpr std::array<MxFn, sizeof...(I)> mxfp4_sr_table(std::integer_sequence<int, I...>) {
    return {&mxfp4_sr_one<ALG, I + 2>...};
}

template <int ALG>
int mxfp4_sr_unit(int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "fused MXFP4 stochastic-rounding kernel needs 2 <= P <= " + std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    static constexpr auto table = mxfp4_sr_table<ALG>(std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{});
    table[P - 2](ptrs, mx, n, s);
    return check_launch("fused MXFP4 stochastic-rounding P-way kernel launch");
}

}  // namespace fmi::dev
