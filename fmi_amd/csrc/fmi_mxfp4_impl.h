// fmi_mxfp4_impl.h — the MXFP4 kernels of fmi_dev_reduce_tree_mx (include/fmi_dev.h): the sum or mean of block-scaled
// E2M1 buckets, two elements to a byte, one E8M0 scale byte per 32 elements, and of fmi_dev_reduce_tree_mx_sr at that
// type. Included by the fmi_fused_mxfp4_*.hip translation units, fmi_mx.hip and fmi_mx_sr.hip alone.
//
//   v_p = fl32(widen(x_p) * scale32(e_p[b]));  S = F32_program(v);  S = fl32(S * r)      (r = fl32(1 / P) or 1)
//   f32 output:   out = S
//   E2M1 output:  per block b  A = umax bits(|S|);  e_out = mxfp4_scale_byte(A);  out = narrow(fl32(S * 2^(127 - e_out)))
//
// The fused kernel has the shape of fp8_mx_kernel (fmi_mx_impl.h): both access policies, its in-flight budget, r as an
// argument. What differs:
//   - ONE LANE IS ONE BLOCK: its 16-B word per peer holds 32 elements, so the block's amax needs no cross-lane exchange,
//     the vector path covers the n / 32 whole blocks, and each lane loads its own scale byte per peer and stores its
//     own output scale byte;
//   - the program runs over 32 f32 values per lane in four pieces of 8 (Fp8Half), piece k from word k of every peer's
//     16 B: a word is dead once its piece ran, so the live set shrinks by P words while it grows by 8 results. With an
//     f32 output a piece is stored (two 16-B stores) as soon as it is computed; with an E2M1 output the 32 results are
//     kept until the block's scale is known;
//   - the ragged last block (n % 32 elements, possibly an odd count) goes to the first wave of workgroup 0, one element
//     per lane; the even lane writes the byte from its own and its neighbour's nibble, so no byte is written twice and
//     the unused high nibble of an odd bucket's last byte is 0.
// Conversions. The vector path widens with v_cvt_scalef32_pk_f32_fp4 and narrows with v_cvt_scalef32_pk_fp4_f32, both
// at the scale operand 1.0f: the E8M0 scale and the inverse scale are applied by separate IEEE f32 multiplies
// (v_pk_mul_f32), so what the instructions do with a NaN scale or the subnormal-encoded 2^-127 never matters. The
// ragged block, the fallback's kernels (fmi_mx.hip) and the host use the integer-code forms below.
//
// Stochastic rounding (fmi_dev_reduce_tree_mx_sr at FMI_F4E2M1; the template flag SR, E2M1 output only) is the same
// kernel with narrow_sr (fmi_mx_sr.h) where the round-to-nearest one narrows. One lane is one block b of 32 elements at
// the stream positions first + 32 b + k: four whole Philox groups, q = (first >> 3) + 4 b + K for piece K, whose output
// word k holds r of the piece's elements 2 k and 2 k + 1, the two lanes of Fp8Half::p[k] and the two nibbles of byte k of
// output word K. A group's four words are dead once its piece is narrowed, so one Philox state is live at a time beside
// the 32 results. That narrowing is a few exact f32 operations per element, not the packed conversion instruction: that
// one rounds to nearest, and its stochastic form was not shown to follow this definition.
#pragma once

#include "fmi_mx_impl.h"

namespace fmi::dev {

// widen: the 16-entry table as bits. Codes 0..7: 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign.
__host__ __device__ __forceinline__ float fp4_widen_sw(uint32_t c) {
    const uint32_t m = c & 7u;
    // m >= 2: exponent field (m >> 1) + 126, mantissa bit m & 1; m = 1: 0.5; m = 0: 0
    uint32_t b = (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);
    b = m == 1u ? 0x3F000000u : b;
    b = m == 0u ? 0u : b;
    return __builtin_bit_cast(float, b | ((c & 8u) << 28));
}

// narrow: round to nearest on the eight magnitudes, ties to the even code; defined for finite |y| <= 6. On the bits of
// |y| (monotonic for non-negative floats): a midpoint whose lower neighbour has an even code stays below (>), one whose
// upper neighbour has the even code goes up (>=).
__host__ __device__ __forceinline__ uint32_t fp4_narrow_sw(float y) {
    const uint32_t u = __builtin_bit_cast(uint32_t, y), a = u & 0x7FFFFFFFu;
    const uint32_t c = (a > 0x3E800000u) + (a >= 0x3F400000u) + (a > 0x3FA00000u) + (a >= 0x3FE00000u) +  // .25 .75 1.25 1.75
                       (a > 0x40200000u) + (a >= 0x40600000u) + (a > 0x40A00000u);                       // 2.5 3.5 5
    return c | ((u >> 28) & 8u);
}

// mx_scale_byte at EMAX = 2: the largest finite element is 6 = 1.5 * 2^2 (mantissa bits 0x400000).
__host__ __device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t A) {
    const int f = static_cast<int>(A >> 23);
    const int e = f - 2 + ((A & 0x7FFFFFu) > 0x400000u ? 1 : 0);
    return f == 255 ? 255u : static_cast<uint32_t>(e < 0 ? 0 : e);
}

// The 8 elements of one 32-bit word, byte j holding elements 2j (bits 3:0) and 2j + 1 (bits 7:4).
__device__ __forceinline__ Fp8Half fp4_widen_word(uint32_t w) {
    return {{__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1),
             __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3)}};
}
__device__ __forceinline__ uint32_t fp4_narrow_word(const Fp8Half& v) {
    uint32_t w = 0u;
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v.p[0].x, v.p[0].y, 1.0f, 0);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v.p[1].x, v.p[1].y, 1.0f, 1);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v.p[2].x, v.p[2].y, 1.0f, 2);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v.p[3].x, v.p[3].y, 1.0f, 3);
    return w;
}

// Piece K of a lane's block (elements 8K .. 8K + 7): widen and scale every peer, run the program, times r, fold |S|
// into A.
template <int ALG, int P, int K>
__device__ __forceinline__ Fp8Half mxfp4_piece(const Fp8Words* raw, const float* s, float r, uint32_t& A) {
    Fp8Half v[P + kNumSteps<ALG, P>];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        v[p] = fp4_widen_word(raw[p].w[K]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[p].p[k] = v[p].p[k] * s[p];
    }
    fp8_run_steps<OpSum, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    Fp8Half S = v[kOut<ALG, P, 0>];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        S.p[k] = S.p[k] * r;
        A = max(A, max(mx_abs_bits(S.p[k].x), mx_abs_bits(S.p[k].y)));
    }
    return S;
}

// The 8 nibbles of one piece under narrow_sr, from the Philox output of its 8 elements.
__device__ __forceinline__ uint32_t fp4_narrow_sr_word(const Fp8Half& v, const Philox4& W) {
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w |= (fp4_narrow_sr(v.p[k].x, W.w[k] & 0xFFFFu) | (fp4_narrow_sr(v.p[k].y, W.w[k] >> 16) << 4)) << (8 * k);
    return w;
}

// POL, group0, lane, seed, q0: as mx_group. b = group0 + lane is the lane's BLOCK: bytes 16 b .. 16 b + 15 of every bucket.
template <int ALG, int P, bool OUT32, bool SR, bool POL>
__device__ __forceinline__ void mxfp4_block(const PeerPtrs& ptrs, const MxArgs& mx, uint64_t seed, uint64_t q0, size_t group0, unsigned lane) {
    const size_t b = group0 + lane;
    const Fp8Access<POL, kTreeStoreAux, uint8_t> acc{POL ? group0 * 16 : b * 16, POL ? lane * 16u : 0u};
    Fp8Words raw[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    float s[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((s[I] = mx_scale32(mx.in_scales[I][b])), ...); }(std::make_index_sequence<P>{});
    uint32_t A = 0;
    if constexpr (OUT32) {
        // 32 f32 values, 128 B: piece K is bytes 32 K .. 32 K + 31 of them, stored as soon as it is known
        [&]<size_t... K>(std::index_sequence<K...>) {
            (([&] {
                 const Fp8Half S = mxfp4_piece<ALG, P, K>(raw, s, mx.r, A);
#pragma unroll
                 for (int k = 0; k < 2; ++k) {
                     Lanes<float, 4> q;
                     q.v[0] = S.p[2 * k].x, q.v[1] = S.p[2 * k].y, q.v[2] = S.p[2 * k + 1].x, q.v[3] = S.p[2 * k + 1].y;
                     if constexpr (POL)
                         store_tile<kTreeStoreAux, float, 4>(ptrs.out[0], group0 * 128, lane * 128u + K * 32u + k * 16u, q);
                     else
                         store_lanes<kFusedNT, float, 4>(static_cast<float*>(ptrs.out[0]) + b * 32 + K * 8 + k * 4, q);
                 }
             }()),
             ...);
        }(std::make_index_sequence<4>{});
    } else {
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
            // a NaN block: scale byte 255, every nibble 0
            if constexpr (SR) {
                const uint32_t w = fp4_narrow_sr_word(S[K], philox4x32_10(q0 + 4 * b + K, seed));
                out.w[K] = e_out == 255u ? 0u : w;
            } else {
                out.w[K] = e_out == 255u ? 0u : fp4_narrow_word(S[K]);
            }
        }
        acc.store(ptrs.out[0], out);
        mx.out_scales[b] = static_cast<uint8_t>(e_out);
    }
}

// The grid of fp8_mx_kernel over the n / 32 whole blocks; the first wave of workgroup 0 takes the ragged last block.
template <int ALG, int P, bool OUT32, bool SR>
__global__ void __launch_bounds__(256) mxfp4_kernel(PeerPtrs ptrs, MxArgs mx, size_t n, int pol) {
    static_assert(!(SR && OUT32), "stochastic rounding exists only with the element type's own output");
    uint64_t seed = 0, q0 = 0;  // a round-to-nearest kernel reads neither
    if constexpr (SR) seed = *mx.seed, q0 = mx.first >> 3;
    const size_t nblk = n / 32;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nblk; tile += gridDim.x)
            if (tile * B + threadIdx.x < nblk) mxfp4_block<ALG, P, OUT32, SR, true>(ptrs, mx, seed, q0, tile * B, threadIdx.x);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t b = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; b < nblk; b += stride)
            mxfp4_block<ALG, P, OUT32, SR, false>(ptrs, mx, seed, q0, b, 0u);
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
        if constexpr (OUT32) {
            if (have) static_cast<float*>(ptrs.out[0])[i] = S;
        } else {
            uint32_t A = mx_abs_bits(S);  // 0 on the lanes beyond the block
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
            const uint32_t e_out = mxfp4_scale_byte(A);
            // beyond the block: code 0, which is what an odd bucket's last high nibble takes
            uint32_t code;
            if constexpr (SR) {
                const uint64_t j = mx.first + i;
                const uint32_t sr = fp4_narrow_sr(S * mx_inv_scale(e_out), sr_bits(philox4x32_10(j >> 3, seed), j));
                code = have && e_out != 255u ? sr : 0u;
            } else {
                code = have && e_out != 255u ? fp4_narrow_sw(S * mx_inv_scale(e_out)) : 0u;
            }
            const uint32_t next = static_cast<uint32_t>(__shfl_xor(static_cast<int>(code), 1, 64));
            if (have && shift == 0u) static_cast<uint8_t*>(ptrs.out[0])[i / 2] = static_cast<uint8_t>(code | (next << 4));
            if (threadIdx.x == 0) mx.out_scales[nblk] = static_cast<uint8_t>(e_out);
        }
    }
}

template <int ALG, bool OUT32, bool SR, int P>
void mxfp4_one(const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(n / 32, kFusedBlock), kFusedGridCap));
    // mx_one's in-flight budget (fmi_mx_impl.h): a workgroup loads the same 4 KiB per peer
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 8);
    mxfp4_kernel<ALG, P, OUT32, SR><<<grid, kFusedBlock, lds, s>>>(ptrs, mx, n, fused_policy(false, P));
}

template <int ALG, bool OUT32, bool SR, int... I>
constexpr std::array<MxFn, sizeof...(I)> mxfp4_table(std::integer_sequence<int, I...>) {
    return {&mxfp4_one<ALG, OUT32, SR, I + 2>...};
}

// mx_unit's signature and its rule for SR; dtype is FMI_F4E2M1 (launch_fused_mx sends nothing else here).
template <int ALG, bool SR>
int mxfp4_unit(int, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, std::string(SR ? "fused MXFP4 stochastic-rounding" : "fused MXFP4") + " kernel needs 2 <= P <= " +
                                         std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    constexpr auto seq = std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{};
    static constexpr auto same = mxfp4_table<ALG, false, SR>(seq);
    if constexpr (SR) {
        same[P - 2](ptrs, mx, n, s);
    } else {
        static constexpr auto wide = mxfp4_table<ALG, true, false>(seq);
        (out_dtype == FMI_F32 ? wide : same)[P - 2](ptrs, mx, n, s);
    }
    return check_launch(SR ? "fused MXFP4 stochastic-rounding P-way kernel launch" : "fused MXFP4 P-way kernel launch");
}

}  // namespace fmi::dev
