// fmi_mxfp6_impl.h — the MXFP6 kernels of fmi_dev_reduce_tree_mx (include/fmi_dev.h): the sum or mean of block-scaled
// E2M3 / E3M2 buckets, four elements to three bytes, one E8M0 scale byte per 32 elements, and of
// fmi_dev_reduce_tree_mx_sr at those types. Included by the fmi_fused_mxfp6_*.hip translation units, fmi_mx.hip and
// fmi_mx_sr.hip alone.
//
//   v_p = fl32(widen(x_p) * scale32(e_p[b]));  S = F32_program(v);  S = fl32(S * r)      (r = fl32(1 / P) or 1)
//   f32 output:   out = S
//   FP6 output:   per block b  A = umax bits(|S|);  e_out = mxfp6_scale_byte(A);  out = narrow(fl32(S * 2^(127 - e_out)))
//
// The element type is the template argument M, its mantissa bits: 3 is E2M3 (FMI_F6E2M3), 2 is E3M2 (FMI_F6E3M2).
// The fused kernel has the shape of mxfp4_kernel (fmi_mxfp4_impl.h): both access policies, its in-flight budget, r as an
// argument, a lane owning whole blocks (no cross-lane exchange for the amax, its own scale bytes). What differs:
//   - a block is 24 B, which is not a 16-B multiple, so ONE LANE IS TWO CONSECUTIVE BLOCKS: 48 B per peer, three 16-B
//     loads at lane stride 48, 16-B aligned whenever the bucket is. The vector path covers the n / 64 block pairs;
//   - the program runs over the first block and then the second, each in four pieces of 8 elements (Fp8Half). Piece K
//     is bits 48 K .. 48 K + 47 of the block's 192: dwords 0, 1 (low half) for K = 0, dwords 1 (high half), 2 for K = 1,
//     and the same of dwords 3..5 for K = 2, 3. The piece's 48 bits are the first 8 elements of a conversion operand
//     whose other elements are not read back. With an f32 output a piece is stored as soon as it is computed; with an
//     FP6 output the block's 32 results are kept until its scale is known, then narrowed by ONE conversion;
//   - the leftovers, an odd last whole block and the ragged tail (up to 63 elements in all), go to the first wave of
//     workgroup 0, one element per lane: lanes 0..31 are one block and lanes 32..63 the other, so a block's amax is five
//     exchanges inside its half. Four neighbouring lanes exchange their codes and write their three bytes, one byte per
//     lane, so no byte is written twice and the unused high bits of the bucket's last byte are 0.
// Conversions. The vector path widens with v_cvt_scalef32_pk32_f32_fp6 / _bf6 and narrows with
// v_cvt_scalef32_2xpk16_fp6_f32 / _bf6_f32, all at the scale operand 1.0f: the E8M0 scale and the inverse scale are
// applied by separate IEEE f32 multiplies. What the instructions were found to do is in DESIGN.md §5. The leftovers, the
// fallback's kernels (fmi_mx.hip) and the host use the integer-code forms below.
//
// Stochastic rounding (the template flag SR, FP6 output only) is the same kernel with narrow_sr (fmi_mx_sr.h,
// sr_magnitude<3, 0> / <2, -2>) where the round-to-nearest one narrows: block b's elements are at the stream positions
// first + 32 b + k, four whole Philox groups, q = (first >> 3) + 4 b + K for piece K, whose output word k holds r of the
// piece's elements 2 k and 2 k + 1. The codes are packed with shifts: the hardware's SR conversion is not used.
#pragma once

#include "fmi_mx_impl.h"

namespace fmi::dev {

// The grid of element type M: the smallest normal exponent, what scales the placed bits to the value (2^(127 - bias)),
// and the scale rule's EMAX and largest mantissa (7.5 = 1.875 * 2^2, 28 = 1.75 * 2^4).
template <int M>
struct Fp6 {
    static_assert(M == 3 || M == 2, "E2M3 (M = 3) or E3M2 (M = 2)");
    static constexpr int kEmin = M == 3 ? 0 : -2;
    static constexpr int kEmax = M == 3 ? 2 : 4;
    static constexpr uint32_t kMaxMant = M == 3 ? 0x700000u : 0x600000u;
    static constexpr uint32_t kUnbias = (M == 3 ? 253u : 251u) << 23;  // 2^126, 2^124
};

// widen: the five magnitude bits placed at the top of an f32's mantissa and the bottom of its exponent (an exponent
// field of 0 is then an f32 subnormal, exactly as in the element), times 2^(127 - bias): exact. Bit 5 is the sign.
template <int M>
__host__ __device__ __forceinline__ float fp6_widen_sw(uint32_t c) {
    const float placed = __builtin_bit_cast(float, (c & 31u) << (23 - M));
    const float v = placed * __builtin_bit_cast(float, Fp6<M>::kUnbias);
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | ((c & 32u) << 26));
}

// narrow: round to nearest on the 32 magnitudes, ties to the even code; defined for finite |y| <= the largest element.
// sr_magnitude's exact steps (fmi_mx_sr.h): t = |y| / step, k = floor(t), frac = t - k; up where frac is above one half,
// or on it with k odd (the code's parity is k's: the exponent field sits above M >= 2 bits).
template <int M>
__host__ __device__ __forceinline__ uint32_t fp6_narrow_sw(float y) {
    constexpr uint32_t kMinExp = static_cast<uint32_t>(Fp6<M>::kEmin + 127) << 23;
    const uint32_t u = __builtin_bit_cast(uint32_t, y), a = u & 0x7FFFFFFFu;
    const uint32_t eb = (a & 0x7F800000u) > kMinExp ? (a & 0x7F800000u) : kMinExp;
    const float t = __builtin_bit_cast(float, a) * __builtin_bit_cast(float, (static_cast<uint32_t>(254 + M) << 23) - eb);
    const float k = __builtin_floorf(t);
    const float frac = t - k;
    const uint32_t ki = static_cast<uint32_t>(k);
    const uint32_t up = (frac > 0.5f || (frac == 0.5f && (ki & 1u))) ? 1u : 0u;
    return ((((eb - kMinExp) >> 23) << M) + ki + up) | ((u >> 26) & 32u);
}

template <int M>
__host__ __device__ __forceinline__ uint32_t fp6_narrow_sr(float y, uint32_t r) {
    return sr_magnitude<M, Fp6<M>::kEmin>(y, r) | ((__builtin_bit_cast(uint32_t, y) >> 26) & 32u);
}

template <int M>
__host__ __device__ __forceinline__ uint32_t mxfp6_scale_byte(uint32_t A) {
    const int f = static_cast<int>(A >> 23);
    const int e = f - Fp6<M>::kEmax + ((A & 0x7FFFFFu) > Fp6<M>::kMaxMant ? 1 : 0);
    return f == 255 ? 255u : static_cast<uint32_t>(e < 0 ? 0 : e);
}

// Element i of a packed bucket, i < n: bits 6 i .. 6 i + 5 of the byte string. The second byte is read only where
// the element reaches into it, and then it is one of the bucket's ceil(3 n / 4).
__host__ __device__ __forceinline__ uint32_t fp6_load_code(const uint8_t* bytes, size_t i) {
    const size_t bit = 6 * i;
    const unsigned sh = static_cast<unsigned>(bit % 8);
    uint32_t w = bytes[bit / 8];
    if (sh > 2u) w |= static_cast<uint32_t>(bytes[bit / 8 + 1]) << 8;
    return (w >> sh) & 63u;
}

// The three bytes of four codes.
__host__ __device__ __forceinline__ uint32_t fp6_pack4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    return c0 | (c1 << 6) | (c2 << 12) | (c3 << 18);
}

using u32x6 = unsigned int __attribute__((ext_vector_type(6)));
using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x32 = float __attribute__((ext_vector_type(32)));

// One lane's 48 B of a bucket: block h is dwords 6 h .. 6 h + 5.
struct Fp6Pair {
    uint32_t w[12];
};

// The 8 elements of piece K of the block at w[0..5].
template <int M, int K>
__device__ __forceinline__ Fp8Half fp6_widen_piece(const uint32_t* w) {
    const uint32_t* t = w + 3 * (K / 2);
    u32x6 x = {0u, 0u, 0u, 0u, 0u, 0u};
    if constexpr (K % 2 == 0) {
        x[0] = t[0], x[1] = t[1];
    } else {
        x[0] = __builtin_amdgcn_alignbit(t[2], t[1], 16), x[1] = t[2] >> 16;
    }
    f32x32 r;
    if constexpr (M == 3)
        r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(x, 1.0f);
    else
        r = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(x, 1.0f);
    return {{f32x2{r[0], r[1]}, f32x2{r[2], r[3]}, f32x2{r[4], r[5]}, f32x2{r[6], r[7]}}};
}

// A block's 32 values, piece K's element 2 k + j at S[K].p[k] lane j, into its six dwords. The conversion INTERLEAVES
// its operands: element 2 i of the result is the first operand's value i, element 2 i + 1 the second's (measured on
// an MI355X), so the even elements go into one operand and the odd ones into the other.
template <int M>
__device__ __forceinline__ void fp6_narrow_block(uint32_t* w, const Fp8Half* S) {
    f32x16 a, b;
#pragma unroll
    for (int K = 0; K < 4; ++K)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[4 * K + k] = S[K].p[k].x, b[4 * K + k] = S[K].p[k].y;
    u32x6 r;
    if constexpr (M == 3)
        r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, 1.0f);
    else
        r = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, 1.0f);
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = r[k];
}

// The 48 bits of one piece under narrow_sr, from the Philox output of its 8 elements: bits 0..31 and 32..47.
template <int M>
__device__ __forceinline__ uint64_t fp6_narrow_sr_piece(const Fp8Half& v, const Philox4& W) {
    uint64_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t two = fp6_narrow_sr<M>(v.p[k].x, W.w[k] & 0xFFFFu) | (fp6_narrow_sr<M>(v.p[k].y, W.w[k] >> 16) << 6);
        bits |= static_cast<uint64_t>(two) << (12 * k);
    }
    return bits;
}

// Piece K of the block at w[0..5]: widen and scale every peer, run the program, times r, fold |S| into A.
template <int M, int ALG, int P, int K, int H>
__device__ __forceinline__ Fp8Half mxfp6_piece(const Fp6Pair* raw, const float* s, float r, uint32_t& A) {
    Fp8Half v[P + kNumSteps<ALG, P>];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        v[p] = fp6_widen_piece<M, K>(raw[p].w + 6 * H);
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

// Block H (0 or 1) of the lane's pair u: the bucket's block 2 u + H. out: the lane's 12 output dwords (FP6 output).
template <int M, int ALG, int P, bool OUT32, bool SR, bool POL, int H>
__device__ __forceinline__ void mxfp6_block(const PeerPtrs& ptrs, const MxArgs& mx, const Fp6Pair* raw, uint64_t seed, uint64_t q0, size_t group0,
                                            unsigned lane, Fp6Pair& out) {
    const size_t b = 2 * (group0 + lane) + H;
    float s[P];
    [&]<size_t... I>(std::index_sequence<I...>) { ((s[I] = mx_scale32(mx.in_scales[I][b])), ...); }(std::make_index_sequence<P>{});
    uint32_t A = 0;
    if constexpr (OUT32) {
        // the lane's 64 f32 values, 256 B: piece K of block H is bytes 128 H + 32 K .. + 31 of them
        [&]<size_t... K>(std::index_sequence<K...>) {
            (([&] {
                 const Fp8Half S = mxfp6_piece<M, ALG, P, K, H>(raw, s, mx.r, A);
#pragma unroll
                 for (int k = 0; k < 2; ++k) {
                     Lanes<float, 4> q;
                     q.v[0] = S.p[2 * k].x, q.v[1] = S.p[2 * k].y, q.v[2] = S.p[2 * k + 1].x, q.v[3] = S.p[2 * k + 1].y;
                     if constexpr (POL)
                         store_tile<kTreeStoreAux, float, 4>(ptrs.out[0], group0 * 256, lane * 256u + H * 128u + K * 32u + k * 16u, q);
                     else
                         store_lanes<kFusedNT, float, 4>(static_cast<float*>(ptrs.out[0]) + b * 32 + K * 8 + k * 4, q);
                 }
             }()),
             ...);
        }(std::make_index_sequence<4>{});
    } else {
        Fp8Half S[4];
        S[0] = mxfp6_piece<M, ALG, P, 0, H>(raw, s, mx.r, A);
        S[1] = mxfp6_piece<M, ALG, P, 1, H>(raw, s, mx.r, A);
        S[2] = mxfp6_piece<M, ALG, P, 2, H>(raw, s, mx.r, A);
        S[3] = mxfp6_piece<M, ALG, P, 3, H>(raw, s, mx.r, A);
        const uint32_t e_out = mxfp6_scale_byte<M>(A);
        const float inv = mx_inv_scale(e_out);
#pragma unroll
        for (int K = 0; K < 4; ++K)
#pragma unroll
            for (int k = 0; k < 4; ++k) S[K].p[k] = S[K].p[k] * inv;
        uint32_t* w = out.w + 6 * H;
        if constexpr (SR) {
            uint64_t bits[4];
#pragma unroll
            for (int K = 0; K < 4; ++K) bits[K] = fp6_narrow_sr_piece<M>(S[K], philox4x32_10(q0 + 4 * b + K, seed));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint64_t lo = bits[2 * j], hi = bits[2 * j + 1];  // 48 bits each: 96 bits, three dwords
                w[3 * j] = static_cast<uint32_t>(lo);
                w[3 * j + 1] = static_cast<uint32_t>(lo >> 32) | (static_cast<uint32_t>(hi) << 16);
                w[3 * j + 2] = static_cast<uint32_t>(hi >> 16);
            }
        } else {
            fp6_narrow_block<M>(w, S);
        }
        // a NaN block: scale byte 255, every code 0
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = e_out == 255u ? 0u : w[k];
        mx.out_scales[b] = static_cast<uint8_t>(e_out);
    }
}

// POL, group0, lane, seed, q0: as mx_group. u = group0 + lane is the lane's PAIR of blocks: bytes 48 u .. 48 u + 47 of
// every bucket.
template <int M, int ALG, int P, bool OUT32, bool SR, bool POL>
__device__ __forceinline__ void mxfp6_pair(const PeerPtrs& ptrs, const MxArgs& mx, uint64_t seed, uint64_t q0, size_t group0, unsigned lane) {
    const size_t u = group0 + lane;
    Fp6Pair raw[P];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const Fp8Access<POL, kTreeStoreAux, uint8_t> acc{POL ? group0 * 48 : u * 48 + j * 16, POL ? lane * 48u + j * 16u : 0u};
        [&]<size_t... I>(std::index_sequence<I...>) {
            (([&] {
                 const Fp8Words x = acc.load(ptrs.in[I]);
#pragma unroll
                 for (int k = 0; k < 4; ++k) raw[I].w[4 * j + k] = x.w[k];
             }()),
             ...);
        }(std::make_index_sequence<P>{});
    }
    Fp6Pair out;
    mxfp6_block<M, ALG, P, OUT32, SR, POL, 0>(ptrs, mx, raw, seed, q0, group0, lane, out);
    mxfp6_block<M, ALG, P, OUT32, SR, POL, 1>(ptrs, mx, raw, seed, q0, group0, lane, out);
    if constexpr (!OUT32) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const Fp8Access<POL, kTreeStoreAux, uint8_t> acc{POL ? group0 * 48 : u * 48 + j * 16, POL ? lane * 48u + j * 16u : 0u};
            acc.store(ptrs.out[0], Fp8Words{{out.w[4 * j], out.w[4 * j + 1], out.w[4 * j + 2], out.w[4 * j + 3]}});
        }
    }
}

// The grid of mxfp4_kernel over the n / 64 block pairs; the first wave of workgroup 0 takes the leftovers.
template <int M, int ALG, int P, bool OUT32, bool SR>
__global__ void __launch_bounds__(256) mxfp6_kernel(PeerPtrs ptrs, MxArgs mx, size_t n, int pol) {
    static_assert(!(SR && OUT32), "stochastic rounding exists only with the element type's own output");
    uint64_t seed = 0, q0 = 0;  // a round-to-nearest kernel reads neither
    if constexpr (SR) seed = *mx.seed, q0 = mx.first >> 3;
    const size_t npair = n / 64;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < npair; tile += gridDim.x)
            if (tile * B + threadIdx.x < npair) mxfp6_pair<M, ALG, P, OUT32, SR, true>(ptrs, mx, seed, q0, tile * B, threadIdx.x);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t u = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; u < npair; u += stride)
            mxfp6_pair<M, ALG, P, OUT32, SR, false>(ptrs, mx, seed, q0, u, 0u);
    }
    const size_t first = npair * 64;
    if (blockIdx.x == 0 && threadIdx.x < 64 && first < n) {  // one whole wave: uniform for the exchanges below
        // first is a multiple of 64 elements and of 48 bytes: lanes 4 g .. 4 g + 3 share bytes first * 3 / 4 + 3 g .. + 2
        const size_t i = first + threadIdx.x;
        const bool have = i < n;  // 1..63 lanes
        const size_t blk = i / 32;  // lanes 0..31 and 32..63: a block each
        float S = 0.0f;
        if (have) {
            Lanes<float, 1> v[P + kNumSteps<ALG, P>];
            [&]<size_t... I>(std::index_sequence<I...>) {
                ((v[I].v[0] = fp6_widen_sw<M>(fp6_load_code(static_cast<const uint8_t*>(ptrs.in[I]), i)) * mx_scale32(mx.in_scales[I][blk])), ...);
            }(std::make_index_sequence<P>{});
            run_steps<OpSum, float, 1, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
            S = v[kOut<ALG, P, 0>].v[0] * mx.r;
        }
        if constexpr (OUT32) {
            if (have) static_cast<float*>(ptrs.out[0])[i] = S;
        } else {
            uint32_t A = mx_abs_bits(S);  // 0 on the lanes beyond the bucket
#pragma unroll
            for (int d = 16; d > 0; d >>= 1) A = max(A, static_cast<uint32_t>(__shfl_xor(static_cast<int>(A), d, 64)));
            const uint32_t e_out = mxfp6_scale_byte<M>(A);
            // beyond the bucket: code 0, which is what the last byte's unused bits take
            uint32_t code;
            if constexpr (SR) {
                const uint64_t j = mx.first + i;
                const uint32_t sr = fp6_narrow_sr<M>(S * mx_inv_scale(e_out), sr_bits(philox4x32_10(j >> 3, seed), j));
                code = have && e_out != 255u ? sr : 0u;
            } else {
                code = have && e_out != 255u ? fp6_narrow_sw<M>(S * mx_inv_scale(e_out)) : 0u;
            }
            const unsigned l4 = threadIdx.x & 3u, base = threadIdx.x & ~3u;
            const uint32_t three = fp6_pack4(static_cast<uint32_t>(__shfl(static_cast<int>(code), base, 64)),
                                             static_cast<uint32_t>(__shfl(static_cast<int>(code), base + 1, 64)),
                                             static_cast<uint32_t>(__shfl(static_cast<int>(code), base + 2, 64)),
                                             static_cast<uint32_t>(__shfl(static_cast<int>(code), base + 3, 64)));
            const size_t byte = first / 4 * 3 + (threadIdx.x / 4) * 3 + l4;
            if (l4 < 3u && byte < (3 * n + 3) / 4) static_cast<uint8_t*>(ptrs.out[0])[byte] = static_cast<uint8_t>(three >> (8 * l4));
            if (have && threadIdx.x % 32 == 0) mx.out_scales[blk] = static_cast<uint8_t>(e_out);
        }
    }
}

template <int M, int ALG, bool OUT32, bool SR, int P>
void mxfp6_one(const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(n / 64, kFusedBlock), kFusedGridCap));
    // mxfp4_one's in-flight budget: a workgroup loads 12 KiB per peer
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 8);
    mxfp6_kernel<M, ALG, P, OUT32, SR><<<grid, kFusedBlock, lds, s>>>(ptrs, mx, n, fused_policy(false, P));
}

template <int M, int ALG, bool OUT32, bool SR, int... I>
constexpr std::array<MxFn, sizeof...(I)> mxfp6_table(std::integer_sequence<int, I...>) {
    return {&mxfp6_one<M, ALG, OUT32, SR, I + 2>...};
}

// mx_unit's signature and its rule for SR; dtype is FMI_F6E2M3 or FMI_F6E3M2 (launch_fused_mx sends nothing else here).
template <int ALG, bool SR>
int mxfp6_unit(int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, std::string(SR ? "fused MXFP6 stochastic-rounding" : "fused MXFP6") + " kernel needs 2 <= P <= " +
                                         std::to_string(sched::kMaxFusedPeers) + ", got " + std::to_string(P));
    const auto launch = [&]<int M>() {
        constexpr auto seq = std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{};
        static constexpr auto same = mxfp6_table<M, ALG, false, SR>(seq);
        if constexpr (SR) {
            same[P - 2](ptrs, mx, n, s);
        } else {
            static constexpr auto wide = mxfp6_table<M, ALG, true, false>(seq);
            (out_dtype == FMI_F32 ? wide : same)[P - 2](ptrs, mx, n, s);
        }
    };
    if (dtype == FMI_F6E2M3)
        launch.template operator()<3>();
    else
        launch.template operator()<2>();
    return check_launch(SR ? "fused MXFP6 stochastic-rounding P-way kernel launch" : "fused MXFP6 P-way kernel launch");
}

}  // namespace fmi::dev
