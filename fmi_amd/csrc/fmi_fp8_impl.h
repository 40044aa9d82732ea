// fmi_fp8_impl.h — the fused f32-accumulating P-way kernels of the 8-bit floats (FMI_F8E4M3 / FMI_F8E5M2 with
// FMI_ACC_F32, and FMI_OP_AVG on them), included by the fmi_fused_fp8_acc32_*.hip translation units alone.
//
// out = narrow(F32_program(widen(x))), as for the 16-bit floats (Acc32<T>, fmi_kernels.h), but a 16-B access holds
// 16 elements: 16 peers x 16 f32 lanes would be 256 VGPRs of inputs alone. So a thread keeps the P raw 16-B words it
// loaded (4 VGPRs per peer) and evaluates the program twice, over 8 lanes each: widen words 2h and 2h + 1 of every
// peer (v_cvt_pk_f32_fp8 / _bf8), run the steps on 2-lane f32 vectors (v_pk_add_f32 / v_pk_mul_f32), narrow every
// stored value into words 2h and 2h + 1 of its output (v_cvt_pk_fp8_f32 / _bf8_f32), h = 0, 1. Loads and stores stay
// 16 B, the policy (buffer or global accesses, cache bits) is the plain fused kernels'. The < 16-B tail of a bucket
// goes through the generic one-lane groups (tree_group / scan_group at W = 1). Launched by fused_one (fmi_fused_impl.h)
// at element Acc32<T>, T an 8-bit float: op sum, prod or (the three reduce algorithms) the mean.
#pragma once

#include "fmi_fused_impl.h"

namespace fmi::dev {

struct Fp8Words {
    uint32_t w[4];
};

// POL: buffer accesses through tile descriptors (at: the tile's first byte, lane: the lane's byte offset) or global
// accesses (at: the lane group's first byte).
template <bool POL, int AUX_STORE, class T>
struct Fp8Access {
    size_t at;
    unsigned lane;
    __device__ __forceinline__ Fp8Words load(const void* bucket) const {
        if constexpr (POL)
            return __builtin_bit_cast(Fp8Words, load_tile<kFusedLoadAux, T, 16>(bucket, at, lane));
        else
            return __builtin_bit_cast(Fp8Words, load_lanes<kFusedNT, T, 16>(static_cast<const T*>(bucket) + at));
    }
    __device__ __forceinline__ void store(void* bucket, const Fp8Words& x) const {
        if constexpr (POL)
            store_tile<AUX_STORE, T, 16>(bucket, at, lane, __builtin_bit_cast(Lanes<T, 16>, x));
        else
            store_lanes<kFusedNT, T, 16>(static_cast<T*>(bucket) + at, __builtin_bit_cast(Lanes<T, 16>, x));
    }
};

// The 8 f32 lanes of one half as four 2-lane vectors, each the register pair one packed conversion writes and one
// v_pk_add_f32 / v_pk_mul_f32 reads: combined pair by pair along the element axis, with no move between them.
struct Fp8Half {
    f32x2 p[4];
};

template <class T, int H>
__device__ __forceinline__ Fp8Half fp8_widen_half(const Fp8Words& x) {
    return {{fp8_widen2<T, false>(x.w[2 * H]), fp8_widen2<T, true>(x.w[2 * H]), fp8_widen2<T, false>(x.w[2 * H + 1]),
             fp8_widen2<T, true>(x.w[2 * H + 1])}};
}

template <class T, int H>
__device__ __forceinline__ void fp8_narrow_half(Fp8Words& out, const Fp8Half& v) {
    out.w[2 * H] = fp8_narrow2<T, true>(v.p[1].x, v.p[1].y, fp8_narrow2<T, false>(v.p[0].x, v.p[0].y, 0u));
    out.w[2 * H + 1] = fp8_narrow2<T, true>(v.p[3].x, v.p[3].y, fp8_narrow2<T, false>(v.p[2].x, v.p[2].y, 0u));
}

// A lane group's 16 f32 results, 64 B, with the output's own addressing (tile base and lane offset are 4x the input's):
// the f32 output of the scaled and the MX kernels. POL, group0, lane: as Fp8Access's tile and lane.
template <bool POL>
__device__ __forceinline__ void fp8_store_f32(void* out, size_t group0, unsigned lane, const Fp8Half& lo, const Fp8Half& hi) {
    Lanes<float, 4> q[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        q[k].v[0] = lo.p[2 * k].x, q[k].v[1] = lo.p[2 * k].y, q[k].v[2] = lo.p[2 * k + 1].x, q[k].v[3] = lo.p[2 * k + 1].y;
        q[2 + k].v[0] = hi.p[2 * k].x, q[2 + k].v[1] = hi.p[2 * k].y, q[2 + k].v[2] = hi.p[2 * k + 1].x, q[2 + k].v[3] = hi.p[2 * k + 1].y;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (POL)
            store_tile<kTreeStoreAux, float, 4>(out, group0 * 64, lane * 64u + k * 16u, q[k]);
        else
            store_lanes<kFusedNT, float, 4>(static_cast<float*>(out) + (group0 + lane) * 16 + k * 4, q[k]);
    }
}

template <class Op>
__device__ __forceinline__ Fp8Half fp8_combine_half(const Fp8Half& a, const Fp8Half& b) {
    Fp8Half r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (std::is_same_v<Op, OpSum>)
            r.p[k] = a.p[k] + b.p[k];
        else
            r.p[k] = a.p[k] * b.p[k];
    }
    return r;
}

template <class Op, int ALG, int P, size_t... S>
__device__ __forceinline__ void fp8_run_steps(Fp8Half* v, std::index_sequence<S...>) {
    ((v[P + S] = fp8_combine_half<Op>(v[kStepA<ALG, P, S>], v[kStepB<ALG, P, S>])), ...);
}

// One half of the lanes: every stored output R in [FIRST, FIRST + NOUT) of the program, narrowed into out[R - FIRST].
// OpAvg: the one stored value times r_P = fl32(1 / P) first (one f32 multiply per lane; no instruction fuses it with
// the narrowing).
template <class Op, class T, int ALG, int P, int FIRST, int NOUT, int H>
__device__ __forceinline__ void fp8_acc_half(const Fp8Words* raw, Fp8Words* out) {
    Fp8Half v[P + kNumSteps<ALG, P>];
    [&]<size_t... I>(std::index_sequence<I...>) {
        ((v[I] = fp8_widen_half<T, H>(raw[I])), ...);
    }(std::make_index_sequence<P>{});
    fp8_run_steps<typename StepOp<Op>::type, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    [&]<size_t... R>(std::index_sequence<R...>) {
        if constexpr (is_avg_v<Op>) {
            static_assert(NOUT == 1, "the mean is a reduction result");
            constexpr float r = 1.0f / static_cast<float>(P);
            Fp8Half m = v[kOut<ALG, P, FIRST>];
#pragma unroll
            for (int k = 0; k < 4; ++k) m.p[k] = m.p[k] * r;
            fp8_narrow_half<T, H>(out[0], m);
        } else {
            ((fp8_narrow_half<T, H>(out[R], v[kOut<ALG, P, FIRST + R>])), ...);
        }
    }(std::make_index_sequence<NOUT>{});
}

template <class Op, class T, int ALG, int P, bool SCAN, class A>
__device__ __forceinline__ void fp8_acc_group(const PeerPtrs& ptrs, const A& acc) {
    constexpr int kFirst = SCAN && sched::is_carry_alg(ALG) ? 1 : 0;  // carry programs leave output 0 alone
    constexpr int kOuts = SCAN ? P - kFirst : 1;
    Fp8Words raw[P], out[kOuts];
    [&]<size_t... I>(std::index_sequence<I...>) { ((raw[I] = acc.load(ptrs.in[I])), ...); }(std::make_index_sequence<P>{});
    fp8_acc_half<Op, T, ALG, P, kFirst, kOuts, 0>(raw, out);
    fp8_acc_half<Op, T, ALG, P, kFirst, kOuts, 1>(raw, out);
    [&]<size_t... R>(std::index_sequence<R...>) { ((acc.store(ptrs.out[kFirst + R], out[R])), ...); }(std::make_index_sequence<kOuts>{});
}

// The grid of tree_kernel / scan_kernel (fmi_kernels.h): one thread per 16-B lane group up to kFusedGridCap
// workgroups, striding beyond; workgroup 0 takes the tail.
template <class Op, class T, int ALG, int P, bool SCAN>
__global__ void __launch_bounds__(256) fp8_acc_kernel(PeerPtrs ptrs, size_t n, int pol) {
    constexpr int kStoreAux = SCAN ? kScanStoreAux : kTreeStoreAux;
    const size_t nvec = n / 16;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec)
                fp8_acc_group<Op, T, ALG, P, SCAN>(ptrs, Fp8Access<true, kStoreAux, T>{tile * B * 16, threadIdx.x * 16u});
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            fp8_acc_group<Op, T, ALG, P, SCAN>(ptrs, Fp8Access<false, kStoreAux, T>{g * 16, 0u});
    }
    const size_t first = nvec * 16;
    if (blockIdx.x == 0 && first + threadIdx.x < n) {
        if constexpr (SCAN)
            scan_group<Op, T, ALG, P, 1, float>(ptrs, first + threadIdx.x);
        else
            tree_group<Op, T, ALG, P, false, 1, float>(ptrs, 0, first + threadIdx.x);
    }
}

}  // namespace fmi::dev
