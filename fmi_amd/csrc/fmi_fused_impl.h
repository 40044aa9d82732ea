// fmi_fused_impl.h — launch tables for the fused P-way kernels (included by one TU per algorithm).
#pragma once

#include <algorithm>
#include <array>
#include <type_traits>

#include "fmi_internal.h"

namespace fmi::dev {

inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return FMI_OK;
}

constexpr unsigned kFusedBlock = 256;

using FusedFn = void (*)(const PeerPtrs&, size_t, int, hipStream_t);

template <class Op, class T, int ALG, bool ALL_RANKS, int P>
void fused_one(const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    const size_t nvec = n / kVecLanes<T>;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 16);
    if constexpr (sched::stores_all_outputs(ALG))
        scan_kernel<Op, T, ALG, P><<<grid, kFusedBlock, lds, s>>>(ptrs, n, fused_policy(true, P));
    else
        tree_kernel<Op, T, ALG, P, ALL_RANKS><<<grid, kFusedBlock, lds, s>>>(ptrs, n, rank, fused_policy(false, P));
}

template <class Op, class T, int ALG, bool ALL_RANKS, int LO, int... I>
constexpr std::array<FusedFn, sizeof...(I)> fused_table(std::integer_sequence<int, I...>) {
    return {&fused_one<Op, T, ALG, ALL_RANKS, I + LO>...};
}

// RANK_AWARE: the algorithm hands different operand orders to different peers (allreduce); the
// rank-selecting kernel is instantiated only where that can change bits (float max/min).
// [LO, HI]: the peer counts this translation unit instantiates. TIER: the dtypes it instantiates; the core
// tier hands the 16-bit floats to their own translation units (launch_fused_half).
template <int ALG, bool RANK_AWARE, int LO = 2, int HI = sched::kMaxFusedPeers, int TIER = kTierCore>
int launch_fused(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    static_assert(2 <= LO && LO <= HI && HI <= sched::max_fused_peers(ALG), "fused peer range");
    if constexpr (TIER == kTierCore) {
        if (is_fp8_dtype(storage_dtype(dtype))) {
            if (!accumulates_f32(dtype))
                return fail(FMI_ERR_INVALID, "the 8-bit floats have fused kernels only with FMI_ACC_F32");
            return launch_fused_fp8_acc32(ALG, op, storage_dtype(dtype), P, ptrs, n, s);
        }
        if (op == FMI_OP_AVG) return launch_fused_avg(ALG, dtype, P, ptrs, n, s);
        if (accumulates_f32(dtype)) return launch_fused_acc32(ALG, op, dtype, P, ptrs, n, s);
        if (is_half_dtype(dtype)) return launch_fused_half(ALG, RANK_AWARE, op, dtype, P, ptrs, n, rank, s);
    }
    if (P < LO || P > HI)
        return fail(FMI_ERR_INVALID, "fused kernel needs " + std::to_string(LO) + " <= P <= " + std::to_string(HI) +
                                         ", got " + std::to_string(P));
    return with_op_dtype<TIER>(op, dtype, [&]<class Op, class T>() -> int {
        constexpr bool order_sensitive =
            RANK_AWARE && is_float_elem_v<T> && (std::is_same_v<Op, OpMax> || std::is_same_v<Op, OpMin>);
        static constexpr auto table =
            fused_table<Op, T, ALG, order_sensitive, LO>(std::make_integer_sequence<int, HI - LO + 1>{});
        table[P - LO](ptrs, n, order_sensitive ? rank : 0, s);
        return check_launch("fused P-way kernel launch");
    });
}

// FMI_ACC_F32: the same programs on f32 values over 16-bit float storage (the kernels at element Acc32<T>), sum
// and prod, P = 2..16, one family per translation unit (fmi_fused_acc32_*.hip). dtype: the storage dtype.
template <class Op, class T, int ALG, int P>
void fused_acc32_one(const PeerPtrs& ptrs, size_t n, int, hipStream_t s) {
    const size_t nvec = n / kVecLanes<T>;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 16);
    if constexpr (sched::stores_all_outputs(ALG))
        scan_kernel<Op, Acc32<T>, ALG, P><<<grid, kFusedBlock, lds, s>>>(ptrs, n, fused_policy(true, P));
    else
        tree_kernel<Op, Acc32<T>, ALG, P, false><<<grid, kFusedBlock, lds, s>>>(ptrs, n, 0, fused_policy(false, P));
}

template <class Op, class T, int ALG, int... I>
constexpr std::array<FusedFn, sizeof...(I)> fused_acc32_table(std::integer_sequence<int, I...>) {
    return {&fused_acc32_one<Op, T, ALG, I + 2>...};
}

template <int ALG>
int launch_fused_acc32_family(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "fused f32-accumulating kernel needs 2 <= P <= 16, got " + std::to_string(P));
    return with_op_dtype<kTierHalf>(op, dtype, [&]<class Op, class T>() -> int {
        if constexpr (std::is_same_v<Op, OpSum> || std::is_same_v<Op, OpProd>) {
            static constexpr auto table =
                fused_acc32_table<Op, T, ALG>(std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{});
            table[P - 2](ptrs, n, 0, s);
            return check_launch("fused f32-accumulating kernel launch");
        } else {
            return fail(FMI_ERR_INVALID, "f32 accumulation: max / min are selections and run the plain kernels");
        }
    });
}

// FMI_OP_AVG: the tree kernels at op OpAvg (the SUM program, the stored value scaled by fl(1 / P) before its one store),
// P = 2..16, the three reduce algorithms, one per translation unit (fmi_fused_avg_*.hip). E: float, double, _Float16,
// __bf16, or Acc32 of the last two. A sum gives every rank the same bits, so rank 0's expression serves every rank.
template <class E, int ALG, int P>
void fused_avg_one(const PeerPtrs& ptrs, size_t n, int, hipStream_t s) {
    static_assert(!sched::stores_all_outputs(ALG), "the mean is a reduction result");
    const size_t nvec = n / kVecLanes<typename Elem<E>::storage>;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 16);
    tree_kernel<OpAvg, E, ALG, P, false><<<grid, kFusedBlock, lds, s>>>(ptrs, n, 0, fused_policy(false, P));
}

template <class E, int ALG, int... I>
constexpr std::array<FusedFn, sizeof...(I)> fused_avg_table(std::integer_sequence<int, I...>) {
    return {&fused_avg_one<E, ALG, I + 2>...};
}

// dtype: the storage dtype, with FMI_ACC_F32 where the program's values are f32.
template <int ALG>
int launch_fused_avg_family(int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    if (P < 2 || P > sched::kMaxFusedPeers)
        return fail(FMI_ERR_INVALID, "fused mean kernel needs 2 <= P <= 16, got " + std::to_string(P));
    auto launch = [&]<class E>() -> int {
        static constexpr auto table = fused_avg_table<E, ALG>(std::make_integer_sequence<int, sched::kMaxFusedPeers - 1>{});
        table[P - 2](ptrs, n, 0, s);
        return check_launch("fused mean kernel launch");
    };
    switch (dtype) {
        case FMI_F32: return launch.template operator()<float>();
        case FMI_F64: return launch.template operator()<double>();
        case FMI_F16: return launch.template operator()<_Float16>();
        case FMI_BF16: return launch.template operator()<__bf16>();
        case FMI_F16 | FMI_ACC_F32: return launch.template operator()<Acc32<_Float16>>();
        case FMI_BF16 | FMI_ACC_F32: return launch.template operator()<Acc32<__bf16>>();
        default: return fail(FMI_ERR_INVALID, "FMI_OP_AVG: dtype " + std::to_string(dtype) + " is not a float dtype");
    }
}

}  // namespace fmi::dev
