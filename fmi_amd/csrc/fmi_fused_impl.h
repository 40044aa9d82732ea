// fmi_fused_impl.h — the launch recipe and the launch tables of the fused P-way kernels: the definition of fused_unit
// (fmi_internal.h), included by the fmi_fused_*.hip translation units that instantiate it, one unit each.
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

// The kernel of Acc32 over an 8-bit float (fmi_fp8_impl.h, which the units of that element include).
template <class Op, class T, int ALG, int P, bool SCAN>
__global__ void __launch_bounds__(256) fp8_acc_kernel(PeerPtrs ptrs, size_t n, int pol);

// One launch. E: the element as the kernels take it (T, or Acc32<T>: T stored, f32 values); one thread per 16-B lane
// group of the storage type. RANKS (fmi_internal.h) other than kRankZero: an allreduce program on float max / min.
template <class Op, class E, int ALG, int RANKS, int P>
void fused_one(const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    using T = typename Elem<E>::storage;
    constexpr bool kScan = sched::stores_all_outputs(ALG) || RANKS == kRankEvery;
    const size_t nvec = n / kVecLanes<T>;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(grid_for(nvec, kFusedBlock), kFusedGridCap));
    const size_t lds = fused_lds_bytes(P, kFusedBlock * 16);
    const int pol = fused_policy(kScan, P);
    if constexpr (is_fp8_v<T>)
        fp8_acc_kernel<Op, T, ALG, P, kScan><<<grid, kFusedBlock, lds, s>>>(ptrs, n, pol);
    else if constexpr (kScan)
        scan_kernel<Op, E, ALG, P><<<grid, kFusedBlock, lds, s>>>(ptrs, n, pol);
    else
        tree_kernel<Op, E, ALG, P, RANKS == kRankPicked><<<grid, kFusedBlock, lds, s>>>(ptrs, n, rank, pol);
}

template <class Op, class E, int ALG, int RANKS, int LO, int... I>
constexpr std::array<FusedFn, sizeof...(I)> fused_table(std::integer_sequence<int, I...>) {
    return {&fused_one<Op, E, ALG, RANKS, I + LO>...};
}

// Invoke f.template operator()<Op, E>() for the (op, dtype argument) of a call, among those a unit of variant VAR
// instantiates at ALG. launch_fused has checked both, so the refusals here only end the branches no call takes.
template <int VAR, int ALG, class F>
int with_fused_elem(int op, int dtype_arg, F&& f) {
    [[maybe_unused]] auto none = [&]() {
        return fail(FMI_ERR_INVALID, "fused unit: no kernel for op " + std::to_string(op) + ", dtype " + std::to_string(dtype_arg));
    };
    if constexpr (VAR == kFusedAvg) {
        // the SUM program, the stored value scaled by fl(1 / P) before its one store (OpAvg, fmi_kernels.h)
        switch (dtype_arg) {
            case FMI_F32: return f.template operator()<OpAvg, float>();
            case FMI_F64: return f.template operator()<OpAvg, double>();
            case FMI_F16: return f.template operator()<OpAvg, _Float16>();
            case FMI_BF16: return f.template operator()<OpAvg, __bf16>();
            case FMI_F16 | FMI_ACC_F32: return f.template operator()<OpAvg, Acc32<_Float16>>();
            case FMI_BF16 | FMI_ACC_F32: return f.template operator()<OpAvg, Acc32<__bf16>>();
            default: return none();
        }
    } else if constexpr (VAR == kFusedAcc32 || VAR == kFusedFp8Acc32) {
        return with_dtype<VAR == kFusedAcc32 ? kTierHalf : kTierFp8>(storage_dtype(dtype_arg), [&]<class T>() -> int {
            if (op == FMI_OP_SUM) return f.template operator()<OpSum, Acc32<T>>();
            if (op == FMI_OP_PROD) return f.template operator()<OpProd, Acc32<T>>();
            if constexpr (VAR == kFusedFp8Acc32 && !sched::stores_all_outputs(ALG))
                if (op == FMI_OP_AVG) return f.template operator()<OpAvg, Acc32<T>>();
            return none();
        });
    } else {
        constexpr int kTier = VAR == kFusedCore ? kTierCore : VAR == kFusedHalf ? kTierHalf : VAR == kFusedF16 ? kTierF16 : kTierBF16;
        return with_op_dtype<kTier>(op, dtype_arg, [&]<class Op, class T>() -> int { return f.template operator()<Op, T>(); });
    }
}

// RANKS == kRankPicked: the algorithm hands different operand orders to different peers (allreduce); the
// rank-selecting kernel is instantiated only where that can change bits (float max / min), rank 0's elsewhere.
// RANKS == kRankEvery: only there.
template <int ALG, int VAR, int LO, int HI, int RANKS>
int fused_unit(int op, int dtype_arg, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    static_assert(2 <= LO && LO <= HI && HI <= sched::max_fused_peers(ALG), "fused peer range");
    static_assert(RANKS == kRankZero || ALG == sched::kAllreduce, "only an allreduce's value depends on the rank");
    if (P < LO || P > HI)
        return fail(FMI_ERR_INVALID, "fused kernel needs " + std::to_string(LO) + " <= P <= " + std::to_string(HI) +
                                         ", got " + std::to_string(P));
    return with_fused_elem<VAR, ALG>(op, dtype_arg, [&]<class Op, class E>() -> int {
        constexpr bool order_sensitive = is_float_elem_v<E> && (std::is_same_v<Op, OpMax> || std::is_same_v<Op, OpMin>);
        if constexpr (RANKS == kRankEvery && !order_sensitive) {
            return fail(FMI_ERR_INVALID, "all-ranks allreduce kernel: only float max / min depend on the rank");
        } else {
            constexpr int kRanks = order_sensitive ? RANKS : kRankZero;
            static constexpr auto table = fused_table<Op, E, ALG, kRanks, LO>(std::make_integer_sequence<int, HI - LO + 1>{});
            table[P - LO](ptrs, n, kRanks == kRankPicked ? rank : 0, s);
            return check_launch("fused P-way kernel launch");
        }
    });
}

}  // namespace fmi::dev
