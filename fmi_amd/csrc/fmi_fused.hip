// fmi_fused.hip — the one entry of every fused P-way launch, and the one place that knows the translation units that
// hold the kernels. Host code only: this file sees fused_unit's declaration (fmi_internal.h), never its definition
// (fmi_fused_impl.h), so it instantiates no kernel, and a unit named here that no fmi_fused_*.hip instantiates is an
// undefined symbol when the library is linked, not FMI_ERR_INVALID on a GPU. The partition (which file holds what):
//   core (f32 f64 i32 i64)   fmi_fused_allreduce.hip (P <= 16, and every rank's values), _allreduce_wide.hip (17..31 and
//                            the 32-input pre-fold block), _reduce.hip (reduce, reduce_ltr, partials), _scan.hip (the two
//                            scans and their carry blocks), _scan_wide.hip (17..31)
//   16-bit floats            fmi_fused_half_*.hip: the same programs, one family and peer range per unit, the wide
//                            allreduce one dtype per unit
//   FMI_ACC_F32, 16-bit      fmi_fused_acc32_*.hip, one per algorithm
//   FMI_ACC_F32, 8-bit       fmi_fused_fp8_acc32_*.hip, one per algorithm (sum, prod and the mean)
//   FMI_OP_AVG               fmi_fused_avg_*.hip, one per reduce algorithm (f32 f64 f16 bf16, the last two with f32 values too)
//   scaled 8-bit sums        fmi_fused_fp8_scaled_*.hip, one per reduce algorithm (fmi_dev_reduce_tree_scaled: both 8-bit
//                            floats, 8-bit and f32 output; their own entry, launch_fused_scaled below)
//   MX 8-bit sums and means  fmi_fused_mx_*.hip, one per reduce algorithm (fmi_dev_reduce_tree_mx: both 8-bit floats, 8-bit
//                            and f32 output; their own entry, launch_fused_mx below)
//   MXFP4 sums and means     fmi_fused_mxfp4_*.hip, one per reduce algorithm (the same call at FMI_F4E2M1: E2M1 and f32
//                            output; launch_fused_mx too)
//   stochastic rounding      fmi_fused_mx_sr_*.hip and fmi_fused_mxfp4_sr_*.hip, one per reduce algorithm
//                            (fmi_dev_reduce_tree_mx_sr: the same kernels' SR instantiations, the element type's output
//                            rounded by narrow_sr; launch_fused_mx with a seed)
// Everything else a call can be runs elsewhere (fmi_dev.hip): P beyond a variant's kernels and unaligned buckets as
// blocks of fused programs, as widen / the f32 program / narrow, as the SUM program and the scale kernel
// (fmi_scale.hip), or as pairwise passes in the program's order.
#include "fmi_internal.h"

namespace fmi::dev {
namespace {

constexpr int kHi = sched::kMaxFusedPeers;  // the narrow units hold P = 2..16, the wide ones 17..31

template <int ALG, int VAR, int LO, int HI, int RANKS = kRankZero>
FusedUnit* unit_if(int P) {
    return P >= LO && P <= HI ? &fused_unit<ALG, VAR, LO, HI, RANKS> : nullptr;
}

// The plain variants, any op. WIDE: the variant of the allreduce's P = 17..31 units. picked: the rank-selecting allreduce.
template <int VAR, int WIDE>
FusedUnit* plain_unit(int alg, int P, bool picked) {
    const bool wide = P > kHi;
    switch (alg) {
        case sched::kAllreduce:
            if (wide) return unit_if<sched::kAllreduce, WIDE, kHi + 1, sched::kMaxFusedAllreducePeers, kRankPicked>(P);
            return picked ? unit_if<sched::kAllreduce, VAR, 2, kHi, kRankPicked>(P) : unit_if<sched::kAllreduce, VAR, 2, kHi>(P);
        case sched::kAllreducePrefold16: return unit_if<sched::kAllreducePrefold16, VAR, 32, 32>(P);
        case sched::kReduce: return unit_if<sched::kReduce, VAR, 2, kHi>(P);
        case sched::kReduceLtr: return unit_if<sched::kReduceLtr, VAR, 2, kHi>(P);
        case sched::kReducePartials: return unit_if<sched::kReducePartials, VAR, 2, kHi>(P);
        case sched::kScan:
            return wide ? unit_if<sched::kScan, VAR, kHi + 1, sched::kMaxFusedScanPeers>(P) : unit_if<sched::kScan, VAR, 2, kHi>(P);
        case sched::kScanLtr:
            return wide ? unit_if<sched::kScanLtr, VAR, kHi + 1, sched::kMaxFusedScanPeers>(P) : unit_if<sched::kScanLtr, VAR, 2, kHi>(P);
        case sched::kScanCarry: return unit_if<sched::kScanCarry, VAR, 2, kHi>(P);
        case sched::kScanLtrCarry: return unit_if<sched::kScanLtrCarry, VAR, 2, kHi>(P);
        default: return nullptr;
    }
}

// The variants with f32 values and the mean, P = 2..16: sum, prod (max / min are selections and run the plain kernels)
// and, at the three algorithms whose output is a reduction result, the mean. Rank 0's expression: a sum's or a
// product's bits are every rank's.
template <int VAR>
FusedUnit* value_unit(int alg, int op, int P) {
    const bool mean = op == FMI_OP_AVG;  // all a kFusedAvg call can be
    if (!mean && op != FMI_OP_SUM && op != FMI_OP_PROD) return nullptr;
    switch (alg) {
        case sched::kAllreduce: return unit_if<sched::kAllreduce, VAR, 2, kHi>(P);
        case sched::kReduce: return unit_if<sched::kReduce, VAR, 2, kHi>(P);
        case sched::kReduceLtr: return unit_if<sched::kReduceLtr, VAR, 2, kHi>(P);
        default: break;
    }
    if constexpr (VAR != kFusedAvg) {
        if (!mean) switch (alg) {
            case sched::kReducePartials: return unit_if<sched::kReducePartials, VAR, 2, kHi>(P);
            case sched::kScan: return unit_if<sched::kScan, VAR, 2, kHi>(P);
            case sched::kScanLtr: return unit_if<sched::kScanLtr, VAR, 2, kHi>(P);
            default: break;
        }
    }
    return nullptr;
}

// The unit that holds a call's kernels, nullptr if there is none.
FusedUnit* find_unit(int alg, int op, int dtype_arg, int P, bool picked) {
    switch (fused_variant(op, dtype_arg)) {
        case kFusedCore: return plain_unit<kFusedCore, kFusedCore>(alg, P, picked);
        case kFusedHalf:
            return storage_dtype(dtype_arg) == FMI_F16 ? plain_unit<kFusedHalf, kFusedF16>(alg, P, picked)
                                                       : plain_unit<kFusedHalf, kFusedBF16>(alg, P, picked);
        case kFusedAcc32: return value_unit<kFusedAcc32>(alg, op, P);
        case kFusedFp8Acc32: return value_unit<kFusedFp8Acc32>(alg, op, P);
        case kFusedAvg: return value_unit<kFusedAvg>(alg, op, P);
        default: return nullptr;
    }
}

}  // namespace

bool fused_has_unit(int alg, int op, int dtype_arg, int P) { return find_unit(alg, op, dtype_arg, P, false) != nullptr; }

int launch_fused(int alg, int op, int dtype_arg, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s) {
    // allreduce: the rank-selecting kernel has to evaluate every peer's value, so it runs only where no relabelling
    // of the peers makes rank 0's expression the rank's own
    bool picked = alg == sched::kAllreduce;
    PeerPtrs perm = ptrs;
    if (alg == sched::kAllreduce && P <= kHi && (P & (P - 1)) == 0 && rank > 0 && rank < P) {
        // For P = 2^k, recursive doubling is symmetric under relabelling peers p -> p ^ rank: the value
        // peer `rank` ends with is rank 0's expression over inputs x[p ^ rank] (every operand order
        // included; checked against the schedule in tests/test_abi.py). So the rank-0 kernel over
        // permuted pointers replaces the rank-selecting one.
        for (int p = 0; p < P; ++p) perm.in[p] = ptrs.in[p ^ rank];
        picked = false;
    } else if (alg == sched::kAllreducePrefold16) {
        // the block's 16-peer recursive doubling likewise; each peer's partner moves with it
        for (int j = 0; j < 16; ++j) {
            perm.in[j] = ptrs.in[j ^ (rank & 15)];
            perm.in[16 + j] = ptrs.in[16 + (j ^ (rank & 15))];
        }
    }
    if (FusedUnit* unit = find_unit(alg, op, dtype_arg, P, picked)) return unit(op, dtype_arg, P, perm, n, rank, s);
    const int var = fused_variant(op, dtype_arg);
    const char* why = var == kFusedNone && is_fp8_dtype(storage_dtype(dtype_arg)) ? "the 8-bit floats have fused kernels only with FMI_ACC_F32"
                      : var == kFusedNone                                         ? "no fused kernel for this op and dtype"
                      : accumulates_f32(dtype_arg) && (op == FMI_OP_MAX || op == FMI_OP_MIN)
                          ? "f32 accumulation: max / min are selections and run the plain kernels"
                      : op == FMI_OP_AVG && sched::stores_all_outputs(alg) ? "FMI_OP_AVG: only a reduction result has a mean"
                                                                           : "no kernel for this algorithm and P";
    return fail(FMI_ERR_INVALID, "fused launch (algorithm " + std::to_string(alg) + ", op " + std::to_string(op) + ", dtype " +
                                     std::to_string(dtype_arg) + ", P = " + std::to_string(P) + "): " + why);
}

int launch_fused_scaled(int alg, int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const ScaledArgs& sc, size_t n, hipStream_t s) {
    // a sum's bits are every rank's, so no allreduce call needs a permutation or a rank
    switch (alg) {
        case sched::kAllreduce: return scaled_unit<sched::kAllreduce>(dtype, out_dtype, P, ptrs, sc, n, s);
        case sched::kReduce: return scaled_unit<sched::kReduce>(dtype, out_dtype, P, ptrs, sc, n, s);
        case sched::kReduceLtr: return scaled_unit<sched::kReduceLtr>(dtype, out_dtype, P, ptrs, sc, n, s);
        default: return fail(FMI_ERR_INVALID, "fused scaled launch: no kernel for algorithm " + std::to_string(alg));
    }
}

// The unit of one algorithm's six MX families: fmi_fused_mx_*.hip, _mx_sr_, _mxfp4_, _mxfp4_sr_, _mxfp6_, _mxfp6_sr_.
// bits: the element's width, 8, 4 or 6.
template <int ALG>
MxUnit* mx_family(int bits, bool sr) {
    if (bits == 4) return sr ? &mxfp4_unit<ALG, true> : &mxfp4_unit<ALG, false>;
    if (bits == 6) return sr ? &mxfp6_unit<ALG, true> : &mxfp6_unit<ALG, false>;
    return sr ? &mx_unit<ALG, true> : &mx_unit<ALG, false>;
}

int launch_fused_mx(int alg, int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s) {
    const int bits = dtype == FMI_F4E2M1 ? 4 : is_fp6_dtype(dtype) ? 6 : 8;
    const bool sr = mx.seed != nullptr;
    if (sr && out_dtype != dtype) return fail(FMI_ERR_INVALID, "fused MX stochastic-rounding launch: the output is the element type's");
    switch (alg) {
        case sched::kAllreduce: return mx_family<sched::kAllreduce>(bits, sr)(dtype, out_dtype, P, ptrs, mx, n, s);
        case sched::kReduce: return mx_family<sched::kReduce>(bits, sr)(dtype, out_dtype, P, ptrs, mx, n, s);
        case sched::kReduceLtr: return mx_family<sched::kReduceLtr>(bits, sr)(dtype, out_dtype, P, ptrs, mx, n, s);
        default:
            return fail(FMI_ERR_INVALID, std::string("fused ") + (sr ? "MX stochastic-rounding" : bits == 4 ? "MXFP4" : bits == 6 ? "MXFP6" : "MX") +
                                             " launch: no kernel for algorithm " + std::to_string(alg));
    }
}

int launch_fused_all_ranks(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s) {
    if (is_half_dtype(dtype)) return fused_unit<sched::kAllreduce, kFusedHalf, 2, kHi, kRankEvery>(op, dtype, P, ptrs, n, 0, s);
    return fused_unit<sched::kAllreduce, kFusedCore, 2, kHi, kRankEvery>(op, dtype, P, ptrs, n, 0, s);
}

}  // namespace fmi::dev
