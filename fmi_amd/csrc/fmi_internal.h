// fmi_internal.h — declarations shared by the translation units of libfmi_dev.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <exception>
#include <new>
#include <string>

#include "../../include/fmi_dev.h"
#include "fmi_kernels.h"

namespace fmi::dev {

// Records a failure message for fmi_last_error() and returns `code`.
int fail(int code, const std::string& msg);

// Runs a C-ABI entry point's body: no C++ exception may cross the extern "C" boundary (it would call
// std::terminate in the caller). std::bad_alloc (e.g. a host program or expression for millions of peers)
// becomes FMI_ERR_ALLOC, anything else FMI_ERR_INVALID, with the message for fmi_last_error().
template <class F>
int guarded(const char* what, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(FMI_ERR_ALLOC, std::string(what) + ": out of host memory");
    } catch (const std::exception& e) {
        return fail(FMI_ERR_INVALID, std::string(what) + ": " + e.what());
    } catch (...) {
        return fail(FMI_ERR_INVALID, std::string(what) + ": unknown exception");
    }
}

// The library's default stream (what a NULL fmi_stream_t means); nullptr before fmi_dev_init.
hipStream_t library_stream();

// Dynamic LDS a fused P-way launch reserves (the kernels use none) so that the peer loads its resident
// workgroups keep in flight per CU stay within FMI_TUNE_FUSED_INFLIGHT_KIB: fewer concurrent HBM streams
// at large P, better DRAM row locality. `wg_load_bytes_per_peer` = bytes one workgroup loads per peer.
size_t fused_lds_bytes(int P, size_t wg_load_bytes_per_peer);
int fused_policy(bool scan, int P);  // FMI_TUNE_FUSED_POLICY: the fused kernels' `pol` argument

// The dtypes every kernel is instantiated for (the fused P-way kernels included).
inline bool is_core_dtype(int dtype) { return dtype >= FMI_F32 && dtype <= FMI_I64; }
// The 16-bit float dtypes: the pairwise family and every fused / one-pass family, each instantiated in the
// fmi_fused_half_*.hip translation units.
inline bool is_half_dtype(int dtype) { return dtype == FMI_F16 || dtype == FMI_BF16; }
// The 8-bit float dtypes: the pairwise family, and with FMI_ACC_F32 the fused kernels of fmi_fused_fp8_acc32_*.hip.
// Their plain P-way programs have no fused kernel (out of scope on purpose): they run as pairwise passes in order.
inline bool is_fp8_dtype(int dtype) { return dtype == FMI_F8E4M3 || dtype == FMI_F8E5M2; }
// The element types an MX bucket can have: the two 8-bit floats and FMI_F4E2M1, which is valid in the MX calls ALONE
// (two elements to a byte: mx_elem_bytes). Every other entry point refuses it on the host, naming it (refuse_fp4).
// The same holds for the two 6-bit floats FMI_F6E2M3 and FMI_F6E3M2 (MXFP6: four elements to three bytes).
inline bool is_fp6_dtype(int dtype) { return dtype == FMI_F6E2M3 || dtype == FMI_F6E3M2; }
inline bool is_mx_dtype(int dtype) { return is_fp8_dtype(dtype) || dtype == FMI_F4E2M1 || is_fp6_dtype(dtype); }
inline size_t mx_elem_bytes(int dtype, size_t n) {
    if (is_fp6_dtype(dtype)) return n / 4 * 3 + (n % 4 * 3 + 3) / 4;  // ceil(3 n / 4) without the overflow of 3 n
    return dtype == FMI_F4E2M1 ? n / 2 + n % 2 : n;
}
// refuse_fp4: the sub-byte element types, FMI_F4E2M1 and the two 6-bit floats.
inline int refuse_fp4(int dtype_arg) {
    const int st = dtype_arg & ~FMI_ACC_F32;  // with or without the flag
    if (is_fp6_dtype(st))
        return fail(FMI_ERR_INVALID, "dtype " + std::to_string(dtype_arg) + (st == FMI_F6E2M3 ? " (FMI_F6E2M3)" : " (FMI_F6E3M2)") +
                                     " is valid only as the element type of the MX calls (fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize, "
                                     "fmi_dev_mx_dequantize, fmi_comm_allreduce_mx): 6-bit elements have no other kernel");
    if (st != FMI_F4E2M1) return FMI_OK;
    return fail(FMI_ERR_INVALID, "dtype " + std::to_string(dtype_arg) + " (FMI_F4E2M1) is valid only as the element type of "
                                 "the MX calls (fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize, fmi_dev_mx_dequantize, "
                                 "fmi_comm_allreduce_mx): 4-bit elements have no other kernel");
}

// The dtype ARGUMENT of a P-way call may carry FMI_ACC_F32 (include/fmi_dev.h): its storage dtype, which sizes,
// alignment, order_sensitive, fused_covers and with_dtype take, and whether the program's values are kept in f32.
inline int storage_dtype(int dtype_arg) { return dtype_arg & ~FMI_ACC_F32; }
inline bool accumulates_f32(int dtype_arg) { return (dtype_arg & FMI_ACC_F32) != 0; }
// What every entry point does with its dtype argument, once: the flag is valid on the 16-bit and 8-bit float dtypes alone
// (FMI_ERR_INVALID naming the dtype otherwise), and it is dropped where it cannot change a bit: max / min are
// selections, and a pairwise call (pway = false) or a single peer makes no second rounding. *canon: the storage
// dtype, with the flag where the call accumulates in f32. An unknown storage dtype is left to the caller's own check.
inline int canonical_dtype(int op, int dtype_arg, bool pway, int P, int* canon) {
    *canon = storage_dtype(dtype_arg);
    if (int rc = refuse_fp4(dtype_arg)) return rc;
    if (!accumulates_f32(dtype_arg)) return FMI_OK;
    if (!is_half_dtype(*canon) && !is_fp8_dtype(*canon))
        return fail(FMI_ERR_INVALID, "dtype " + std::to_string(dtype_arg) + ": FMI_ACC_F32 is valid only as FMI_F16 | FMI_ACC_F32, "
                                     "FMI_BF16 | FMI_ACC_F32, FMI_F8E4M3 | FMI_ACC_F32 or FMI_F8E5M2 | FMI_ACC_F32");
    if (pway && P != 1 && (op == FMI_OP_SUM || op == FMI_OP_PROD || op == FMI_OP_AVG)) *canon |= FMI_ACC_F32;
    return FMI_OK;
}

// FMI_OP_AVG (include/fmi_dev.h) is valid only where a call produces a reduction result over float buckets. The entry
// points that cannot take it refuse it first of all, before any other check and before a device is needed:
// `who` names the entry point, `why` the reason.
inline int refuse_avg(int op, const char* who, const char* why) {
    if (op != FMI_OP_AVG) return FMI_OK;
    return fail(FMI_ERR_INVALID, std::string(who) + ": op " + std::to_string(op) + " (FMI_OP_AVG) is not valid here: " + why);
}

// The variants of a fused P-way launch: which elements and ops a call's kernels are instantiated for. Every translation
// unit of fused kernels holds one variant of one algorithm over one peer range (fused_unit below).
enum FusedVariant : int {
    kFusedNone = -1,  // no fused kernel: pairwise passes in the program's order (run_program_stepwise)
    kFusedCore,       // f32 f64 i32 i64, the four ops
    kFusedHalf,       // f16 bf16, the four ops
    kFusedF16,        // one of the two: the largest half programs (allreduce, P = 17..31) build one dtype per
    kFusedBF16,       // translation unit
    kFusedAcc32,      // FMI_ACC_F32 over f16 / bf16 (element Acc32<T>): sum, prod
    kFusedFp8Acc32,   // FMI_ACC_F32 over the 8-bit floats (fp8_acc_kernel): sum, prod and, on a reduction result, the mean
    kFusedAvg,        // FMI_OP_AVG over f32 f64 f16 bf16 and Acc32 of the last two
};
// The variant of a call. op: an fmi_op_t; dtype_arg: in canonical form (canonical_dtype). The 8-bit floats are fused
// only with the flag (their plain P-way programs are out of scope on purpose); the 8/16-bit and unsigned integers never.
inline int fused_variant(int op, int dtype_arg) {
    const int st = storage_dtype(dtype_arg);
    if (is_fp8_dtype(st)) return accumulates_f32(dtype_arg) ? kFusedFp8Acc32 : kFusedNone;
    if (op == FMI_OP_AVG) return st == FMI_F32 || st == FMI_F64 || is_half_dtype(st) ? kFusedAvg : kFusedNone;
    if (accumulates_f32(dtype_arg)) return is_half_dtype(st) ? kFusedAcc32 : kFusedNone;
    return is_half_dtype(st) ? kFusedHalf : is_core_dtype(st) ? kFusedCore : kFusedNone;
}
// Whether launch_fused (below) has a unit for the call (fmi_fused.hip, from the one table of units it dispatches on).
// alg: a sched::Alg (the C-ABI's fmi_alg_t values are its first five).
bool fused_has_unit(int alg, int op, int dtype_arg, int P);
// Which (op, dtype argument, algorithm, P) have a single-pass kernel: a fused unit, or for the plain variants at any
// P beyond theirs a program built from fused blocks (the callers send P > 16 and unaligned buckets of the other
// variants to their fallbacks first). No (op, algorithm, P) of the 16-bit floats is held back: none of their
// kernels needs scratch memory.
inline bool fused_covers(int op, int dtype_arg, int alg, int P) {
    const int var = fused_variant(op, dtype_arg);
    return var == kFusedCore || var == kFusedHalf || fused_has_unit(alg, op, dtype_arg, P);
}

// Dispatch tiers of with_dtype. The fused launch tables are built per tier: the core tier in the translation
// units that always held them, the half tier in fmi_fused_half_*.hip, so core + half is what a plain fused
// launch serves and ALL what the pairwise family serves.
inline constexpr int kTierCore = 0;  // f32 f64 i32 i64
inline constexpr int kTierAll = 1;   // every fmi_dtype_t
inline constexpr int kTierHalf = 2;  // f16 bf16 alone
inline constexpr int kTierF16 = 3;   // one of the two: the largest half-tier programs build one dtype per
inline constexpr int kTierBF16 = 4;  // translation unit
inline constexpr int kTierFp8 = 5;   // the two 8-bit floats alone (fmi_fused_fp8_acc32_*.hip, the conversions)

// Invoke f.template operator()<T>() for a runtime dtype of the tier; returns FMI_ERR_INVALID if it is not in it.
template <int TIER, class F>
int with_dtype(int dtype, F&& f) {
    if constexpr (TIER == kTierCore || TIER == kTierAll) {
        switch (dtype) {
            case FMI_F32: return f.template operator()<float>();
            case FMI_F64: return f.template operator()<double>();
            case FMI_I32: return f.template operator()<int32_t>();
            case FMI_I64: return f.template operator()<int64_t>();
            default: break;
        }
    }
    if constexpr (TIER == kTierAll || TIER == kTierHalf || TIER == kTierF16)
        if (dtype == FMI_F16) return f.template operator()<_Float16>();
    if constexpr (TIER == kTierAll || TIER == kTierHalf || TIER == kTierBF16)
        if (dtype == FMI_BF16) return f.template operator()<__bf16>();
    if constexpr (TIER == kTierAll || TIER == kTierFp8) {
        if (dtype == FMI_F8E4M3) return f.template operator()<f8e4m3>();
        if (dtype == FMI_F8E5M2) return f.template operator()<f8e5m2>();
    }
    if constexpr (TIER == kTierAll) {
        switch (dtype) {
            case FMI_U32: return f.template operator()<uint32_t>();
            case FMI_U64: return f.template operator()<uint64_t>();
            case FMI_I8: return f.template operator()<int8_t>();
            case FMI_U8: return f.template operator()<uint8_t>();
            case FMI_I16: return f.template operator()<int16_t>();
            case FMI_U16: return f.template operator()<uint16_t>();
            default: break;
        }
    }
    if (int rc = refuse_fp4(dtype)) return rc;
    return fail(FMI_ERR_INVALID, "unknown dtype " + std::to_string(dtype));
}

// Invoke f.template operator()<Op, T>() for a runtime (op, dtype); returns FMI_ERR_INVALID if unknown.
template <int TIER = kTierAll, class F>
int with_op_dtype(int op, int dtype, F&& f) {
    auto by_dtype = [&]<class Op>() -> int {
        return with_dtype<TIER>(dtype, [&]<class T>() -> int { return f.template operator()<Op, T>(); });
    };
    switch (op) {
        case FMI_OP_SUM: return by_dtype.template operator()<OpSum>();
        case FMI_OP_PROD: return by_dtype.template operator()<OpProd>();
        case FMI_OP_MAX: return by_dtype.template operator()<OpMax>();
        case FMI_OP_MIN: return by_dtype.template operator()<OpMin>();
        default: return fail(FMI_ERR_INVALID, "unknown op " + std::to_string(op));
    }
}

inline size_t dtype_size(int dtype) {
    switch (dtype) {
        case FMI_F32: case FMI_I32: case FMI_U32: return 4;
        case FMI_F64: case FMI_I64: case FMI_U64: return 8;
        case FMI_I8: case FMI_U8: case FMI_F8E4M3: case FMI_F8E5M2: return 1;
        case FMI_I16: case FMI_U16: case FMI_F16: case FMI_BF16: return 2;
        default: return 0;
    }
}

inline bool is_float(int dtype) { return dtype == FMI_F32 || dtype == FMI_F64 || is_half_dtype(dtype) || is_fp8_dtype(dtype); }

// Every fused single-pass launch (fmi_fused.hip; all pointers 16-B aligned): classifies the call (fused_variant),
// checks op and P against the variant's kernels at `alg`, applies the allreduce's host-side pointer permutations and
// calls the one translation unit that holds the instantiations. Returns 0 or a negative fmi_status_t.
// alg: a sched::Alg. op: an fmi_op_t, FMI_OP_AVG included. dtype_arg: in canonical form. rank: the allreduces' alone.
//   kAllreduce (P <= 31), kReduce, kReduceLtr: ptrs.out[0] = the result (of peer `rank`);
//   kAllreducePrefold16 (P = 32): a 16-peer allreduce block whose peers all pre-fold a partner: in[0..16) the block,
//     in[16..32) the partners; out[0] = the value of block peer `rank` (< 16);
//   kReducePartials: reduce_no_order with every (transformed) peer's final sendbuf stored, ptrs.out[t] for t < P;
//   kScan, kScanLtr (P <= 31): ptrs.out[p] for p < P;
//   kScanCarry, kScanLtrCarry: blocks of a scan beyond 16 peers, ptrs.in[0] is the carry, out[0] unused.
int launch_fused(int alg, int op, int dtype_arg, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s);
// allreduce_no_order's value for every peer at once (outs[r] for r < P <= 16), float max / min only
int launch_fused_all_ranks(int op, int dtype, int P, const PeerPtrs& ptrs, size_t n, hipStream_t s);
// float max / min: which operand is kept on a tie (±0) or a NaN depends on the order, so every peer of an
// allreduce can end with different bits
inline bool order_sensitive(int op, int dtype) { return is_float(dtype) && (op == FMI_OP_MAX || op == FMI_OP_MIN); }
// Whose value the launch of an allreduce program stores.
inline constexpr int kRankZero = 0;    // rank 0's expression: every rank's where no rank changes the bits, or the caller permuted the pointers
inline constexpr int kRankPicked = 1;  // the `rank` argument's: the rank-selecting kernel where the rank can change bits (float max / min)
inline constexpr int kRankEvery = 2;   // every rank's, out[r] for r < P: the scan kernel over the program, float max / min only
// One translation unit's fused kernels: algorithm ALG, variant VAR (a FusedVariant), P in [LO, HI]. Declared here for
// the dispatcher, defined in fmi_fused_impl.h and explicitly instantiated by exactly one fmi_fused_*.hip each (so the
// ~3,800 instantiations build in parallel), which makes a unit that launch_fused names but no file builds an
// undefined symbol when the library is linked. Arguments as launch_fused's, already checked by it.
using FusedUnit = int(int op, int dtype_arg, int P, const PeerPtrs& ptrs, size_t n, int rank, hipStream_t s);
template <int ALG, int VAR, int LO, int HI, int RANKS = kRankZero>
FusedUnit fused_unit;
// fmi_dev_reduce_tree_scaled (include/fmi_dev.h): the scaled sum of 8-bit float buckets. What its kernels take beside
// the peer pointers, every pointer device memory: in_scales[P] in the CALLER's peer order (the kernel reads input slot
// t's scale at (t + rot) % P: rot = the root of a kReduce call, whose pointers the caller rotated, 0 otherwise),
// out_scale and amax one f32 each, either may be nullptr.
struct ScaledArgs {
    const float* in_scales;
    const float* out_scale;
    float* amax;
    int rot;
};
// The fused scaled kernels (fmi_fused.hip -> fmi_fused_fp8_scaled_*.hip): 2 <= P <= 16, all pointers 16-B aligned.
// alg: kAllreduce, kReduce or kReduceLtr; dtype: FMI_F8E4M3 / FMI_F8E5M2; out_dtype: dtype or FMI_F32; ptrs.in[t] the
// (transformed) inputs, ptrs.out[0] the result.
int launch_fused_scaled(int alg, int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const ScaledArgs& sc, size_t n, hipStream_t s);
// One translation unit's scaled kernels (algorithm ALG, P = 2..16, both dtypes, both outputs): declared here for the
// dispatcher, defined in fmi_fp8_scaled_impl.h, instantiated by one fmi_fused_fp8_scaled_*.hip each.
using ScaledUnit = int(int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const ScaledArgs& sc, size_t n, hipStream_t s);
template <int ALG>
ScaledUnit scaled_unit;
// The scaled call's other kernels (fmi_fp8_scaled.hip), any alignment. dtype / out_dtype as above.
//   widen_scale: dst[i] = fl32(widen(src[i]) * *scale)
//   finish:      amax (if given) folded with max bits(|S[i]|); out[i] = narrow(fl32(S[i] * t)) or fl32(S[i] * t)
//   amax_fold:   *amax = umax(bits(*amax), words[0..count))
int launch_widen_scale_f32(int dtype, float* dst, const void* src, const float* scale, size_t n, hipStream_t s);
int launch_scaled_finish(int dtype, int out_dtype, void* out, const float* S, const float* out_scale, float* amax, size_t n,
                         hipStream_t s);
int launch_amax_fold(float* amax, const uint32_t* words, int count, hipStream_t s);
// The host-side checks of fmi_dev_reduce_tree_scaled's op, dtype argument, alg and out_dtype (fmi_dev.hip), shared with
// fmi_comm_allreduce_scaled; *dtype: the storage dtype. And the call after its validation: the comm call's shard step.
int scaled_check_args(const char* who, int op, int dtype_arg, int alg, int out_dtype, int* dtype);
int reduce_tree_scaled(int dtype, int alg, int out_dtype, void* out, const void* const* ins, const float* in_scales,
                       const float* out_scale, float* amax, int P, int rank, size_t n, hipStream_t s);
// fmi_dev_reduce_tree_mx (include/fmi_dev.h): the sum or mean of block-scaled (MX) 8-bit float buckets. What its fused
// kernels take beside the peer pointers, the kernel argument's 2 P + 2 pointers in all: in_scales[t] the E8M0 scale
// bytes of ptrs.in[t] (a kReduce call's caller rotates them with the inputs), out_scales the result's (unused with an
// f32 output), r the mean's factor fl32(1 / P), or 1.0f for a sum. seed / first: the stochastic-rounding calls alone
// (fmi_dev_reduce_tree_mx_sr): the device word that holds the Philox key and the stream position of element 0, a
// multiple of 32; seed == nullptr is a round-to-nearest call, whose kernels read neither.
struct MxArgs {
    const uint8_t* in_scales[sched::kMaxFusedPeers];
    uint8_t* out_scales;
    float r;
    const uint64_t* seed;
    uint64_t first;
};
// The fused MX kernels (fmi_fused.hip -> fmi_fused_mx_*.hip): 2 <= P <= 16, the element buckets 16-B aligned, the
// scale arrays of any alignment. alg, dtype, out_dtype, ptrs as launch_fused_scaled's.
int launch_fused_mx(int alg, int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s);
// One translation unit's MX kernels: algorithm ALG, P = 2..16, one of four families, the element format by the
// template's name and the rounding by SR.
//   mx_unit<ALG, false>      both 8-bit floats, 8-bit and f32 output    fmi_mx_impl.h, one fmi_fused_mx_*.hip each
//   mx_unit<ALG, true>       both 8-bit floats, stochastic rounding     fmi_mx_impl.h, one fmi_fused_mx_sr_*.hip each
//   mxfp4_unit<ALG, false>   FMI_F4E2M1, E2M1 and f32 output            fmi_mxfp4_impl.h, one fmi_fused_mxfp4_*.hip each
//   mxfp4_unit<ALG, true>    FMI_F4E2M1, stochastic rounding            fmi_mxfp4_impl.h, one fmi_fused_mxfp4_sr_*.hip each
//   mxfp6_unit<ALG, false>   FMI_F6E2M3 / FMI_F6E3M2, FP6 and f32 output fmi_mxfp6_impl.h, one fmi_fused_mxfp6_*.hip each
//   mxfp6_unit<ALG, true>    FMI_F6E2M3 / FMI_F6E3M2, stochastic rounding fmi_mxfp6_impl.h, one fmi_fused_mxfp6_sr_*.hip each
// A stochastic-rounding unit (mx.seed != nullptr) holds the element type's own output only: out_dtype == dtype.
// n counts elements (FMI_F4E2M1: two to a byte; the 6-bit floats: four to three bytes).
using MxUnit = int(int dtype, int out_dtype, int P, const PeerPtrs& ptrs, const MxArgs& mx, size_t n, hipStream_t s);
template <int ALG, bool SR>
MxUnit mx_unit;
template <int ALG, bool SR>
MxUnit mxfp4_unit;
template <int ALG, bool SR>
MxUnit mxfp6_unit;
// fmi_dev_mx_dequantize / fmi_dev_mx_quantize (fmi_mx.hip), any alignment, one launch each. dtype: FMI_F8E4M3,
// FMI_F8E5M2, FMI_F4E2M1 (packed: n elements in ceil(n / 2) bytes) or FMI_F6E2M3 / FMI_F6E3M2 (packed: ceil(3 n / 4)
// bytes); dst_dtype / src_dtype: FMI_F32, FMI_F16 or FMI_BF16 (FMI_ERR_INVALID otherwise).
int launch_mx_dequantize(int dst_dtype, void* dst, int dtype, const void* src, const uint8_t* scales, size_t n, hipStream_t s);
int launch_mx_quantize(int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, hipStream_t s);
// fmi_dev_mx_quantize_sr (fmi_mx.hip too): launch_mx_quantize with narrow_sr (fmi_mx_sr.h); seed one u64 in device memory, first the
// stream position of element 0 (a multiple of 32).
int launch_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, int src_dtype, const void* src, size_t n, const uint64_t* seed,
                          uint64_t first, hipStream_t s);
// fmi_host_mx_quantize_sr after its checks (fmi_mx_sr.hip): the same quantization on host memory, from the same functions.
int host_mx_quantize_sr(int dtype, void* out, uint8_t* out_scales, const float* src, size_t n, uint64_t seed, uint64_t first);
// The host-side checks of fmi_dev_reduce_tree_mx's op, dtype argument, alg, out_dtype and out_scales (fmi_dev.hip),
// shared with fmi_comm_allreduce_mx; *dtype: the storage dtype. And the call after its validation: the comm call's
// shard step.
int mx_check_args(const char* who, int op, int dtype_arg, int alg, int out_dtype, const void* out_scales, int* dtype);
// seed != nullptr: the stochastic-rounding call (out_dtype == dtype), element 0 at stream position `first`.
int reduce_tree_mx(int op, int dtype, int alg, int out_dtype, void* out, void* out_scales, const void* const* ins,
                   const void* const* in_scales, int P, int rank, size_t n, hipStream_t s, const uint64_t* seed = nullptr,
                   uint64_t first = 0);
// The host-side checks the stochastic-rounding calls add: seed, first % 32, first + n.
int mx_sr_check(const char* who, const void* seed, uint64_t first, size_t n);
// kReducePartials for any P and any alignment / dtype (fused kernel where it applies, pairwise passes otherwise):
// outs[t] = the value transformed peer t of reduce_no_order holds in its sendbuf at the end
// (src/comm/PeerToPeer.cpp:66-78); ins in transformed order. Defined in fmi_dev.hip.
int reduce_partials(int op, int dtype, void* const* outs, const void* const* ins, int P, size_t n, hipStream_t s);
// The mean's scale step alone (fmi_scale.hip), in place, any alignment: inout[i] = store(fl_V(value(inout[i]) * fl_V(1 / P))).
// dtype: one of the six float dtypes.
int launch_mean_scale(int dtype, void* inout, size_t n, int P, hipStream_t s);
// The fallback's streaming conversions (fmi_acc32_convert.hip), any alignment: dst[i] = (float)src[i] (exact) and
// dst[i] = the storage type's rounding of src[i]. dtype: FMI_F16, FMI_BF16, FMI_F8E4M3 or FMI_F8E5M2.
int launch_widen_f32(int dtype, float* dst, const void* src, size_t n, hipStream_t s);
int launch_narrow_f32(int dtype, void* dst, const float* src, size_t n, hipStream_t s);
// fmi_dev_convert: dst[i] = narrow_dst(widen_src(src[i])) between any two of f32 / f16 / bf16 / E4M3 / E5M2 (equal
// dtypes: the bits copied), one launch, any alignment, dst == src allowed at equal element size.
int launch_convert(int dst_dtype, void* dst, int src_dtype, const void* src, size_t n, hipStream_t s);
// scan_no_order over B full blocks of 16 peers (2 <= B <= kMaxOnePassScanBlocks, P = 32..143) in one pass: every input read
// once, all 16 B outputs written (fmi_fused_scan_blocked.hip); a ragged last block is left to the caller.
inline constexpr int kMaxOnePassScanBlocks = 8;
inline constexpr int kOnePassScanBlocksNarrow = 4;  // B <= 4 in one translation unit, 5..8 in another
struct BlockedScanPtrs {
    const void* in[sched::kScanBlock * kMaxOnePassScanBlocks];
    void* out[sched::kScanBlock * kMaxOnePassScanBlocks];
};
int launch_scan_blocks_one_pass(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s);
int launch_scan_blocks_one_pass_wide(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s);
// reduce_no_order over any 17..128 peers (ragged last block included) and allreduce_no_order over P = 32, 64, 128
// in one pass: ptrs.in[0..P) the (transformed) inputs, ptrs.out[0] the result of peer `rank` (allreduce)
// (fmi_fused_tree_blocked.hip)
bool tree_blocks_one_pass_covers(int op, int dtype, int alg, int P);
// allreduce_no_order over P = 48, 80, 96, 112 (full blocks pre-fold) in one pass: ptrs.in[0..2^k) the doubling
// group and ptrs.in[2^k..P) the partners, each block permuted by rank % 16 by the caller; rank_hi = rank / 16
bool prefold_blocks_one_pass_covers(int alg, int P);
int launch_prefold_blocks_one_pass(int op, int dtype, int P, const BlockedScanPtrs& ptrs, size_t n, int rank_hi,
                                   hipStream_t s);
// scan_ltr (scan = true: ptrs.out[0..P)) and reduce_ltr (ptrs.out[0]) over 2..128 peers in one pass, the running
// value carried in registers (fmi_fused_chain.hip)
// carry_in: ptrs.in[0] is an earlier segment's running value (scan: ptrs.out[0] is not written).
int launch_chain_one_pass(int op, int dtype, bool scan, int P, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s,
                          bool carry_in = false);
int launch_tree_blocks_one_pass(int op, int dtype, int alg, int P, const BlockedScanPtrs& ptrs, size_t n, int rank,
                                hipStream_t s);
// The 16-bit float instantiations of the one-pass launches above (arguments already checked by them).
int launch_chain_one_pass_half(int op, int dtype, bool scan, int P, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s,
                               bool carry_in);
int launch_tree_blocks_one_pass_half(int op, int dtype, int alg, int P, const BlockedScanPtrs& ptrs, size_t n, int rank,
                                     hipStream_t s);
int launch_prefold_blocks_one_pass_half(int op, int dtype, int P, const BlockedScanPtrs& ptrs, size_t n, int rank_hi,
                                        hipStream_t s);
int launch_scan_blocks_one_pass_half(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s);
int launch_scan_blocks_one_pass_half_wide(int op, int dtype, int B, const BlockedScanPtrs& ptrs, size_t n, hipStream_t s);

// Many independent pairwise combines in one launch (fmi_dev_reduce_pair_batch, fmi_pair_batch.hip): up to
// kPairBatchMax descriptors, every pointer 16-B aligned; workgroup t works on tile t - first_tile[k] of the
// descriptor k with first_tile[k] <= t < first_tile[k + 1] (kPairBatchTile lane groups per tile).
inline constexpr int kPairBatchMax = 64;
inline constexpr unsigned kPairBatchBlock = 256;
inline constexpr int kPairBatchUnroll = 4;
inline constexpr size_t kPairBatchTile = size_t(kPairBatchBlock) * kPairBatchUnroll;
struct PairBatch {
    void* inout[kPairBatchMax];
    const void* in[kPairBatchMax];
    unsigned long long n[kPairBatchMax];         // elements
    unsigned first_tile[kPairBatchMax + 1];      // prefix sums of the descriptors' tile counts
    int count;
};
int launch_pair_batch(int op, int dtype, const PairBatch& pb, hipStream_t s);

// dst <- src (bytes) on stream s: the copy_tile kernel (nontemporal, ≈ the chip's copy rate) when both are
// 16-B aligned, non-overlapping device allocations of >= kDeviceCopyMin bytes; hipMemcpyAsync otherwise
// (host or unknown pointers, small or overlapping copies).
inline constexpr size_t kDeviceCopyMin = size_t(256) << 10;
int device_copy(void* dst, const void* src, size_t bytes, hipStream_t s);

// Workgroups to cover `items` with `block` threads each (at least 1). Callers cap it before narrowing.
inline size_t grid_for(size_t items, unsigned block) {
    const size_t g = (items + block - 1) / block;
    return g == 0 ? 1 : g;
}

}  // namespace fmi::dev
