// fmi_kernels.h — gfx950 (CDNA4) kernels for FMI's bucket reduction.
//
// All kernels here are HBM-streaming element-wise kernels (≈1/12 flop per byte for f32 add): there is
// no dense contraction, so no MFMA and no LDS staging — the work is to keep enough 16-byte
// loads in flight per CU that HBM3E, not latency, is the limit (MI355X_MICROARCH.md §HBM).
//
//   pair_tile / pair_stride   out[i] = op(a[i], b[i])          one pass: 2 reads + 1 write per element
//   tree_kernel               out    = program(x0..x{P-1})     one pass: P reads + 1 write
//   scan_kernel               outs[k]= program_k(x0..x{P-1})   one pass: P reads + P writes
//   synth_kernel              counter-based synthetic buckets (splitmix64), identical to the host
//
// Every access is a 16-B global_load_dwordx4 / global_store_dwordx4 (4 f32/i32, 2 f64/i64, 8 f16/bf16 or 16 8-bit lanes);
// the < 16-B remainder of a bucket is handled by the first threads of block 0 with scalar accesses,
// so a launch never touches a byte outside [0, n).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "fmi_schedule.h"

namespace fmi::dev {

// ---------------------------------------------------------------------------------------------------
// Element ops. Semantics are the reference's built-ins (reference python/PythonCommunicator.h:131-149):
// std::plus, std::multiplies, std::max(a,b) = (a<b)?b:a, std::min(a,b) = (b<a)?b:a — NOT fmaxf/fminf,
// which differ on NaN and on signed zeros. Integer sum/prod wrap (computed in the unsigned type).
// ---------------------------------------------------------------------------------------------------
template <class T>
struct Wrap {
    using type = T;
};
// The 16-bit float elements, _Float16 (IEEE binary16) and __bf16 (the upper 16 bits of binary32): one combine
// widens both operands to f32 (exact), applies the op in f32 and rounds the result back to the storage type
// (round-to-nearest-even, subnormals kept, NaN stays NaN), after EVERY combine of a P-way program: what the
// reference's f.f(mine, received) computes at such an element type (std::plus<__bf16>). max / min compare the
// widened values and keep one operand's 16 bits unchanged.
template <>
struct Wrap<_Float16> {
    using type = float;
};
template <>
struct Wrap<__bf16> {
    using type = float;
};
template <class T>
inline constexpr bool is_half_float_v = std::is_same_v<T, _Float16> || std::is_same_v<T, __bf16>;

// The 8-bit float elements (FMI_F8E4M3, FMI_F8E5M2: the OCP formats, include/fmi_dev.h): one byte each, as wrapper
// types of their own so that uint8_t keeps meaning FMI_U8. The rule of the 16-bit floats holds: one combine widens both
// operands to f32 (exact), applies the op in f32 and narrows, after EVERY combine of a plain P-way program; max / min
// compare the widened values and keep one operand's byte. Narrowing is round-to-nearest-even with subnormals kept and
// does NOT saturate: a rounded magnitude beyond the largest finite value (or +-inf) gives +-inf (E5M2) or NaN (E4M3).
struct f8e4m3 {
    uint8_t b;
};
struct f8e5m2 {
    uint8_t b;
};
template <class T>
inline constexpr bool is_fp8_v = std::is_same_v<T, f8e4m3> || std::is_same_v<T, f8e5m2>;
// The float elements narrower than their f32 value type
template <class T>
inline constexpr bool is_narrow_float_v = is_half_float_v<T> || is_fp8_v<T>;

// f32 -> fp8 in integer code, by the definition: what the synthetic buckets narrow with, on the host and on the device
// alike (their values are exact in the format). M mantissa bits, B the bias.
template <class T>
__host__ __device__ __forceinline__ uint8_t fp8_narrow_sw(float f) {
    constexpr bool k5 = std::is_same_v<T, f8e5m2>;
    constexpr int M = k5 ? 2 : 3, B = k5 ? 15 : 7, emin = 1 - B;
    // the first magnitude that no longer rounds to a finite value or, by the carry out of the mantissa, to the
    // format's own inf / NaN pattern: 2^16 (E5M2: [61440, 2^16) carries into 0x7C), 480 (E4M3: (464, 480) carries into 0x7F)
    constexpr uint32_t over = k5 ? 0x47800000u : 0x43F00000u;
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    const uint32_t s = (u >> 24) & 0x80u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return static_cast<uint8_t>(s | 0x7Fu);
    if (a >= over) return static_cast<uint8_t>(s | (k5 ? 0x7Cu : 0x7Fu));
    const int e = static_cast<int>(a >> 23) - 127;
    if (e >= emin) {
        constexpr int shift = 23 - M;
        const uint32_t r = (a + ((1u << (shift - 1)) - 1u) + ((a >> shift) & 1u)) >> shift;
        return static_cast<uint8_t>(s | (r - (static_cast<uint32_t>(127 - B) << M)));
    }
    if (e < emin - M - 1) return static_cast<uint8_t>(s);  // below half the smallest subnormal
    const uint32_t mant = (a & 0x7FFFFFu) | 0x800000u;
    const int shift = (23 - M) + (emin - e);  // <= 24
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return static_cast<uint8_t>(s | r);
}

// The hardware conversions (v_cvt_pk_f32_fp8 / _bf8, v_cvt_pk_fp8_f32 / _bf8_f32: the OCP encodings on gfx950, no
// clamp): they equal the definition on every input compared.

// the two elements in the low (HI = false) or high half of a word, widened
template <class T, bool HI>
__device__ __forceinline__ float __attribute__((ext_vector_type(2))) fp8_widen2(uint32_t w) {
    if constexpr (std::is_same_v<T, f8e4m3>)
        return __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), HI);
    else
        return __builtin_amdgcn_cvt_pk_f32_bf8(static_cast<int>(w), HI);
}
// `old` with its low / high half replaced by (narrow(x), narrow(y))
template <class T, bool HI>
__device__ __forceinline__ uint32_t fp8_narrow2(float x, float y, uint32_t old) {
    if constexpr (std::is_same_v<T, f8e4m3>) {
        return static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(x, y, static_cast<int>(old), HI));
    } else {
        return static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_bf8_f32(x, y, static_cast<int>(old), HI));
    }
}
template <class T>
__device__ __forceinline__ float fp8_widen(T x) {
    return fp8_widen2<T, false>(x.b).x;
}
template <class T>
__device__ __forceinline__ T fp8_narrow(float f) {
    return T{static_cast<uint8_t>(fp8_narrow2<T, false>(f, f, 0u) & 0xFFu)};
}
__device__ __forceinline__ bool operator<(f8e4m3 a, f8e4m3 b) { return fp8_widen(a) < fp8_widen(b); }
__device__ __forceinline__ bool operator<(f8e5m2 a, f8e5m2 b) { return fp8_widen(a) < fp8_widen(b); }
// "Is a float element" (operand order can change the bits of max / min): the library's own answer, not
// libstdc++'s, which differs between versions for the two 16-bit types.
template <class T>
inline constexpr bool is_float_elem_v = std::is_same_v<T, float> || std::is_same_v<T, double> || is_narrow_float_v<T>;
template <>
struct Wrap<int32_t> {
    using type = uint32_t;
};
template <>
struct Wrap<int64_t> {
    using type = uint64_t;
};
// Sub-dword integers compute in 32 bits (no promotion to a signed int that could overflow) and keep the
// low bits on conversion back, as the reference's std::plus / std::multiplies on A do.
template <>
struct Wrap<int8_t> {
    using type = uint32_t;
};
template <>
struct Wrap<uint8_t> {
    using type = uint32_t;
};
template <>
struct Wrap<int16_t> {
    using type = uint32_t;
};
template <>
struct Wrap<uint16_t> {
    using type = uint32_t;
};

struct OpSum {
    template <class T>
    __device__ __forceinline__ static T apply(T a, T b) {
        if constexpr (is_fp8_v<T>) {
            return fp8_narrow<T>(fp8_widen(a) + fp8_widen(b));
        } else {
            using U = typename Wrap<T>::type;
            return static_cast<T>(static_cast<U>(a) + static_cast<U>(b));
        }
    }
};
struct OpProd {
    template <class T>
    __device__ __forceinline__ static T apply(T a, T b) {
        if constexpr (is_fp8_v<T>) {
            return fp8_narrow<T>(fp8_widen(a) * fp8_widen(b));
        } else {
            using U = typename Wrap<T>::type;
            return static_cast<T>(static_cast<U>(a) * static_cast<U>(b));
        }
    }
};
struct OpMax {
    template <class T>
    __device__ __forceinline__ static T apply(T a, T b) {
        return (a < b) ? b : a;
    }
};
struct OpMin {
    template <class T>
    __device__ __forceinline__ static T apply(T a, T b) {
        return (b < a) ? b : a;
    }
};
// FMI_OP_AVG (include/fmi_dev.h): the mean over the P peers of a fused tree program. Its steps are OpSum's (StepOp), so
// every combine is the SUM program's; `finish` then scales the one value a thread is about to store by r_P = fl_V(1 / P),
// a constant of the instantiation, in the value type V (f32 for the 16-bit floats, plain or Acc32) and narrows once:
// out = store(fl_V(S * r_P)). Only the tree kernels know it: no pairwise, scan or with_op_dtype instantiation exists.
struct OpAvg : OpSum {};
template <class Op>
inline constexpr bool is_avg_v = std::is_same_v<Op, OpAvg>;
template <class Op>
struct StepOp {
    using type = Op;
};
template <>
struct StepOp<OpAvg> {
    using type = OpSum;
};

// ---------------------------------------------------------------------------------------------------
// 16-byte lane groups and their loads/stores.
// ---------------------------------------------------------------------------------------------------
// Sub-dword elements are held as a clang vector (<16 x i8>, <8 x i16>): reinterpreting one as 32-bit
// words is then free, where a plain array is split per element and reassembled (it turned the 16-B loads
// of the 8-bit kernels into 2-byte ones).
template <class T, int W, bool VEC = (sizeof(T) < 4 && W > 1)>
struct LaneStorage {
    T v[W];
};
template <class T, int W>
struct LaneStorage<T, W, true> {
    // the 8-bit floats as their bytes: a lane group of them is only ever read as 32-bit words
    std::conditional_t<is_fp8_v<T>, uint8_t, T> __attribute__((ext_vector_type(W))) v;
};

template <class T, int W>
struct alignas(sizeof(T) * W) Lanes : LaneStorage<T, W> {};

template <class T>
inline constexpr int kVecLanes = 16 / static_cast<int>(sizeof(T));

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

template <bool NT, class T, int W>
__device__ __forceinline__ Lanes<T, W> load_lanes(const T* p) {
    if constexpr (NT && sizeof(T) * W == 16) {
        const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        return __builtin_bit_cast(Lanes<T, W>, r);
    } else {
        return *reinterpret_cast<const Lanes<T, W>*>(p);
    }
}

template <bool NT, class T, int W>
__device__ __forceinline__ void store_lanes(T* p, const Lanes<T, W>& x) {
    if constexpr (NT && sizeof(T) * W == 16) {
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, x), reinterpret_cast<u32x4*>(p));
    } else {
        *reinterpret_cast<Lanes<T, W>*>(p) = x;
    }
}

// 8-bit lanes, four bytes per 32-bit word: sum by SWAR (the carry out of each byte is dropped, exactly
// the wrap of the per-byte add), prod / max / min on packed 16-bit halves (even bytes and odd bytes; the
// low byte of a 16-bit product is the wrapped byte product, signed or not), one or two instructions per
// 2-4 bytes instead of several per byte.
using u16x2 = unsigned short __attribute__((ext_vector_type(2)));
using i16x2 = short __attribute__((ext_vector_type(2)));

template <class Op, class T>
__device__ __forceinline__ uint32_t combine_bytes(uint32_t a, uint32_t b) {
    if constexpr (std::is_same_v<Op, OpSum>) {
        return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
    } else if constexpr (std::is_same_v<Op, OpProd>) {
        const u16x2 ae = __builtin_bit_cast(u16x2, a & 0x00FF00FFu), be = __builtin_bit_cast(u16x2, b & 0x00FF00FFu);
        const u16x2 ao = __builtin_bit_cast(u16x2, (a >> 8) & 0x00FF00FFu), bo = __builtin_bit_cast(u16x2, (b >> 8) & 0x00FF00FFu);
        const uint32_t e = __builtin_bit_cast(uint32_t, static_cast<u16x2>(ae * be)) & 0x00FF00FFu;
        const uint32_t o = __builtin_bit_cast(uint32_t, static_cast<u16x2>(ao * bo)) & 0x00FF00FFu;
        return e | (o << 8);
    } else {
        using V = std::conditional_t<std::is_signed_v<T>, i16x2, u16x2>;
        const V a16 = __builtin_bit_cast(V, a), b16 = __builtin_bit_cast(V, b);
        const V ae = (a16 << 8) >> 8, be = (b16 << 8) >> 8;  // even bytes, widened
        const V ao = a16 >> 8, bo = b16 >> 8;                  // odd bytes, widened
        V e, o;
        if constexpr (std::is_same_v<Op, OpMax>) {
            e = __builtin_elementwise_max(ae, be);
            o = __builtin_elementwise_max(ao, bo);
        } else {
            e = __builtin_elementwise_min(ae, be);
            o = __builtin_elementwise_min(ao, bo);
        }
        return (__builtin_bit_cast(uint32_t, e) & 0x00FF00FFu) | ((__builtin_bit_cast(uint32_t, o) & 0x00FF00FFu) << 8);
    }
}

// 16-bit float lanes, two per 32-bit word, the same bits as Op::apply<T> per element (above).
// f16 sum / prod: packed math (v_pk_add_f16 / v_pk_mul_f16); it equals the widened form: products are exact in
// f32, and a sum's f32 intermediate keeps 24 >= 2 * 11 + 2 bits, so rounding twice is rounding once.
// bf16 sum / prod: the widened form IS the definition: each half to f32 by a shift / a mask, v_pk_add_f32 /
// v_pk_mul_f32, and both results narrowed by one v_cvt_pk_bf16_f32. max / min: compare per half, keep the
// operand's own 16 bits.
// REWIDEN (bf16 max / min): widen from opaque copies of the two words, so that no widened half can be shared with
// another combine. Otherwise the compiler keeps the f32 copies of every value that several ranks' expressions of a
// rank-selecting kernel reuse next to the packed words: 256 VGPRs + 256 AGPRs and 20-24 bytes of scratch per lane
// from 26 peers on; re-widening, P = 31 takes 256 + 48 and no scratch. Only there: these kernels are bound by VALU
// work, and redoing the shifts and masks costs more than the AGPR copies (kRewidenFused below).
using f16x2 = _Float16 __attribute__((ext_vector_type(2)));
using bf16x2 = __bf16 __attribute__((ext_vector_type(2)));
using f32x2 = float __attribute__((ext_vector_type(2)));

template <class Op, class T, bool REWIDEN = false>
__device__ __forceinline__ uint32_t combine_halves(uint32_t a, uint32_t b) {
    constexpr bool kSelect = std::is_same_v<Op, OpMax> || std::is_same_v<Op, OpMin>;
    if constexpr (kSelect) {
        bool lo, hi;  // take b's half
        if constexpr (std::is_same_v<T, _Float16>) {
            const f16x2 x = __builtin_bit_cast(f16x2, a), y = __builtin_bit_cast(f16x2, b);
            lo = std::is_same_v<Op, OpMax> ? (x.x < y.x) : (y.x < x.x);
            hi = std::is_same_v<Op, OpMax> ? (x.y < y.y) : (y.y < x.y);
        } else {
            uint32_t wa = a, wb = b;
            if constexpr (REWIDEN) {
                asm("" : "+v"(wa));
                asm("" : "+v"(wb));
            }
            const float xl = __builtin_bit_cast(float, wa << 16), xh = __builtin_bit_cast(float, wa & 0xFFFF0000u);
            const float yl = __builtin_bit_cast(float, wb << 16), yh = __builtin_bit_cast(float, wb & 0xFFFF0000u);
            lo = std::is_same_v<Op, OpMax> ? (xl < yl) : (yl < xl);
            hi = std::is_same_v<Op, OpMax> ? (xh < yh) : (yh < xh);
        }
        return ((lo ? b : a) & 0x0000FFFFu) | ((hi ? b : a) & 0xFFFF0000u);
    } else if constexpr (std::is_same_v<T, _Float16>) {
        const f16x2 x = __builtin_bit_cast(f16x2, a), y = __builtin_bit_cast(f16x2, b);
        if constexpr (std::is_same_v<Op, OpSum>)
            return __builtin_bit_cast(uint32_t, static_cast<f16x2>(x + y));
        else
            return __builtin_bit_cast(uint32_t, static_cast<f16x2>(x * y));
    } else {
        f32x2 x, y;
        x.x = __builtin_bit_cast(float, a << 16);
        x.y = __builtin_bit_cast(float, a & 0xFFFF0000u);
        y.x = __builtin_bit_cast(float, b << 16);
        y.y = __builtin_bit_cast(float, b & 0xFFFF0000u);
        if constexpr (std::is_same_v<Op, OpSum>)
            return __builtin_bit_cast(uint32_t, __builtin_convertvector(x + y, bf16x2));
        else
            return __builtin_bit_cast(uint32_t, __builtin_convertvector(x * y, bf16x2));
    }
}

// 8-bit float lanes, four per 32-bit word, the same bits as Op::apply<T> per element. sum / prod: both halves of each
// word widened by the packed conversions, v_pk_add_f32 / v_pk_mul_f32, and the four results narrowed two at a time
// into the low and the high half of the result word. max / min: compare the widened values per byte and keep the
// operand's own byte (never re-narrowed).
template <class Op, class T>
__device__ __forceinline__ uint32_t combine_fp8(uint32_t a, uint32_t b) {
    const f32x2 al = fp8_widen2<T, false>(a), ah = fp8_widen2<T, true>(a);
    const f32x2 bl = fp8_widen2<T, false>(b), bh = fp8_widen2<T, true>(b);
    if constexpr (std::is_same_v<Op, OpMax> || std::is_same_v<Op, OpMin>) {
        constexpr bool kMax = std::is_same_v<Op, OpMax>;  // mask: take b's byte
        const uint32_t m = ((kMax ? (al.x < bl.x) : (bl.x < al.x)) ? 0x000000FFu : 0u) |
                           ((kMax ? (al.y < bl.y) : (bl.y < al.y)) ? 0x0000FF00u : 0u) |
                           ((kMax ? (ah.x < bh.x) : (bh.x < ah.x)) ? 0x00FF0000u : 0u) |
                           ((kMax ? (ah.y < bh.y) : (bh.y < ah.y)) ? 0xFF000000u : 0u);
        return (b & m) | (a & ~m);
    } else {
        f32x2 rl, rh;
        if constexpr (std::is_same_v<Op, OpSum>) {
            rl = al + bl;
            rh = ah + bh;
        } else {
            rl = al * bl;
            rh = ah * bh;
        }
        return fp8_narrow2<T, true>(rh.x, rh.y, fp8_narrow2<T, false>(rl.x, rl.y, 0u));
    }
}

template <class Op, class T, int W, bool REWIDEN = false>
__device__ __forceinline__ Lanes<T, W> combine(const Lanes<T, W>& a, const Lanes<T, W>& b) {
    if constexpr (is_fp8_v<T> && W % 4 == 0) {
        struct Words {
            uint32_t w[W / 4];
        };
        const Words x = __builtin_bit_cast(Words, a), y = __builtin_bit_cast(Words, b);
        Words r;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) r.w[k] = combine_fp8<Op, T>(x.w[k], y.w[k]);
        return __builtin_bit_cast(Lanes<T, W>, r);
    } else if constexpr (is_half_float_v<T> && W % 2 == 0) {
        struct Words {
            uint32_t w[W / 2];
        };
        const Words x = __builtin_bit_cast(Words, a), y = __builtin_bit_cast(Words, b);
        Words r;
#pragma unroll
        for (int k = 0; k < W / 2; ++k) r.w[k] = combine_halves<Op, T, REWIDEN>(x.w[k], y.w[k]);
        return __builtin_bit_cast(Lanes<T, W>, r);
    } else if constexpr (sizeof(T) == 1 && W % 4 == 0) {
        struct Words {
            uint32_t w[W / 4];
        };
        const Words x = __builtin_bit_cast(Words, a), y = __builtin_bit_cast(Words, b);
        Words r;
#pragma unroll
        for (int k = 0; k < W / 4; ++k) r.w[k] = combine_bytes<Op, T>(x.w[k], y.w[k]);
        return __builtin_bit_cast(Lanes<T, W>, r);
    } else {
        Lanes<T, W> r;
#pragma unroll
        for (int k = 0; k < W; ++k) r.v[k] = Op::template apply<T>(a.v[k], b.v[k]);
        return r;
    }
}

// f32 accumulation of the 16-bit floats (FMI_ACC_F32, include/fmi_dev.h): the fused kernels' group functions take the
// storage type T (what is loaded and stored) and the value type V (what the program's values are held and combined
// in) as two parameters; the kernels take one element parameter E and read the two from Elem<E> (so that the plain
// instantiations keep their names and their code). V = T everywhere but at E = Acc32<T>, T _Float16 / __bf16: each
// loaded lane group is widened once (exact), the steps are combine<Op, float, W> (v_pk_add_f32 / v_pk_mul_f32), and
// each stored value is narrowed once, round-to-nearest-even with subnormals kept and NaN staying NaN: the conversion
// Op::apply<T> ends with (v_cvt_pk_bf16_f32; v_cvt_f16_f32 / v_cvt_pk_f16_f32, never the rtz pack). At V = T the group
// functions keep their expressions as they were (if constexpr), so the plain kernels compile to the same code.
template <class T>
struct Acc32 {};  // element parameter of a fused kernel: T stored, f32 values (sum / prod, whose bits no rank changes)
template <class E>
struct Elem {
    using storage = E;
    using value = E;
};
template <class T>
struct Elem<Acc32<T>> {
    using storage = T;
    using value = float;
};

template <class V, class T, int W>
__device__ __forceinline__ Lanes<V, W> to_value(const Lanes<T, W>& x) {
    if constexpr (std::is_same_v<V, T>) {
        return x;
    } else {
        static_assert(std::is_same_v<V, float> && is_narrow_float_v<T>, "f32 values of 8- or 16-bit float storage");
        Lanes<V, W> r;
        if constexpr (is_fp8_v<T> && W % 4 == 0) {
            struct Words {
                uint32_t w[W / 4];
            };
            const Words p = __builtin_bit_cast(Words, x);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) {
                const f32x2 lo = fp8_widen2<T, false>(p.w[k]), hi = fp8_widen2<T, true>(p.w[k]);
                r.v[4 * k] = lo.x;
                r.v[4 * k + 1] = lo.y;
                r.v[4 * k + 2] = hi.x;
                r.v[4 * k + 3] = hi.y;
            }
        } else if constexpr (is_fp8_v<T>) {
#pragma unroll
            for (int k = 0; k < W; ++k) r.v[k] = fp8_widen(x.v[k]);
        } else if constexpr (std::is_same_v<T, __bf16> && W % 2 == 0) {
            struct Words {
                uint32_t w[W / 2];
            };
            const Words p = __builtin_bit_cast(Words, x);
#pragma unroll
            for (int k = 0; k < W / 2; ++k) {
                r.v[2 * k] = __builtin_bit_cast(float, p.w[k] << 16);
                r.v[2 * k + 1] = __builtin_bit_cast(float, p.w[k] & 0xFFFF0000u);
            }
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) r.v[k] = static_cast<float>(x.v[k]);
        }
        return r;
    }
}

template <class T, class V, int W>
__device__ __forceinline__ Lanes<T, W> to_storage(const Lanes<V, W>& x) {
    if constexpr (std::is_same_v<V, T>) {
        return x;
    } else {
        static_assert(std::is_same_v<V, float> && is_narrow_float_v<T>, "f32 values of 8- or 16-bit float storage");
        Lanes<T, W> r;
        if constexpr (is_fp8_v<T> && W % 4 == 0) {
            struct Words {
                uint32_t w[W / 4];
            } p;
#pragma unroll
            for (int k = 0; k < W / 4; ++k)
                p.w[k] = fp8_narrow2<T, true>(x.v[4 * k + 2], x.v[4 * k + 3], fp8_narrow2<T, false>(x.v[4 * k], x.v[4 * k + 1], 0u));
            r = __builtin_bit_cast(Lanes<T, W>, p);
        } else if constexpr (is_fp8_v<T>) {
#pragma unroll
            for (int k = 0; k < W; ++k) r.v[k] = fp8_narrow<T>(x.v[k]);
        } else if constexpr (std::is_same_v<T, __bf16> && W % 2 == 0) {
            struct Words {
                uint32_t w[W / 2];
            } p;
#pragma unroll
            for (int k = 0; k < W / 2; ++k) {
                f32x2 y;
                y.x = x.v[2 * k];
                y.y = x.v[2 * k + 1];
                p.w[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(y, bf16x2));
            }
            r = __builtin_bit_cast(Lanes<T, W>, p);
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                float f = x.v[k];
                // One element per lane (the ragged tail): keep the narrowing apart from the combine before it. The
                // compiler otherwise fuses an f32 multiply and the conversion to f16 into v_fma_mixlo_f16 x, y, +0,
                // and a product that is -0 comes out as +0.
                if constexpr (W == 1) asm("" : "+v"(f));
                r.v[k] = static_cast<T>(f);
            }
        }
        return r;
    }
}

// OpAvg's last step: the value a tree kernel is about to store, times r_P, as storage lanes. f32 / f64: one IEEE multiply
// in the element type. 16-bit floats: the value in f32 (widened, exact, where the program keeps 16-bit values), one f32
// multiply, and the narrowing Op::apply ends with, from an opaque register in every lane-group width: the compiler
// otherwise fuses multiply and narrowing into v_fma_mixlo_f16 x, y, +0 (to_storage above), and -0 * r comes out as +0.
template <class T, int P, class V, int W>
__device__ __forceinline__ Lanes<T, W> finish_avg(const Lanes<V, W>& x) {
    if constexpr (is_narrow_float_v<T>) {
        constexpr float r = 1.0f / static_cast<float>(P);
        Lanes<float, W> f = to_value<float>(x);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float y = f.v[k] * r;
            asm("" : "+v"(y));
            f.v[k] = y;
        }
        return to_storage<T>(f);
    } else {
        static_assert(std::is_same_v<V, T> && (std::is_same_v<T, float> || std::is_same_v<T, double>), "mean of float elements");
        constexpr T r = static_cast<T>(1) / static_cast<T>(P);
        Lanes<T, W> y;
#pragma unroll
        for (int k = 0; k < W; ++k) y.v[k] = x.v[k] * r;
        return y;
    }
}

// Buffer-op form of the fused kernels' 16-B accesses (pol = 1, FMI_TUNE_FUSED_POLICY): every access of a
// 256-thread tile goes through a descriptor based at the tile's first byte of that bucket (a uniform
// 64-bit address, so any bucket size) with the lane's 32-bit byte offset, and carries an explicit cache
// policy: loads nt; the tree's one output stream sc1 (written lines leave the XCD L2 at once), the scan's
// P output streams nt sc1. tools/microbench_cachepol.hip measured, on the same buffers, tree P = 8 3.3 %
// and scan P = 8 4.6 % faster than global_load / global_store nt (bit-identical results) with few rotating
// sets; with no set re-read from the MALL (tools/ab_fused_policy.py --footprint-gib 6) the scans keep ~2 %,
// trees of 4 peers 2.4 %, trees of 8 / 16 are within 1 % either way. The pairwise kernel keeps global nt
// accesses and stores some of its tiles with sc1 (pair_tile below).
inline constexpr int kAuxNT = 2, kAuxSC1 = 16;
inline constexpr int kTreeStoreAux = kAuxSC1, kScanStoreAux = kAuxNT | kAuxSC1, kFusedLoadAux = kAuxNT;
using b128 = unsigned int __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* tile_base) {
    // raw (stride 0) descriptor, 32-bit data format; num_records covers any tile (<= 64 KiB past its base)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(tile_base), 0, 1 << 30, 0x00020000);
}
template <int AUX, class T, int W>
__device__ __forceinline__ Lanes<T, W> load_tile(const void* bucket, size_t tile_byte, unsigned lane_byte) {
    static_assert(sizeof(T) * W == 16, "16-B lane groups");
    const b128 r = __builtin_amdgcn_raw_buffer_load_b128(tile_rsrc(static_cast<const char*>(bucket) + tile_byte), lane_byte, 0, AUX);
    return __builtin_bit_cast(Lanes<T, W>, r);
}
template <int AUX, class T, int W>
__device__ __forceinline__ void store_tile(void* bucket, size_t tile_byte, unsigned lane_byte, const Lanes<T, W>& x) {
    static_assert(sizeof(T) * W == 16, "16-B lane groups");
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(b128, x), tile_rsrc(static_cast<char*>(bucket) + tile_byte),
                                           lane_byte, 0, AUX);
}

// Device copy (device_copy in fmi_dev.hip: the reference's P = 1 allreduce and every staging copy of the
// communicator): the pair tile's shape with one stream in and one out — U 16-B vectors per thread (U = 1 in
// the library, profiles/r04_copy_unroll.jsonl), one tile per workgroup. Whole tiles load nontemporal and store with sc1 through a buffer descriptor (the tree kernel's
// policy, above): 4.6 % faster than global nontemporal stores at 256 MiB, 3 % at 64 MiB, with no set
// re-read from the MALL (profiles/archive/r03_copypol.jsonl). The partial last tile
// goes through bounds-checked global accesses; workgroup 0 copies the sub-16-B tail. Algorithmic HBM bytes:
// 2 x bytes. Both pointers 16-B aligned.
template <int U>
__global__ void __launch_bounds__(256) copy_tile(char* out, const char* in, size_t bytes) {
    const size_t nvec = bytes / 16;
    const size_t base = static_cast<size_t>(blockIdx.x) * U * 256 + threadIdx.x;
    if (static_cast<size_t>(blockIdx.x + 1) * U * 256 <= nvec) {
        const size_t tile_byte = static_cast<size_t>(blockIdx.x) * U * 256 * 16;
        Lanes<unsigned, 4> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            v[u] = load_tile<kAuxNT, unsigned, 4>(in, tile_byte, static_cast<unsigned>((u * 256 + threadIdx.x) * 16));
#pragma unroll
        for (int u = 0; u < U; ++u)
            store_tile<kAuxSC1, unsigned, 4>(out, tile_byte, static_cast<unsigned>((u * 256 + threadIdx.x) * 16), v[u]);
    } else {
        const u32x4* src = reinterpret_cast<const u32x4*>(in);
        u32x4* dst = reinterpret_cast<u32x4*>(out);
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (base + u * 256 < nvec) v[u] = __builtin_nontemporal_load(src + base + u * 256);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (base + u * 256 < nvec) __builtin_nontemporal_store(v[u], dst + base + u * 256);
    }
    if (blockIdx.x == 0 && nvec * 16 + threadIdx.x < bytes) out[nvec * 16 + threadIdx.x] = in[nvec * 16 + threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------
// Pairwise combine. A "tile" is U vectors per thread: thread t of block b owns vectors
// b*U*B + u*B + t (u < U), so each of the U wave-instructions is one contiguous 1-KiB access and each
// thread keeps 2U independent 16-B loads in flight before its first add.
// ---------------------------------------------------------------------------------------------------
// NT: cache policy bitmask — bit 0 nontemporal loads, bit 1 nontemporal stores. `sc1` (uniform per tile):
// store this tile with sc1 instead (pair_tile's sc1 tiles, FMI_TUNE_PAIR_SC1_OF_8).
template <class Op, class T, int U, int NT>
__device__ __forceinline__ void pair_tile_body(T* out, const T* a, const T* b, size_t nvec, size_t tile, bool sc1 = false) {
    constexpr int W = kVecLanes<T>;
    constexpr bool NTL = (NT & 1) != 0;
    constexpr bool NTS = (NT & 2) != 0;
    using L = Lanes<T, W>;
    const size_t B = blockDim.x;
    const size_t base = tile * U * B + threadIdx.x;
    L va[U], vb[U];
    if (tile * U * B + U * B <= nvec) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            va[u] = load_lanes<NTL, T, W>(a + (base + u * B) * W);
            vb[u] = load_lanes<NTL, T, W>(b + (base + u * B) * W);
        }
        // one descriptor at the tile's first output byte, lane offsets < U * B * 16 (U = 8: not taken; the
        // second store path spills the 8-bit max / min forms to scratch under the 1024-thread bound)
        if (U <= 4 && sc1) {
            const size_t tile_byte = tile * U * B * 16;
#pragma unroll
            for (int u = 0; u < U; ++u)
                store_tile<kAuxSC1, T, W>(out, tile_byte, static_cast<unsigned>((u * B + threadIdx.x) * 16),
                                          combine<Op, T, W>(va[u], vb[u]));
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) store_lanes<NTS, T, W>(out + (base + u * B) * W, combine<Op, T, W>(va[u], vb[u]));
        }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + u * B;
            if (i < nvec) {
                va[u] = load_lanes<NTL, T, W>(a + i * W);
                vb[u] = load_lanes<NTL, T, W>(b + i * W);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = base + u * B;
            if (i < nvec) store_lanes<NTS, T, W>(out + i * W, combine<Op, T, W>(va[u], vb[u]));
        }
    }
}

template <class Op, class T>
__device__ __forceinline__ void pair_tail(T* out, const T* a, const T* b, size_t n) {
    constexpr int W = kVecLanes<T>;
    const size_t first = (n / W) * W;
    if (blockIdx.x == 0 && first + threadIdx.x < n) {
        const size_t i = first + threadIdx.x;
        out[i] = Op::template apply<T>(a[i], b[i]);
    }
}

// One-shot grid: one tile per workgroup. Pointers must be 16-B aligned. Whole tiles t with t % 8 < sc1_k
// store with sc1, the rest nontemporal (default 0: none, the round-1 kernel the exploration tools compare
// against). Consecutive workgroups are dispatched to different XCDs, so sc1_k of the 8 XCDs store sc1
// (FMI_TUNE_PAIR_SC1_OF_8; tools/ab_pair_sc1.py).
template <class Op, class T, int U, int NT>
__global__ void __launch_bounds__(1024) pair_tile(T* out, const T* a, const T* b, size_t n, unsigned sc1_k = 0) {
    const size_t nvec = n / kVecLanes<T>;
    pair_tile_body<Op, T, U, NT>(out, a, b, nvec, blockIdx.x, (blockIdx.x & 7u) < sc1_k);
    pair_tail<Op, T>(out, a, b, n);
}

// Grid-stride: a fixed grid (k workgroups per CU) walks the tiles. Pointers must be 16-B aligned. Every
// tile stores nontemporal (a second store path inside the loop spills the U = 8 forms to scratch).
template <class Op, class T, int U, int NT>
__global__ void __launch_bounds__(1024) pair_stride(T* out, const T* a, const T* b, size_t n) {
    const size_t nvec = n / kVecLanes<T>;
    const size_t ntiles = (nvec + static_cast<size_t>(U) * blockDim.x - 1) / (static_cast<size_t>(U) * blockDim.x);
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) pair_tile_body<Op, T, U, NT>(out, a, b, nvec, t);
    pair_tail<Op, T>(out, a, b, n);
}

// Any alignment: scalar grid-stride loop.
template <class Op, class T>
__global__ void __launch_bounds__(256) pair_scalar(T* out, const T* a, const T* b, size_t n) {
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * blockDim.x)
        out[i] = Op::template apply<T>(a[i], b[i]);
}

// ---------------------------------------------------------------------------------------------------
// Fused P-way kernels: evaluate a sched::Fused<ALG,P> program per 16-B lane group, every value in
// registers. Indices into the value array are template constants (fold over index_sequence), so the
// array is promoted to VGPRs — no scratch.
// ---------------------------------------------------------------------------------------------------
// Peer buckets are streamed exactly once per launch: nontemporal loads/stores (global_* nt) keep them
// from displacing other data in L2/MALL, as for the pairwise kernel (tools/tune_pair.py: +13%).
inline constexpr bool kFusedNT = true;

struct PeerPtrs {
    const void* in[sched::kFusedInputCap];
    void* out[sched::kFusedInputCap];
};

// Program fields as integral constants: reading them through these variable templates guarantees the
// value-array indices are folded in the front end, so SROA keeps every value in VGPRs (no scratch).
template <int ALG, int P, size_t S>
inline constexpr int kStepA = sched::Fused<ALG, P>::prog.step[S].a;
template <int ALG, int P, size_t S>
inline constexpr int kStepB = sched::Fused<ALG, P>::prog.step[S].b;
template <int ALG, int P, size_t R>
inline constexpr int kOut = sched::Fused<ALG, P>::prog.out[R];
template <int ALG, int P>
inline constexpr int kNumSteps = sched::Fused<ALG, P>::prog.nsteps;

// The rank-selecting kernels (ALL_RANKS) evaluate every rank's expression. Their bf16 max / min combines re-widen
// (combine_halves) from kRewidenMinPeers peers on, where the shared widened copies no longer fit the register file
// (max spills from 26 peers, min from 30). Below, sharing them is faster: the 24-peer kernel runs at 0.48 of the
// f32 kernel's rate against 0.41 re-widening.
inline constexpr int kRewidenMinPeers = 26;
template <class T, bool ALL_RANKS, int P>
inline constexpr bool kRewidenFused = ALL_RANKS && std::is_same_v<T, __bf16> && P >= kRewidenMinPeers;

template <class Op, class T, int W, int ALG, int P, bool REWIDEN = false, size_t... S>
__device__ __forceinline__ void run_steps(Lanes<T, W>* v, std::index_sequence<S...>) {
    ((v[P + S] = combine<Op, T, W, REWIDEN>(v[kStepA<ALG, P, S>], v[kStepB<ALG, P, S>])), ...);
}

template <class T, int W, int P, class V, size_t... I>
__device__ __forceinline__ void load_peers(Lanes<V, W>* v, const PeerPtrs& ptrs, size_t elem,
                                           std::index_sequence<I...>) {
    if constexpr (std::is_same_v<V, T>)
        ((v[I] = load_lanes<kFusedNT, T, W>(static_cast<const T*>(ptrs.in[I]) + elem)), ...);
    else
        ((v[I] = to_value<V>(load_lanes<kFusedNT, T, W>(static_cast<const T*>(ptrs.in[I]) + elem))), ...);
}

// The value as an opaque register operand. A select chain over loads from one array (pick_rank below) is
// otherwise folded by LLVM into a single load at a rank-dependent index, which pins the whole value array
// in scratch memory (it did, for every rank-aware instantiation, up to 1.3 KiB per thread at P = 16).
template <class T, int W>
__device__ __forceinline__ Lanes<T, W> opaque(Lanes<T, W> x) {
    if constexpr (sizeof(x) == 16) {
        u32x4 b = __builtin_bit_cast(u32x4, x);
        asm("" : "+v"(b));
        return __builtin_bit_cast(Lanes<T, W>, b);
    } else if constexpr (sizeof(x) == 8) {
        uint64_t b = __builtin_bit_cast(uint64_t, x);
        asm("" : "+v"(b));
        return __builtin_bit_cast(Lanes<T, W>, b);
    } else if constexpr (sizeof(x) == 4) {
        uint32_t b = __builtin_bit_cast(uint32_t, x);
        asm("" : "+v"(b));
        return __builtin_bit_cast(Lanes<T, W>, b);
    } else {
        static_assert(sizeof(x) == 2, "lane group of 2, 4, 8 or 16 bytes");
        uint32_t b = __builtin_bit_cast(uint16_t, x);  // one 16-bit float element (the W = 1 tail groups)
        asm("" : "+v"(b));
        return __builtin_bit_cast(Lanes<T, W>, static_cast<uint16_t>(b));
    }
}

template <class T, int W, int ALG, int P, size_t... R>
__device__ __forceinline__ Lanes<T, W> pick_rank(const Lanes<T, W>* v, int rank, std::index_sequence<R...>) {
    Lanes<T, W> r = v[kOut<ALG, P, 0>];
    ((r = (rank == static_cast<int>(R)) ? opaque(v[kOut<ALG, P, R>]) : r), ...);
    return r;
}

template <class T, int W, int ALG, int P, class V, size_t... R>
__device__ __forceinline__ void store_all(const Lanes<V, W>* v, const PeerPtrs& ptrs, size_t elem,
                                          std::index_sequence<R...>) {
    if constexpr (std::is_same_v<V, T>)
        ((store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[R]) + elem, v[kOut<ALG, P, R>])), ...);
    else
        ((store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[R]) + elem, to_storage<T>(v[kOut<ALG, P, R>]))), ...);
}

template <class T, int W, int P, class V, size_t... I>
__device__ __forceinline__ void load_peers_tile(Lanes<V, W>* v, const PeerPtrs& ptrs, size_t tile_byte, unsigned lane_byte,
                                                std::index_sequence<I...>) {
    if constexpr (std::is_same_v<V, T>)
        ((v[I] = load_tile<kFusedLoadAux, T, W>(ptrs.in[I], tile_byte, lane_byte)), ...);
    else
        ((v[I] = to_value<V>(load_tile<kFusedLoadAux, T, W>(ptrs.in[I], tile_byte, lane_byte))), ...);
}

// ALL_RANKS: honour `rank` (output = the value peer `rank` holds). Needed only where operand order can
// change bits (float max/min on ±0); otherwise rank 0's expression is bit-identical for every peer.
// V: the value type (to_value / to_storage above); T itself but in the acc32 kernels.
template <class Op, class T, int ALG, int P, bool ALL_RANKS, int W, class V = T>
__device__ __forceinline__ void tree_group(const PeerPtrs& ptrs, int rank, size_t elem) {
    Lanes<V, W> v[P + kNumSteps<ALG, P>];
    load_peers<T, W, P>(v, ptrs, elem, std::make_index_sequence<P>{});
    run_steps<typename StepOp<Op>::type, V, W, ALG, P, kRewidenFused<V, ALL_RANKS, P>>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    Lanes<V, W> r;
    if constexpr (ALL_RANKS)
        r = pick_rank<V, W, ALG, P>(v, rank, std::make_index_sequence<P>{});
    else
        r = v[kOut<ALG, P, 0>];
    if constexpr (is_avg_v<Op>)
        store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[0]) + elem, finish_avg<T, P>(r));
    else if constexpr (std::is_same_v<V, T>)
        store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[0]) + elem, r);
    else
        store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[0]) + elem, to_storage<T>(r));
}

template <class Op, class T, int ALG, int P, bool ALL_RANKS, int W, class V = T>
__device__ __forceinline__ void tree_group_tile(const PeerPtrs& ptrs, int rank, size_t tile_byte, unsigned lane_byte) {
    Lanes<V, W> v[P + kNumSteps<ALG, P>];
    load_peers_tile<T, W, P>(v, ptrs, tile_byte, lane_byte, std::make_index_sequence<P>{});
    run_steps<typename StepOp<Op>::type, V, W, ALG, P, kRewidenFused<V, ALL_RANKS, P>>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    Lanes<V, W> r;
    if constexpr (ALL_RANKS)
        r = pick_rank<V, W, ALG, P>(v, rank, std::make_index_sequence<P>{});
    else
        r = v[kOut<ALG, P, 0>];
    if constexpr (is_avg_v<Op>)
        store_tile<kTreeStoreAux, T, W>(ptrs.out[0], tile_byte, lane_byte, finish_avg<T, P>(r));
    else if constexpr (std::is_same_v<V, T>)
        store_tile<kTreeStoreAux, T, W>(ptrs.out[0], tile_byte, lane_byte, r);
    else
        store_tile<kTreeStoreAux, T, W>(ptrs.out[0], tile_byte, lane_byte, to_storage<T>(r));
}

// Launched with one thread per 16-B lane group up to kFusedGridCap workgroups; beyond that (buckets of
// > 2^30 lane groups) each thread strides over the rest, so the grid never exceeds HIP's 2^32-thread limit.
inline constexpr size_t kFusedGridCap = size_t(1) << 22;

// pol = 1: buffer accesses tile by tile (the tile index is uniform, so each tile's descriptors are scalar);
// pol = 0: global accesses.
// E: the element type, or Acc32<T> (T stored, f32 values).
template <class Op, class E, int ALG, int P, bool ALL_RANKS>
__global__ void __launch_bounds__(256) tree_kernel(PeerPtrs ptrs, size_t n, int rank, int pol) {
    using T = typename Elem<E>::storage;
    using V = typename Elem<E>::value;
    constexpr int W = kVecLanes<T>;
    const size_t nvec = n / W;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec)
                tree_group_tile<Op, T, ALG, P, ALL_RANKS, W, V>(ptrs, rank, tile * B * 16, threadIdx.x * 16u);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            tree_group<Op, T, ALG, P, ALL_RANKS, W, V>(ptrs, rank, g * W);
    }
    const size_t first = nvec * W;
    if (blockIdx.x == 0 && first + threadIdx.x < n) tree_group<Op, T, ALG, P, ALL_RANKS, 1, V>(ptrs, rank, first + threadIdx.x);
}

// Carry programs (sched::is_carry_alg) leave output 0 alone: value 0 is the carry itself.
template <class T, int W, int ALG, int P, class V, size_t... R>
__device__ __forceinline__ void store_after_carry(const Lanes<V, W>* v, const PeerPtrs& ptrs, size_t elem,
                                                  std::index_sequence<R...>) {
    if constexpr (std::is_same_v<V, T>)
        ((store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[R + 1]) + elem, v[kOut<ALG, P, R + 1>])), ...);
    else
        ((store_lanes<kFusedNT, T, W>(static_cast<T*>(ptrs.out[R + 1]) + elem, to_storage<T>(v[kOut<ALG, P, R + 1>]))), ...);
}

template <class Op, class T, int ALG, int P, int W, class V = T>
__device__ __forceinline__ void scan_group(const PeerPtrs& ptrs, size_t elem) {
    Lanes<V, W> v[P + kNumSteps<ALG, P>];
    load_peers<T, W, P>(v, ptrs, elem, std::make_index_sequence<P>{});
    run_steps<Op, V, W, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    if constexpr (sched::is_carry_alg(ALG))
        store_after_carry<T, W, ALG, P>(v, ptrs, elem, std::make_index_sequence<P - 1>{});
    else
        store_all<T, W, ALG, P>(v, ptrs, elem, std::make_index_sequence<P>{});
}

template <class Op, class T, int ALG, int P, int W, class V = T>
__device__ __forceinline__ void scan_group_tile(const PeerPtrs& ptrs, size_t tile_byte, unsigned lane_byte) {
    Lanes<V, W> v[P + kNumSteps<ALG, P>];
    load_peers_tile<T, W, P>(v, ptrs, tile_byte, lane_byte, std::make_index_sequence<P>{});
    run_steps<Op, V, W, ALG, P>(v, std::make_index_sequence<kNumSteps<ALG, P>>{});
    constexpr int first_out = sched::is_carry_alg(ALG) ? 1 : 0;  // carry programs leave output 0 alone
    [&]<size_t... R>(std::index_sequence<R...>) {
        if constexpr (std::is_same_v<V, T>)
            ((store_tile<kScanStoreAux, T, W>(ptrs.out[R + first_out], tile_byte, lane_byte, v[kOut<ALG, P, R + first_out>])), ...);
        else
            ((store_tile<kScanStoreAux, T, W>(ptrs.out[R + first_out], tile_byte, lane_byte,
                                              to_storage<T>(v[kOut<ALG, P, R + first_out>]))),
             ...);
    }(std::make_index_sequence<P - first_out>{});
}

// E: as for tree_kernel; with Acc32<T> every stored prefix (or partial) is its own f32 value, narrowed once.
template <class Op, class E, int ALG, int P>
__global__ void __launch_bounds__(256) scan_kernel(PeerPtrs ptrs, size_t n, int pol) {
    using T = typename Elem<E>::storage;
    using V = typename Elem<E>::value;
    constexpr int W = kVecLanes<T>;
    const size_t nvec = n / W;
    if (pol == 1) {
        const size_t B = blockDim.x;
        for (size_t tile = blockIdx.x; tile * B < nvec; tile += gridDim.x)
            if (tile * B + threadIdx.x < nvec) scan_group_tile<Op, T, ALG, P, W, V>(ptrs, tile * B * 16, threadIdx.x * 16u);
    } else {
        const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
        for (size_t g = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < nvec; g += stride)
            scan_group<Op, T, ALG, P, W, V>(ptrs, g * W);
    }
    const size_t first = nvec * W;
    if (blockIdx.x == 0 && first + threadIdx.x < n) scan_group<Op, T, ALG, P, 1, V>(ptrs, first + threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------
// Synthetic buckets: h = splitmix64(seed ^ (peer << 40) ^ i).
// ---------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <class T>
__host__ __device__ __forceinline__ T synth_value(uint64_t h) {
    if constexpr (std::is_same_v<T, float>) {
        return static_cast<float>(h >> 40) * 0x1p-24f * 2.0f - 1.0f;
    } else if constexpr (std::is_same_v<T, double>) {
        return static_cast<double>(h >> 11) * 0x1p-53 * 2.0 - 1.0;
    } else if constexpr (std::is_same_v<T, _Float16>) {
        // multiples of 2^-10 in [-1, 1): exact in f32 and in f16 (at most 11 significant bits)
        return static_cast<_Float16>(static_cast<float>(h >> 53) * 0x1p-11f * 2.0f - 1.0f);
    } else if constexpr (std::is_same_v<T, __bf16>) {
        // multiples of 2^-7 in [-1, 1): exact in f32 and in bf16 (at most 8 significant bits)
        return static_cast<__bf16>(static_cast<float>(h >> 56) * 0x1p-8f * 2.0f - 1.0f);
    } else if constexpr (std::is_same_v<T, f8e4m3>) {
        // multiples of 2^-3 in [-1, 1): exact in f32 and in E4M3 (at most 4 significant bits)
        return f8e4m3{fp8_narrow_sw<f8e4m3>(static_cast<float>(h >> 60) * 0x1p-4f * 2.0f - 1.0f)};
    } else if constexpr (std::is_same_v<T, f8e5m2>) {
        // multiples of 2^-2 in [-1, 1): exact in f32 and in E5M2 (at most 3 significant bits)
        return f8e5m2{fp8_narrow_sw<f8e5m2>(static_cast<float>(h >> 61) * 0x1p-3f * 2.0f - 1.0f)};
    } else {
        // integers: the top 8·sizeof(T) bits of h (i32 = h >> 32, i64 = h, as before)
        using U = std::make_unsigned_t<T>;
        return static_cast<T>(static_cast<U>(h >> (64 - 8 * sizeof(T))));
    }
}

template <class T>
__global__ void __launch_bounds__(256) synth_kernel(T* buf, size_t n, uint64_t seed, uint32_t peer, uint64_t first) {
    const uint64_t key = seed ^ (static_cast<uint64_t>(peer) << 40);
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * blockDim.x)
        buf[i] = synth_value<T>(splitmix64(key ^ (first + i)));
}

}  // namespace fmi::dev
