// FMI::Dev — C++ RAII layer over the C-ABI in include/fmi_dev.h (libfmi_dev.so, gfx950).
//
// Error convention: a C-ABI FMI_ERR_TIMEOUT becomes FMI::Utils::Timeout (reference
// include/utils/Common.h:11-15, what its channels throw when a peer stays away, src/comm/Direct.cpp:28-30);
// every other status != 0 a std::runtime_error carrying fmi_last_error(), the exception type the reference
// itself throws for usage errors (reference include/Communicator.h:90,114,138).
#ifndef FMI_AMD_DEV_DEVICE_H
#define FMI_AMD_DEV_DEVICE_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../utils/Common.h"
#include "fmi_dev.h"  // C-ABI: add -I<repo>/include

namespace FMI::Dev {

inline void check(int status, const char* what) {
    if (status == FMI_ERR_TIMEOUT) throw Utils::Timeout();
    if (status != FMI_OK) throw std::runtime_error(std::string(what) + ": " + fmi_last_error());
}

// The 16-bit float element types (FMI_F16: IEEE binary16; FMI_BF16: the upper 16 bits of binary32) as trivially
// copyable 2-byte structs over the raw bits, so no host compiler needs _Float16 / __bf16. Arithmetic is the
// C-ABI's definition (include/fmi_dev.h): widen to float (exact), operate in float, round back to nearest even
// (subnormals kept, NaN stays NaN); `<` and `==` compare the widened values, so std::max / std::min keep one
// operand's bits. An FMI user whose buckets are __bf16 / _Float16 binds them by reinterpreting the storage
// (same size, same bits): see INTEGRATION.md.
namespace detail {
inline float bits_to_float(std::uint32_t u) {
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}
inline std::uint32_t float_to_bits(float f) {
    std::uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}
}  // namespace detail

struct bfloat16 {
    std::uint16_t bits = 0;
    bfloat16() = default;
    explicit bfloat16(float f) {
        const std::uint32_t u = detail::float_to_bits(f);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u)
            bits = static_cast<std::uint16_t>((u >> 16) | 0x0040u);  // NaN stays NaN (quieted)
        else
            bits = static_cast<std::uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);  // round to nearest even
    }
    static bfloat16 from_bits(std::uint16_t b) {
        bfloat16 x;
        x.bits = b;
        return x;
    }
    explicit operator float() const { return detail::bits_to_float(static_cast<std::uint32_t>(bits) << 16); }
};

struct half {
    std::uint16_t bits = 0;
    half() = default;
    explicit half(float f) {
        const std::uint32_t u = detail::float_to_bits(f);
        const std::uint32_t sign = (u >> 16) & 0x8000u, mag = u & 0x7FFFFFFFu;
        if (mag > 0x7F800000u) {
            bits = static_cast<std::uint16_t>(sign | 0x7E00u | ((mag >> 13) & 0x01FFu));  // NaN stays NaN (quieted)
        } else if (mag >= 0x47800000u) {  // >= 2^16 (and inf): past the largest finite half even before rounding
            bits = static_cast<std::uint16_t>(sign | 0x7C00u);
        } else if (mag >= 0x38800000u) {  // normal half, 2^-14 <= |f|: drop 13 bits, round to nearest even
            const std::uint32_t v = mag - 0x38000000u;  // rebias 127 -> 15; a carry out of the mantissa bumps the
            bits = static_cast<std::uint16_t>(sign | ((v + 0x0FFFu + ((v >> 13) & 1u)) >> 13));  // exponent (to inf)
        } else if (mag < 0x33000000u) {  // < 2^-25: below half of the smallest subnormal
            bits = static_cast<std::uint16_t>(sign);
        } else {  // subnormal half: |f| = m * 2^(e-150) with the implicit bit, in units of 2^-24
            const int e = static_cast<int>(mag >> 23);
            const std::uint32_t m = (mag & 0x007FFFFFu) | 0x00800000u;
            const int shift = 126 - e;  // 14..24: m >> shift is |f| / 2^-24
            const std::uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
            bits = static_cast<std::uint16_t>(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
        }
    }
    static half from_bits(std::uint16_t b) {
        half x;
        x.bits = b;
        return x;
    }
    explicit operator float() const {
        const std::uint32_t sign = static_cast<std::uint32_t>(bits & 0x8000u) << 16;
        const std::uint32_t e = (bits >> 10) & 0x1Fu, m = bits & 0x03FFu;
        if (e == 0x1Fu) return detail::bits_to_float(sign | 0x7F800000u | (m << 13));
        if (e != 0) return detail::bits_to_float(sign | ((e + 112u) << 23) | (m << 13));
        const float mag = static_cast<float>(m) * 0x1p-24f;  // zero or subnormal: exact
        return sign ? -mag : mag;
    }
};

inline bfloat16 operator+(bfloat16 a, bfloat16 b) { return bfloat16(static_cast<float>(a) + static_cast<float>(b)); }
inline bfloat16 operator*(bfloat16 a, bfloat16 b) { return bfloat16(static_cast<float>(a) * static_cast<float>(b)); }
inline bool operator<(bfloat16 a, bfloat16 b) { return static_cast<float>(a) < static_cast<float>(b); }
inline bool operator==(bfloat16 a, bfloat16 b) { return static_cast<float>(a) == static_cast<float>(b); }
inline half operator+(half a, half b) { return half(static_cast<float>(a) + static_cast<float>(b)); }
inline half operator*(half a, half b) { return half(static_cast<float>(a) * static_cast<float>(b)); }
inline bool operator<(half a, half b) { return static_cast<float>(a) < static_cast<float>(b); }
inline bool operator==(half a, half b) { return static_cast<float>(a) == static_cast<float>(b); }
static_assert(sizeof(half) == 2 && sizeof(bfloat16) == 2 && std::is_trivially_copyable_v<half> &&
                  std::is_trivially_copyable_v<bfloat16>,
              "16-bit float elements are their raw bits");

// The 8-bit float element types (FMI_F8E4M3: OCP E4M3, e4m3fn; FMI_F8E5M2: OCP E5M2) as trivially copyable 1-byte
// structs over the raw bits. Arithmetic is the C-ABI's definition (include/fmi_dev.h): widen to float (exact), operate
// in float, narrow: round to nearest even, subnormals and the zero's sign kept, NOT saturating (a rounded magnitude
// beyond the largest finite value, or +-inf, gives +-inf for E5M2 and NaN for E4M3; NaN stays NaN). `<` and `==`
// compare the widened values, so std::max / std::min keep one operand's byte.
namespace detail {
// MANT mantissa bits, BIAS; OVER: the first magnitude (f32 bits) that no longer rounds to a finite value or, by the
// carry out of the mantissa, to the format's own inf / NaN pattern; OVER_BYTE: what it gives.
template <int MANT, int BIAS, std::uint32_t OVER, std::uint8_t OVER_BYTE>
inline std::uint8_t narrow_fp8(float f) {
    constexpr int emin = 1 - BIAS;
    const std::uint32_t u = float_to_bits(f);
    const std::uint32_t sign = (u >> 24) & 0x80u, mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return static_cast<std::uint8_t>(sign | 0x7Fu);
    if (mag >= OVER) return static_cast<std::uint8_t>(sign | OVER_BYTE);
    const int e = static_cast<int>(mag >> 23) - 127;
    if (e >= emin) {  // normal: drop 23 - MANT bits, round to nearest even, rebias
        constexpr int shift = 23 - MANT;
        const std::uint32_t r = (mag + ((1u << (shift - 1)) - 1u) + ((mag >> shift) & 1u)) >> shift;
        return static_cast<std::uint8_t>(sign | (r - (static_cast<std::uint32_t>(127 - BIAS) << MANT)));
    }
    if (e < emin - MANT - 1) return static_cast<std::uint8_t>(sign);  // below half of the smallest subnormal
    const std::uint32_t m = (mag & 0x007FFFFFu) | 0x00800000u;
    const int shift = (23 - MANT) + (emin - e);  // <= 24: m >> shift is |f| in units of the smallest subnormal
    const std::uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    return static_cast<std::uint8_t>(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
}
template <int MANT, int BIAS>
inline float widen_fp8(std::uint8_t b) {
    const std::uint32_t sign = static_cast<std::uint32_t>(b & 0x80u) << 24;
    const std::uint32_t e = (b & 0x7Fu) >> MANT, m = b & ((1u << MANT) - 1u);
    if (e != 0) return bits_to_float(sign | ((e + 127u - BIAS) << 23) | (m << (23 - MANT)));
    const float mag = static_cast<float>(m) * bits_to_float(static_cast<std::uint32_t>(127 + 1 - BIAS - MANT) << 23);
    return sign ? -mag : mag;  // zero or subnormal: exact
}
}  // namespace detail

struct float8_e4m3 {
    std::uint8_t bits = 0;
    float8_e4m3() = default;
    explicit float8_e4m3(float f) : bits(detail::narrow_fp8<3, 7, 0x43F00000u, 0x7Fu>(f)) {}  // >= 480: NaN
    static float8_e4m3 from_bits(std::uint8_t b) {
        float8_e4m3 x;
        x.bits = b;
        return x;
    }
    explicit operator float() const {
        if ((bits & 0x7Fu) == 0x7Fu) return detail::bits_to_float((static_cast<std::uint32_t>(bits & 0x80u) << 24) | 0x7FC00000u);
        return detail::widen_fp8<3, 7>(bits);
    }
};

struct float8_e5m2 {
    std::uint8_t bits = 0;
    float8_e5m2() = default;
    explicit float8_e5m2(float f) : bits(detail::narrow_fp8<2, 15, 0x47800000u, 0x7Cu>(f)) {}  // >= 2^16: inf
    static float8_e5m2 from_bits(std::uint8_t b) {
        float8_e5m2 x;
        x.bits = b;
        return x;
    }
    explicit operator float() const {
        const std::uint32_t sign = static_cast<std::uint32_t>(bits & 0x80u) << 24, m = bits & 0x03u;
        if ((bits & 0x7Cu) == 0x7Cu) return detail::bits_to_float(sign | 0x7F800000u | (m << 21));  // inf, NaN
        return detail::widen_fp8<2, 15>(bits);
    }
};

inline float8_e4m3 operator+(float8_e4m3 a, float8_e4m3 b) { return float8_e4m3(static_cast<float>(a) + static_cast<float>(b)); }
inline float8_e4m3 operator*(float8_e4m3 a, float8_e4m3 b) { return float8_e4m3(static_cast<float>(a) * static_cast<float>(b)); }
inline bool operator<(float8_e4m3 a, float8_e4m3 b) { return static_cast<float>(a) < static_cast<float>(b); }
inline bool operator==(float8_e4m3 a, float8_e4m3 b) { return static_cast<float>(a) == static_cast<float>(b); }
inline float8_e5m2 operator+(float8_e5m2 a, float8_e5m2 b) { return float8_e5m2(static_cast<float>(a) + static_cast<float>(b)); }
inline float8_e5m2 operator*(float8_e5m2 a, float8_e5m2 b) { return float8_e5m2(static_cast<float>(a) * static_cast<float>(b)); }
inline bool operator<(float8_e5m2 a, float8_e5m2 b) { return static_cast<float>(a) < static_cast<float>(b); }
inline bool operator==(float8_e5m2 a, float8_e5m2 b) { return static_cast<float>(a) == static_cast<float>(b); }
static_assert(sizeof(float8_e4m3) == 1 && sizeof(float8_e5m2) == 1 && std::is_trivially_copyable_v<float8_e4m3> &&
                  std::is_trivially_copyable_v<float8_e5m2>,
              "8-bit float elements are their raw bits");

// The scale byte of an MX bucket (OCP E8M0): 2^(bits - 127) for 1..254, 2^-127 for 0, NaN for 255; one per 32 elements
// (reduce_tree_mx below). A byte type with a value, no arithmetic, and a label only: it has no C-ABI dtype, so dtype_of
// answers -1 and no reduction, conversion or fill takes a bucket of it; Bucket stores it (bucket_storage below).
struct float8_e8m0 {
    std::uint8_t bits = 127;  // 1.0
    float8_e8m0() = default;
    static float8_e8m0 from_bits(std::uint8_t b) {
        float8_e8m0 x;
        x.bits = b;
        return x;
    }
    explicit operator float() const {
        const std::uint32_t u = bits == 0 ? 0x00400000u : bits == 255 ? 0x7FC00000u : static_cast<std::uint32_t>(bits) << 23;
        float f;
        std::memcpy(&f, &u, sizeof f);
        return f;
    }
};
inline bool operator==(float8_e8m0 a, float8_e8m0 b) { return a.bits == b.bits; }
static_assert(sizeof(float8_e8m0) == 1 && std::is_trivially_copyable_v<float8_e8m0>, "a scale is its raw byte");

// Two elements of an MXFP4 bucket (OCP E2M1: 1 sign, 2 exponent bits of bias 1, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5,
// 2, 3, 4, 6; no inf, no NaN): element 2k in bits 3:0 of byte k, element 2k + 1 in bits 7:4. A byte type with no
// arithmetic: only the MX calls below take buckets of it (FMI_F4E2M1 is valid nowhere else), with the ELEMENT count given
// explicitly, since a bucket of n elements is (n + 1) / 2 bytes. widen / narrow are the library's definition of a
// nibble's value on the host: narrow rounds to nearest with ties to the even code, keeps the sign, and is defined for
// finite |f| <= 6 (what the scale rule at EMAX = 2 feeds it).
struct float4_e2m1x2 {
    std::uint8_t bits = 0;
    float4_e2m1x2() = default;
    static float4_e2m1x2 from_bits(std::uint8_t b) {
        float4_e2m1x2 x;
        x.bits = b;
        return x;
    }
    static float4_e2m1x2 from_codes(std::uint8_t lo, std::uint8_t hi) { return from_bits(static_cast<std::uint8_t>((lo & 0xF) | (hi << 4))); }
    std::uint8_t lo() const { return bits & 0xF; }
    std::uint8_t hi() const { return bits >> 4; }
    static float widen(std::uint8_t code) {
        static constexpr float mag[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
        return (code & 8) ? -mag[code & 7] : mag[code & 7];
    }
    static std::uint8_t narrow(float f) {
        std::uint32_t u;
        std::memcpy(&u, &f, sizeof u);
        const std::uint32_t a = u & 0x7FFFFFFFu;
        // the seven midpoints as float bits: one whose lower neighbour has the even code stays below (>), the others go up
        const unsigned c = (a > 0x3E800000u) + (a >= 0x3F400000u) + (a > 0x3FA00000u) + (a >= 0x3FE00000u) + (a > 0x40200000u) +
                           (a >= 0x40600000u) + (a > 0x40A00000u);
        return static_cast<std::uint8_t>(c | ((u >> 28) & 8u));
    }
};
inline bool operator==(float4_e2m1x2 a, float4_e2m1x2 b) { return a.bits == b.bits; }
static_assert(sizeof(float4_e2m1x2) == 1 && std::is_trivially_copyable_v<float4_e2m1x2>, "two E2M1 elements are one raw byte");
// The bytes of an MXFP4 bucket of n elements.
inline std::size_t fp4_bytes(std::size_t n) { return (n + 1) / 2; }

// One byte of an MXFP6 bucket (OCP FP6, six bits per element: bit 5 the sign, no inf, no NaN; the bucket is a
// little-endian bit string with element i in bits 6 i .. 6 i + 5, so four elements are three bytes and n elements
// fp6_bytes(n)). Tag types with no arithmetic: only the MX calls below take buckets of them (FMI_F6E2M3 / FMI_F6E3M2 are
// valid nowhere else), with the ELEMENT count given explicitly. widen / narrow are the library's definition of a code's
// value on the host: narrow rounds to nearest with ties to the even code, keeps the sign, and is defined for finite |f|
// at most the largest element (7.5 for E2M3, 28 for E3M2).
namespace detail {
template <int M>  // mantissa bits: 3 is E2M3 (bias 1), 2 is E3M2 (bias 3)
struct fp6_code {
    static constexpr int emin = M == 3 ? 0 : -2;
    static float widen(std::uint8_t code) {
        const int e = (code & 31) >> M, m = code & ((1 << M) - 1);
        const float v = e == 0 ? std::ldexp(static_cast<float>(m), emin - M) : std::ldexp(static_cast<float>((1 << M) + m), e - 1 + emin - M);
        return (code & 32) ? -v : v;
    }
    static std::uint8_t narrow(float f) {
        const float a = std::fabs(f);
        int e = 0;
        std::frexp(a, &e);  // a = x * 2^e, 0.5 <= x < 1: the exponent of |f| is e - 1
        const int ex = a == 0.0f || e - 1 < emin ? emin : e - 1;
        const float t = std::ldexp(a, M - ex);  // |f| in grid steps: exact
        const float k = std::floor(t), frac = t - k;
        const unsigned ki = static_cast<unsigned>(k);
        const unsigned up = frac > 0.5f || (frac == 0.5f && (ki & 1u));
        return static_cast<std::uint8_t>((static_cast<unsigned>(ex - emin) << M) + ki + up + (std::signbit(f) ? 32u : 0u));
    }
};
}  // namespace detail
struct float6_e2m3_packed : detail::fp6_code<3> {
    std::uint8_t bits = 0;
};
struct float6_e3m2_packed : detail::fp6_code<2> {
    std::uint8_t bits = 0;
};
inline bool operator==(float6_e2m3_packed a, float6_e2m3_packed b) { return a.bits == b.bits; }
inline bool operator==(float6_e3m2_packed a, float6_e3m2_packed b) { return a.bits == b.bits; }
static_assert(sizeof(float6_e2m3_packed) == 1 && sizeof(float6_e3m2_packed) == 1 && std::is_trivially_copyable_v<float6_e2m3_packed> &&
                  std::is_trivially_copyable_v<float6_e3m2_packed>,
              "a packed FP6 byte is one raw byte");
template <class A>
inline constexpr bool fp6_packed_v = std::is_same_v<A, float6_e2m3_packed> || std::is_same_v<A, float6_e3m2_packed>;
template <class A>
constexpr int fp6_dtype() {
    static_assert(fp6_packed_v<A>, "Dev::float6_e2m3_packed or Dev::float6_e3m2_packed");
    return std::is_same_v<A, float6_e2m3_packed> ? FMI_F6E2M3 : FMI_F6E3M2;
}
// The bytes of an MXFP6 bucket of n elements.
inline std::size_t fp6_bytes(std::size_t n) { return n / 4 * 3 + (n % 4 * 3 + 3) / 4; }
// Codes (one per element, 0..63) into the bucket's bytes and back; the last byte's unused high bits are written 0.
template <class A>
inline std::vector<A> fp6_pack(const std::vector<std::uint8_t>& codes) {
    static_assert(fp6_packed_v<A>, "fp6_pack: Dev::float6_e2m3_packed or Dev::float6_e3m2_packed bytes");
    std::vector<A> out(fp6_bytes(codes.size()));
    for (std::size_t i = 0; i < codes.size(); ++i) {
        const unsigned v = static_cast<unsigned>(codes[i] & 63u) << (6 * i % 8);
        out[6 * i / 8].bits = static_cast<std::uint8_t>(out[6 * i / 8].bits | v);
        if (v >> 8) out[6 * i / 8 + 1].bits = static_cast<std::uint8_t>(out[6 * i / 8 + 1].bits | (v >> 8));
    }
    return out;
}
template <class A>
inline std::vector<std::uint8_t> fp6_unpack(const std::vector<A>& packed, std::size_t n) {
    static_assert(fp6_packed_v<A>, "fp6_unpack: Dev::float6_e2m3_packed or Dev::float6_e3m2_packed bytes");
    if (packed.size() != fp6_bytes(n)) throw std::runtime_error("Dev::fp6_unpack: n elements are fp6_bytes(n) bytes");
    std::vector<std::uint8_t> codes(n);
    for (std::size_t i = 0; i < n; ++i) {
        unsigned w = packed[6 * i / 8].bits;
        if (6 * i % 8 > 2) w |= static_cast<unsigned>(packed[6 * i / 8 + 1].bits) << 8;
        codes[i] = static_cast<std::uint8_t>((w >> (6 * i % 8)) & 63u);
    }
    return codes;
}

// The float element types narrower than float: their values are held and scaled (the mean) in float.
template <class A>
inline constexpr bool narrow_float_v = std::is_same_v<A, half> || std::is_same_v<A, bfloat16> ||
                                       std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2>;

// The C-ABI element type of a fundamental A (any integer type by width and signedness, so long long and
// char map too) or of Dev::half / Dev::bfloat16 / Dev::float8_e4m3 / Dev::float8_e5m2, or -1: bool, long double and
// other types stay on the host.
template <class A>
constexpr int dtype_of() {
    if constexpr (std::is_same_v<A, float>) return FMI_F32;
    else if constexpr (std::is_same_v<A, double>) return FMI_F64;
    else if constexpr (std::is_same_v<A, half>) return FMI_F16;
    else if constexpr (std::is_same_v<A, bfloat16>) return FMI_BF16;
    else if constexpr (std::is_same_v<A, float8_e4m3>) return FMI_F8E4M3;
    else if constexpr (std::is_same_v<A, float8_e5m2>) return FMI_F8E5M2;
    else if constexpr (std::is_integral_v<A> && !std::is_same_v<A, bool>) {
        constexpr bool s = std::is_signed_v<A>;
        switch (sizeof(A)) {
            case 1: return s ? FMI_I8 : FMI_U8;
            case 2: return s ? FMI_I16 : FMI_U16;
            case 4: return s ? FMI_I32 : FMI_U32;
            case 8: return s ? FMI_I64 : FMI_U64;
            default: return -1;
        }
    } else {
        return -1;
    }
}

template <class A>
constexpr bool device_type = dtype_of<A>() >= 0;
// What a Bucket can hold: the device element types, and the scale bytes of MX buckets and the packed bytes of MXFP4
// buckets, which only the MX calls take.
template <class A>
constexpr bool bucket_storage = device_type<A> || std::is_same_v<A, float8_e8m0> || std::is_same_v<A, float4_e2m1x2> || fp6_packed_v<A>;

// Select the device for this process (one process per GPU, as FMI runs one peer per process).
inline void init(int device = 0) { check(fmi_dev_init(device), "fmi_dev_init"); }

inline bool available() {
    int n = 0;
    return fmi_dev_count(&n) == FMI_OK && n > 0;
}

inline void sync() { check(fmi_dev_sync(), "fmi_dev_sync"); }

// A device-resident bucket of n elements of A (owning, move-only).
template <class A>
class Bucket {
    static_assert(bucket_storage<A>, "device buckets hold float, double, Dev::half, Dev::bfloat16, Dev::float8_e4m3, Dev::float8_e5m2, 8/16/32/64-bit integers, Dev::float8_e8m0 scale bytes or Dev::float4_e2m1x2 bytes");

public:
    using value_type = A;
    Bucket() = default;
    explicit Bucket(std::size_t n) : n_(n) {
        void* p = nullptr;
        check(fmi_dev_alloc(&p, n * sizeof(A)), "fmi_dev_alloc");
        ptr_ = static_cast<A*>(p);
    }
    explicit Bucket(const std::vector<A>& host) : Bucket(host.size()) { upload(host); }
    //! `count` buckets of n elements that one kernel streams together (a peer set's inputs and outputs): bucket j
    //! in 4 KiB slot j mod 16 whatever was allocated before (fmi_dev_alloc_group).
    static std::vector<Bucket> group(std::size_t count, std::size_t n) {
        if (count > static_cast<std::size_t>(std::numeric_limits<int>::max()))
            throw std::runtime_error("Bucket::group: too many buckets");
        std::vector<void*> ptrs(count);
        check(fmi_dev_alloc_group(ptrs.data(), static_cast<int>(count), n * sizeof(A)), "fmi_dev_alloc_group");
        std::vector<Bucket> out(count);
        for (std::size_t j = 0; j < count; ++j) {
            out[j].ptr_ = static_cast<A*>(ptrs[j]);
            out[j].n_ = n;
        }
        return out;
    }
    //! A bucket over memory owned elsewhere (e.g. a communicator window): never freed by the bucket.
    static Bucket borrow(A* ptr, std::size_t n) {
        Bucket b;
        b.ptr_ = ptr;
        b.n_ = n;
        b.owns_ = false;
        return b;
    }
    Bucket(const Bucket&) = delete;
    Bucket& operator=(const Bucket&) = delete;
    Bucket(Bucket&& o) noexcept
        : ptr_(std::exchange(o.ptr_, nullptr)), n_(std::exchange(o.n_, 0)), owns_(std::exchange(o.owns_, true)) {}
    Bucket& operator=(Bucket&& o) noexcept {
        if (this != &o) {
            release();
            ptr_ = std::exchange(o.ptr_, nullptr);
            n_ = std::exchange(o.n_, 0);
            owns_ = std::exchange(o.owns_, true);
        }
        return *this;
    }
    ~Bucket() { release(); }

    A* data() const { return ptr_; }
    std::size_t size() const { return n_; }
    std::size_t size_in_bytes() const { return n_ * sizeof(A); }

    void upload(const std::vector<A>& host) {
        if (host.size() != n_) throw std::runtime_error("Bucket::upload: size mismatch");
        check(fmi_dev_h2d_async(ptr_, host.data(), size_in_bytes(), nullptr), "fmi_dev_h2d_async");
        check(fmi_stream_sync(nullptr), "fmi_stream_sync");
    }
    std::vector<A> download() const {
        std::vector<A> host(n_);
        check(fmi_dev_d2h_async(host.data(), ptr_, size_in_bytes(), nullptr), "fmi_dev_d2h_async");
        check(fmi_stream_sync(nullptr), "fmi_stream_sync");
        return host;
    }
    void fill_synthetic(uint64_t seed, uint32_t peer) {
        static_assert(device_type<A>, "fill_synthetic: a device element type (scale bytes have no synthetic fill)");
        check(fmi_dev_fill_synthetic(dtype_of<A>(), ptr_, n_, seed, peer, nullptr), "fmi_dev_fill_synthetic");
    }

private:
    void release() noexcept {
        if (ptr_ && owns_) (void)fmi_dev_free(ptr_);
        ptr_ = nullptr;
        n_ = 0;
        owns_ = true;
    }
    A* ptr_ = nullptr;
    std::size_t n_ = 0;
    bool owns_ = true;
};

// dst = src converted element by element (fmi_dev_convert): between float, Dev::half, Dev::bfloat16, Dev::float8_e4m3 and
// Dev::float8_e5m2, the value through float, one rounding in all. How float / bfloat16 data gets into an 8-bit float bucket.
template <class D, class S>
inline void convert(Bucket<D>& dst, const Bucket<S>& src, fmi_stream_t stream = nullptr) {
    static_assert((std::is_same_v<D, float> || narrow_float_v<D>) && (std::is_same_v<S, float> || narrow_float_v<S>),
                  "convert: float, Dev::half, Dev::bfloat16, Dev::float8_e4m3 or Dev::float8_e5m2 elements");
    if (dst.size() != src.size()) throw std::runtime_error("Dev::convert: size mismatch");
    check(fmi_dev_convert(dtype_of<D>(), dst.data(), dtype_of<S>(), src.data(), src.size(), stream), "fmi_dev_convert");
}

// The scaled sum of 8-bit float buckets (fmi_dev_reduce_tree_scaled): every input times its own scale in float, the
// float SUM program of `alg` (FMI_ALG_ALLREDUCE / _REDUCE / _REDUCE_LTR, `rank` as in fmi_dev_reduce_tree), the largest
// |sum| folded into *amax, the sum times *out_scale stored once: into a bucket of the inputs' type (non-saturating
// narrowing) or a Bucket<float>. in_scales holds one scale per input; out_scale and amax (one float each) may be
// nullptr: 1 and "not wanted". All of them live on the device, so a captured graph replays with new scales.
template <class A, class O>
inline void reduce_tree_scaled(int alg, Bucket<O>& out, const std::vector<const Bucket<A>*>& ins, const Bucket<float>& in_scales,
                               const Bucket<float>* out_scale = nullptr, Bucket<float>* amax = nullptr, int rank = 0,
                               fmi_stream_t stream = nullptr) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2>,
                  "reduce_tree_scaled: Dev::float8_e4m3 or Dev::float8_e5m2 inputs");
    static_assert(std::is_same_v<O, A> || std::is_same_v<O, float>, "reduce_tree_scaled: the output is of the inputs' type or float");
    if (ins.empty() || ins.size() > static_cast<std::size_t>(std::numeric_limits<int>::max()))
        throw std::runtime_error("Dev::reduce_tree_scaled: need at least one input bucket");
    std::vector<const void*> ptrs;
    for (const Bucket<A>* b : ins) {
        if (!b || b->size() != out.size()) throw std::runtime_error("Dev::reduce_tree_scaled: size mismatch");
        ptrs.push_back(b->data());
    }
    if (in_scales.size() < ins.size() || (out_scale && out_scale->size() < 1) || (amax && amax->size() < 1))
        throw std::runtime_error("Dev::reduce_tree_scaled: one scale per input, one element for out_scale and amax");
    check(fmi_dev_reduce_tree_scaled(FMI_OP_SUM, dtype_of<A>(), alg, dtype_of<O>(), out.data(), ptrs.data(), in_scales.data(),
                                     out_scale ? out_scale->data() : nullptr, amax ? amax->data() : nullptr,
                                     static_cast<int>(ins.size()), rank, out.size(), stream),
          "fmi_dev_reduce_tree_scaled");
}

// Block-scaled (MX) 8-bit float buckets (fmi_dev_reduce_tree_mx): n elements of Dev::float8_e4m3 / Dev::float8_e5m2 and
// (n + 31) / 32 Dev::float8_e8m0 scale bytes, one per 32 elements.
inline std::size_t mx_blocks(std::size_t n) { return (n + 31) / 32; }

// The sum (FMI_OP_SUM) or mean (FMI_OP_AVG) of MX buckets: every element times its block's scale in float, the float SUM
// program of `alg` (`rank` as in fmi_dev_reduce_tree), then per block of 32 the smallest power-of-two scale that brings
// the block's largest magnitude within the element type, into out_scales, and the scaled sum narrowed into `out`; or,
// into a Bucket<float>, the sum itself and no output scales.
// Stochastic rounding for the MX calls (fmi_dev_reduce_tree_mx_sr, fmi_dev_mx_quantize_sr): `seed` is ONE u64 in device
// memory, read by the kernel (a captured graph replays with whatever it then holds); `first`, a multiple of 32, is the
// stream position of the call's element 0. Passed last to Dev::reduce_tree_mx and Dev::mx_quantize, after the stream.
struct Sr {
    const Bucket<std::uint64_t>& seed;
    std::uint64_t first = 0;
};

namespace detail {
inline const std::uint64_t* sr_seed(const Sr& sr) {
    if (sr.seed.size() != 1) throw std::runtime_error("Dev::Sr: the seed is a bucket of one std::uint64_t");
    return sr.seed.data();
}

template <class A>
inline void reduce_tree_mx(int op, int alg, int out_dtype, void* out, void* out_scales, std::size_t n,
                           const std::vector<const Bucket<A>*>& ins, const std::vector<const Bucket<float8_e8m0>*>& in_scales,
                           int rank, fmi_stream_t stream, const Sr* sr = nullptr) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2>,
                  "reduce_tree_mx: Dev::float8_e4m3 or Dev::float8_e5m2 elements");
    if (ins.empty() || ins.size() > static_cast<std::size_t>(std::numeric_limits<int>::max()) || in_scales.size() != ins.size())
        throw std::runtime_error("Dev::reduce_tree_mx: need at least one input bucket and one scale bucket per input");
    std::vector<const void*> ptrs, sptrs;
    for (std::size_t p = 0; p < ins.size(); ++p) {
        if (!ins[p] || ins[p]->size() != n) throw std::runtime_error("Dev::reduce_tree_mx: size mismatch");
        if (!in_scales[p] || in_scales[p]->size() != mx_blocks(n))
            throw std::runtime_error("Dev::reduce_tree_mx: a scale bucket holds (n + 31) / 32 bytes");
        ptrs.push_back(ins[p]->data());
        sptrs.push_back(in_scales[p]->data());
    }
    if (sr) {
        check(fmi_dev_reduce_tree_mx_sr(op, dtype_of<A>(), alg, out, out_scales, ptrs.data(), sptrs.data(), sr_seed(*sr), sr->first,
                                        static_cast<int>(ins.size()), rank, n, stream),
              "fmi_dev_reduce_tree_mx_sr");
        return;
    }
    check(fmi_dev_reduce_tree_mx(op, dtype_of<A>(), alg, out_dtype, out, out_scales, ptrs.data(), sptrs.data(),
                                 static_cast<int>(ins.size()), rank, n, stream),
          "fmi_dev_reduce_tree_mx");
}
}  // namespace detail

template <class A>
inline void reduce_tree_mx(int op, int alg, Bucket<A>& out, Bucket<float8_e8m0>& out_scales, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    if (out_scales.size() != mx_blocks(out.size())) throw std::runtime_error("Dev::reduce_tree_mx: out_scales holds (n + 31) / 32 bytes");
    detail::reduce_tree_mx(op, alg, dtype_of<A>(), out.data(), out_scales.data(), out.size(), ins, in_scales, rank, stream);
}
template <class A>
inline void reduce_tree_mx(int op, int alg, Bucket<float>& out, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    detail::reduce_tree_mx(op, alg, FMI_F32, out.data(), nullptr, out.size(), ins, in_scales, rank, stream);
}
// With stochastic rounding (the output of the inputs' type: a float output has nothing to round).
template <class A>
inline void reduce_tree_mx(int op, int alg, Bucket<A>& out, Bucket<float8_e8m0>& out_scales, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank, fmi_stream_t stream, const Sr& sr) {
    if (out_scales.size() != mx_blocks(out.size())) throw std::runtime_error("Dev::reduce_tree_mx: out_scales holds (n + 31) / 32 bytes");
    detail::reduce_tree_mx(op, alg, dtype_of<A>(), out.data(), out_scales.data(), out.size(), ins, in_scales, rank, stream, &sr);
}

namespace detail {
// The C-ABI element type and the bucket's bytes for n elements: one byte per 8-bit float, fp6_bytes(n) for the FP6 tags.
template <class A>
constexpr int mx_dtype() {
    if constexpr (fp6_packed_v<A>) return fp6_dtype<A>();
    else return dtype_of<A>();
}
template <class A>
inline std::size_t mx_bytes(std::size_t n) {
    if constexpr (fp6_packed_v<A>) return fp6_bytes(n);
    else return n;
}
}  // namespace detail

// float / Dev::half / Dev::bfloat16 data into an MX bucket and back (fmi_dev_mx_quantize / fmi_dev_mx_dequantize). The
// float side gives n: an MXFP6 bucket (Dev::float6_e2m3_packed / Dev::float6_e3m2_packed) holds fp6_bytes(n) bytes.
template <class A, class S>
inline void mx_quantize(Bucket<A>& out, Bucket<float8_e8m0>& out_scales, const Bucket<S>& src, fmi_stream_t stream = nullptr) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2> || fp6_packed_v<A>,
                  "mx_quantize: Dev::float8_e4m3, Dev::float8_e5m2 or packed FP6 elements");
    static_assert(std::is_same_v<S, float> || std::is_same_v<S, half> || std::is_same_v<S, bfloat16>, "mx_quantize: float, Dev::half or Dev::bfloat16 source");
    if (out.size() != detail::mx_bytes<A>(src.size()) || out_scales.size() != mx_blocks(src.size())) throw std::runtime_error("Dev::mx_quantize: size mismatch");
    check(fmi_dev_mx_quantize(detail::mx_dtype<A>(), out.data(), out_scales.data(), dtype_of<S>(), src.data(), src.size(), stream), "fmi_dev_mx_quantize");
}
template <class A, class S>
inline void mx_quantize(Bucket<A>& out, Bucket<float8_e8m0>& out_scales, const Bucket<S>& src, fmi_stream_t stream, const Sr& sr) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2> || fp6_packed_v<A>,
                  "mx_quantize: Dev::float8_e4m3, Dev::float8_e5m2 or packed FP6 elements");
    static_assert(std::is_same_v<S, float> || std::is_same_v<S, half> || std::is_same_v<S, bfloat16>, "mx_quantize: float, Dev::half or Dev::bfloat16 source");
    if (out.size() != detail::mx_bytes<A>(src.size()) || out_scales.size() != mx_blocks(src.size())) throw std::runtime_error("Dev::mx_quantize: size mismatch");
    check(fmi_dev_mx_quantize_sr(detail::mx_dtype<A>(), out.data(), out_scales.data(), dtype_of<S>(), src.data(), src.size(), detail::sr_seed(sr), sr.first,
                                 stream),
          "fmi_dev_mx_quantize_sr");
}
// The same quantization of float values on the host (fmi_host_mx_quantize_sr; no device): `seed` is the value itself.
template <class A>
inline void mx_quantize_sr_host(std::vector<A>& out, std::vector<float8_e8m0>& out_scales, const std::vector<float>& src, std::uint64_t seed,
                                std::uint64_t first = 0) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2> || std::is_same_v<A, float4_e2m1x2> || fp6_packed_v<A>,
                  "mx_quantize_sr_host: Dev::float8_e4m3, Dev::float8_e5m2, Dev::float4_e2m1x2 or packed FP6 elements");
    constexpr bool fp4 = std::is_same_v<A, float4_e2m1x2>, fp6 = fp6_packed_v<A>;
    out.assign(fp4 ? fp4_bytes(src.size()) : fp6 ? fp6_bytes(src.size()) : src.size(), A{});
    out_scales.assign(mx_blocks(src.size()), float8_e8m0{});
    int dtype = FMI_F4E2M1;
    if constexpr (fp6) dtype = fp6_dtype<A>();
    else if constexpr (!fp4) dtype = dtype_of<A>();
    check(fmi_host_mx_quantize_sr(dtype, out.data(), out_scales.data(), src.data(), src.size(), seed, first), "fmi_host_mx_quantize_sr");
}
template <class D, class A>
inline void mx_dequantize(Bucket<D>& dst, const Bucket<A>& src, const Bucket<float8_e8m0>& src_scales, fmi_stream_t stream = nullptr) {
    static_assert(std::is_same_v<A, float8_e4m3> || std::is_same_v<A, float8_e5m2> || fp6_packed_v<A>,
                  "mx_dequantize: Dev::float8_e4m3, Dev::float8_e5m2 or packed FP6 elements");
    static_assert(std::is_same_v<D, float> || std::is_same_v<D, half> || std::is_same_v<D, bfloat16>, "mx_dequantize: float, Dev::half or Dev::bfloat16 destination");
    if (src.size() != detail::mx_bytes<A>(dst.size()) || src_scales.size() != mx_blocks(dst.size())) throw std::runtime_error("Dev::mx_dequantize: size mismatch");
    check(fmi_dev_mx_dequantize(dtype_of<D>(), dst.data(), detail::mx_dtype<A>(), src.data(), src_scales.data(), dst.size(), stream), "fmi_dev_mx_dequantize");
}

// MXFP4 (fmi_dev_reduce_tree_mx at FMI_F4E2M1): buckets of Dev::float4_e2m1x2 bytes, fp4_bytes(n) of them for n
// ELEMENTS, which every call takes explicitly or from its float side; scale bytes as above, EMAX = 2 in the scale rule.
namespace detail {
inline void reduce_tree_mxfp4(int op, int alg, int out_dtype, void* out, void* out_scales, std::size_t n,
                              const std::vector<const Bucket<float4_e2m1x2>*>& ins,
                              const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank, fmi_stream_t stream,
                              const Sr* sr = nullptr) {
    if (ins.empty() || ins.size() > static_cast<std::size_t>(std::numeric_limits<int>::max()) || in_scales.size() != ins.size())
        throw std::runtime_error("Dev::reduce_tree_mx: need at least one input bucket and one scale bucket per input");
    std::vector<const void*> ptrs, sptrs;
    for (std::size_t p = 0; p < ins.size(); ++p) {
        if (!ins[p] || ins[p]->size() != fp4_bytes(n)) throw std::runtime_error("Dev::reduce_tree_mx: an MXFP4 bucket of n elements holds (n + 1) / 2 bytes");
        if (!in_scales[p] || in_scales[p]->size() != mx_blocks(n))
            throw std::runtime_error("Dev::reduce_tree_mx: a scale bucket holds (n + 31) / 32 bytes");
        ptrs.push_back(ins[p]->data());
        sptrs.push_back(in_scales[p]->data());
    }
    if (sr) {
        check(fmi_dev_reduce_tree_mx_sr(op, FMI_F4E2M1, alg, out, out_scales, ptrs.data(), sptrs.data(), sr_seed(*sr), sr->first,
                                        static_cast<int>(ins.size()), rank, n, stream),
              "fmi_dev_reduce_tree_mx_sr");
        return;
    }
    check(fmi_dev_reduce_tree_mx(op, FMI_F4E2M1, alg, out_dtype, out, out_scales, ptrs.data(), sptrs.data(),
                                 static_cast<int>(ins.size()), rank, n, stream),
          "fmi_dev_reduce_tree_mx");
}
}  // namespace detail

inline void reduce_tree_mx(int op, int alg, Bucket<float4_e2m1x2>& out, Bucket<float8_e8m0>& out_scales, std::size_t n,
                           const std::vector<const Bucket<float4_e2m1x2>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    if (out.size() != fp4_bytes(n) || out_scales.size() != mx_blocks(n))
        throw std::runtime_error("Dev::reduce_tree_mx: out holds (n + 1) / 2 bytes and out_scales (n + 31) / 32");
    detail::reduce_tree_mxfp4(op, alg, FMI_F4E2M1, out.data(), out_scales.data(), n, ins, in_scales, rank, stream);
}
inline void reduce_tree_mx(int op, int alg, Bucket<float4_e2m1x2>& out, Bucket<float8_e8m0>& out_scales, std::size_t n,
                           const std::vector<const Bucket<float4_e2m1x2>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank, fmi_stream_t stream, const Sr& sr) {
    if (out.size() != fp4_bytes(n) || out_scales.size() != mx_blocks(n))
        throw std::runtime_error("Dev::reduce_tree_mx: out holds (n + 1) / 2 bytes and out_scales (n + 31) / 32");
    detail::reduce_tree_mxfp4(op, alg, FMI_F4E2M1, out.data(), out_scales.data(), n, ins, in_scales, rank, stream, &sr);
}
inline void reduce_tree_mx(int op, int alg, Bucket<float>& out, std::size_t n, const std::vector<const Bucket<float4_e2m1x2>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    if (out.size() != n) throw std::runtime_error("Dev::reduce_tree_mx: a float output holds n elements");
    detail::reduce_tree_mxfp4(op, alg, FMI_F32, out.data(), nullptr, n, ins, in_scales, rank, stream);
}
// n is the float side's length.
template <class S>
inline void mx_quantize(Bucket<float4_e2m1x2>& out, Bucket<float8_e8m0>& out_scales, const Bucket<S>& src, fmi_stream_t stream = nullptr) {
    static_assert(std::is_same_v<S, float> || std::is_same_v<S, half> || std::is_same_v<S, bfloat16>, "mx_quantize: float, Dev::half or Dev::bfloat16 source");
    if (out.size() != fp4_bytes(src.size()) || out_scales.size() != mx_blocks(src.size())) throw std::runtime_error("Dev::mx_quantize: size mismatch");
    check(fmi_dev_mx_quantize(FMI_F4E2M1, out.data(), out_scales.data(), dtype_of<S>(), src.data(), src.size(), stream), "fmi_dev_mx_quantize");
}
template <class S>
inline void mx_quantize(Bucket<float4_e2m1x2>& out, Bucket<float8_e8m0>& out_scales, const Bucket<S>& src, fmi_stream_t stream, const Sr& sr) {
    static_assert(std::is_same_v<S, float> || std::is_same_v<S, half> || std::is_same_v<S, bfloat16>, "mx_quantize: float, Dev::half or Dev::bfloat16 source");
    if (out.size() != fp4_bytes(src.size()) || out_scales.size() != mx_blocks(src.size())) throw std::runtime_error("Dev::mx_quantize: size mismatch");
    check(fmi_dev_mx_quantize_sr(FMI_F4E2M1, out.data(), out_scales.data(), dtype_of<S>(), src.data(), src.size(), detail::sr_seed(sr), sr.first,
                                 stream),
          "fmi_dev_mx_quantize_sr");
}
template <class D>
inline void mx_dequantize(Bucket<D>& dst, const Bucket<float4_e2m1x2>& src, const Bucket<float8_e8m0>& src_scales, fmi_stream_t stream = nullptr) {
    static_assert(std::is_same_v<D, float> || std::is_same_v<D, half> || std::is_same_v<D, bfloat16>, "mx_dequantize: float, Dev::half or Dev::bfloat16 destination");
    if (src.size() != fp4_bytes(dst.size()) || src_scales.size() != mx_blocks(dst.size())) throw std::runtime_error("Dev::mx_dequantize: size mismatch");
    check(fmi_dev_mx_dequantize(dtype_of<D>(), dst.data(), FMI_F4E2M1, src.data(), src_scales.data(), dst.size(), stream), "fmi_dev_mx_dequantize");
}

// MXFP6 (fmi_dev_reduce_tree_mx at FMI_F6E2M3 / FMI_F6E3M2): buckets of Dev::float6_e2m3_packed / Dev::float6_e3m2_packed
// bytes, fp6_bytes(n) of them for n ELEMENTS, which every call takes explicitly or from its float side; scale bytes as
// above. A: one of the two tag types.
namespace detail {
template <class A>
inline void reduce_tree_mxfp6(int op, int alg, int out_dtype, void* out, void* out_scales, std::size_t n, const std::vector<const Bucket<A>*>& ins,
                              const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank, fmi_stream_t stream, const Sr* sr = nullptr) {
    if (ins.empty() || ins.size() > static_cast<std::size_t>(std::numeric_limits<int>::max()) || in_scales.size() != ins.size())
        throw std::runtime_error("Dev::reduce_tree_mx: need at least one input bucket and one scale bucket per input");
    std::vector<const void*> ptrs, sptrs;
    for (std::size_t p = 0; p < ins.size(); ++p) {
        if (!ins[p] || ins[p]->size() != fp6_bytes(n)) throw std::runtime_error("Dev::reduce_tree_mx: an MXFP6 bucket of n elements holds fp6_bytes(n) bytes");
        if (!in_scales[p] || in_scales[p]->size() != mx_blocks(n))
            throw std::runtime_error("Dev::reduce_tree_mx: a scale bucket holds (n + 31) / 32 bytes");
        ptrs.push_back(ins[p]->data());
        sptrs.push_back(in_scales[p]->data());
    }
    if (sr) {
        check(fmi_dev_reduce_tree_mx_sr(op, fp6_dtype<A>(), alg, out, out_scales, ptrs.data(), sptrs.data(), sr_seed(*sr), sr->first,
                                        static_cast<int>(ins.size()), rank, n, stream),
              "fmi_dev_reduce_tree_mx_sr");
        return;
    }
    check(fmi_dev_reduce_tree_mx(op, fp6_dtype<A>(), alg, out_dtype, out, out_scales, ptrs.data(), sptrs.data(), static_cast<int>(ins.size()), rank, n,
                                 stream),
          "fmi_dev_reduce_tree_mx");
}
}  // namespace detail

template <class A, std::enable_if_t<fp6_packed_v<A>, int> = 0>
inline void reduce_tree_mx(int op, int alg, Bucket<A>& out, Bucket<float8_e8m0>& out_scales, std::size_t n, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    if (out.size() != fp6_bytes(n) || out_scales.size() != mx_blocks(n))
        throw std::runtime_error("Dev::reduce_tree_mx: out holds fp6_bytes(n) bytes and out_scales (n + 31) / 32");
    detail::reduce_tree_mxfp6<A>(op, alg, fp6_dtype<A>(), out.data(), out_scales.data(), n, ins, in_scales, rank, stream);
}
template <class A, std::enable_if_t<fp6_packed_v<A>, int> = 0>
inline void reduce_tree_mx(int op, int alg, Bucket<A>& out, Bucket<float8_e8m0>& out_scales, std::size_t n, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank, fmi_stream_t stream, const Sr& sr) {
    if (out.size() != fp6_bytes(n) || out_scales.size() != mx_blocks(n))
        throw std::runtime_error("Dev::reduce_tree_mx: out holds fp6_bytes(n) bytes and out_scales (n + 31) / 32");
    detail::reduce_tree_mxfp6<A>(op, alg, fp6_dtype<A>(), out.data(), out_scales.data(), n, ins, in_scales, rank, stream, &sr);
}
template <class A, std::enable_if_t<fp6_packed_v<A>, int> = 0>
inline void reduce_tree_mx(int op, int alg, Bucket<float>& out, std::size_t n, const std::vector<const Bucket<A>*>& ins,
                           const std::vector<const Bucket<float8_e8m0>*>& in_scales, int rank = 0, fmi_stream_t stream = nullptr) {
    if (out.size() != n) throw std::runtime_error("Dev::reduce_tree_mx: a float output holds n elements");
    detail::reduce_tree_mxfp6<A>(op, alg, FMI_F32, out.data(), nullptr, n, ins, in_scales, rank, stream);
}
// mx_quantize, mx_dequantize and mx_quantize_sr_host at the two tag types are the templates above (the float side gives n).

// Untyped device scratch used by the channel algorithms for temporaries of device-resident buckets.
class Scratch {
public:
    Scratch() = default;
    Scratch(std::size_t bytes, bool on_device) : bytes_(bytes), device_(on_device) {
        if (device_) {
            void* p = nullptr;
            check(fmi_dev_alloc(&p, bytes ? bytes : 1), "fmi_dev_alloc (scratch)");
            ptr_ = static_cast<char*>(p);
        } else {
            ptr_ = new char[bytes ? bytes : 1];
        }
    }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    Scratch& operator=(Scratch&& o) noexcept {
        if (this != &o) {
            release();
            ptr_ = std::exchange(o.ptr_, nullptr);
            bytes_ = o.bytes_;
            device_ = o.device_;
        }
        return *this;
    }
    ~Scratch() { release(); }
    char* get() const { return ptr_; }

private:
    void release() noexcept {
        if (!ptr_) return;
        if (device_)
            (void)fmi_dev_free(ptr_);
        else
            delete[] ptr_;
        ptr_ = nullptr;
    }
    char* ptr_ = nullptr;
    std::size_t bytes_ = 0;
    bool device_ = false;
};

// Page-locks an existing host range for its lifetime (fmi_host_register), e.g. the storage of a
// Data<std::vector<A>> recv buffer reused across collectives, so host-bucket combines take the zero-copy
// path. The range must outlive the registration. Move-only.
class HostRegistration {
public:
    HostRegistration() = default;
    HostRegistration(void* ptr, std::size_t bytes) : ptr_(ptr) { check(fmi_host_register(ptr, bytes), "fmi_host_register"); }
    template <class A>
    explicit HostRegistration(std::vector<A>& v) : HostRegistration(v.data(), v.size() * sizeof(A)) {}
    HostRegistration(const HostRegistration&) = delete;
    HostRegistration& operator=(const HostRegistration&) = delete;
    HostRegistration(HostRegistration&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)) {}
    HostRegistration& operator=(HostRegistration&& o) noexcept {
        if (this != &o) {
            release();
            ptr_ = std::exchange(o.ptr_, nullptr);
        }
        return *this;
    }
    ~HostRegistration() { release(); }

private:
    void release() noexcept {
        if (ptr_) (void)fmi_host_unregister(ptr_);
        ptr_ = nullptr;
    }
    void* ptr_ = nullptr;
};

// Byte copy that knows where both sides live (host-host memcpy, device-device D2D, staged otherwise).
inline void copy_bytes(char* dst, bool dst_dev, const char* src, bool src_dev, std::size_t len) {
    if (len == 0 || dst == src) return;
    if (!dst_dev && !src_dev) {
        std::copy(src, src + len, dst);
        return;
    }
    int rc;
    if (dst_dev && src_dev) rc = fmi_dev_d2d_async(dst, src, len, nullptr);
    else if (dst_dev) rc = fmi_dev_h2d_async(dst, src, len, nullptr);
    else rc = fmi_dev_d2h_async(dst, src, len, nullptr);
    check(rc, "device copy");
    check(fmi_stream_sync(nullptr), "fmi_stream_sync");
}

}  // namespace FMI::Dev

#endif
