// Tests of the 8-bit float element types of the C++ FMI surface (FMI::Dev::float8_e4m3, FMI::Dev::float8_e5m2): the
// structs' conversions by the definition in include/fmi_dev.h (non-saturating narrowing), their C-ABI dtypes, the
// operators, Function(Op, Accumulate::f32) and Op::avg on them.
// Run by tests/test_fp8_cpp.py.
//
//   test_fp8                         the host tests
//   test_fp8 --gpu                   the device tests (tests/test_gpu_fp8.py): Dev::convert and one pairwise combine on
//                                    device buckets equal the host types' own arithmetic
//   test_fp8 --narrow IN OUT         IN: raw f32 values; OUT: their e4m3 bytes, then their e5m2 bytes (the Python side
//                                    compares them with tests/_fp8.py::narrow)
//   test_fp8 --widen OUT             OUT: the 256 e4m3 patterns as f32, then the 256 e5m2 patterns
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fmi/fmi.h"

using FMI::Utils::Accumulate;
using FMI::Utils::Function;
using FMI::Utils::Op;
namespace Dev = FMI::Dev;

static int g_failures = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            ++g_failures;                                                                  \
            std::fprintf(stderr, "  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                  \
    } while (0)

static int narrow_file(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<float> x;
    float buf[4096];
    for (size_t k; (k = std::fread(buf, sizeof(float), 4096, f)) > 0;) x.insert(x.end(), buf, buf + k);
    std::fclose(f);
    std::vector<std::uint8_t> y(2 * x.size());
    for (size_t i = 0; i < x.size(); ++i) {
        y[i] = Dev::float8_e4m3(x[i]).bits;
        y[x.size() + i] = Dev::float8_e5m2(x[i]).bits;
    }
    f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(y.data(), 1, y.size(), f) == y.size();
    std::fclose(f);
    return ok ? 0 : 2;
}

static int widen_file(const char* out) {
    std::vector<float> y(512);
    for (int b = 0; b < 256; ++b) {
        y[b] = static_cast<float>(Dev::float8_e4m3::from_bits(static_cast<std::uint8_t>(b)));
        y[256 + b] = static_cast<float>(Dev::float8_e5m2::from_bits(static_cast<std::uint8_t>(b)));
    }
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(y.data(), sizeof(float), y.size(), f) == y.size();
    std::fclose(f);
    return ok ? 0 : 2;
}

template <class A>
static void roundtrip() {
    for (int b = 0; b < 256; ++b) {
        const A x = A::from_bits(static_cast<std::uint8_t>(b));
        const float f = static_cast<float>(x);
        if (std::isnan(f)) {
            CHECK(std::isnan(static_cast<float>(A(f))));
        } else {
            CHECK(A(f).bits == x.bits);  // widening is exact, so narrowing it back is the identity
        }
    }
}

// f32 values across both formats' ranges: ties, overflow thresholds, subnormals, signed zeros.
static std::vector<float> gpu_values() {
    std::vector<float> x = {0.0f, -0.0f, 1.0f, 1.0625f, 1.1875f, 464.0f, 465.0f, 448.0f, -480.0f, 61440.0f, 61439.9f,
                            57344.0f, -65536.0f, 0x1p-9f, 0x1p-10f, 0x1.8p-9f, 0x1p-16f, 0x1p-17f, 3.0e-5f, -2.5e-3f};
    for (int i = 0; i < 4099 - 20; ++i) x.push_back(static_cast<float>((i * 2654435761u) >> 8) * 0x1p-16f - 128.0f);
    return x;
}

template <class A>
static void gpu_checks() {
    const std::vector<float> x = gpu_values();
    Dev::Bucket<float> src(x);
    Dev::Bucket<A> dst(x.size());
    Dev::convert(dst, src);
    Dev::sync();
    const std::vector<A> got = dst.download();
    size_t bad = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        const A want(x[i]);
        const bool both_nan = std::isnan(static_cast<float>(got[i])) && std::isnan(static_cast<float>(want));
        bad += !(got[i].bits == want.bits || both_nan);
    }
    CHECK(bad == 0);
    // back to float: exact
    Dev::Bucket<float> wide(x.size());
    Dev::convert(wide, dst);
    Dev::sync();
    const std::vector<float> w = wide.download();
    bad = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        const float f = static_cast<float>(got[i]);
        bad += !(std::memcmp(&w[i], &f, 4) == 0 || (std::isnan(w[i]) && std::isnan(f)));
    }
    CHECK(bad == 0);
    // one pairwise combine on the device equals operator+ on the host
    std::vector<A> b(got.rbegin(), got.rend());
    Dev::Bucket<A> db(b);
    FMI::Dev::check(fmi_dev_reduce_pair(FMI_OP_SUM, Dev::dtype_of<A>(), dst.data(), db.data(), x.size(), nullptr), "fmi_dev_reduce_pair");
    Dev::sync();
    const std::vector<A> sum = dst.download();
    bad = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        const A want = got[i] + b[i];
        const bool both_nan = std::isnan(static_cast<float>(sum[i])) && std::isnan(static_cast<float>(want));
        bad += !(sum[i].bits == want.bits || both_nan);
    }
    CHECK(bad == 0);
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--gpu") {
        Dev::init(0);
        gpu_checks<Dev::float8_e4m3>();
        gpu_checks<Dev::float8_e5m2>();
        std::fprintf(stderr, "%d failed checks\n", g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc == 4 && std::string(argv[1]) == "--narrow") return narrow_file(argv[2], argv[3]);
    if (argc == 3 && std::string(argv[1]) == "--widen") return widen_file(argv[2]);

    static_assert(Dev::dtype_of<Dev::float8_e4m3>() == FMI_F8E4M3 && Dev::dtype_of<Dev::float8_e5m2>() == FMI_F8E5M2);
    static_assert(Dev::device_type<Dev::float8_e4m3> && Dev::device_type<Dev::float8_e5m2>);
    static_assert(Dev::dtype_of<std::uint8_t>() == FMI_U8, "uint8_t keeps meaning FMI_U8");
    static_assert(!std::is_convertible_v<float, Dev::float8_e4m3> && !std::is_convertible_v<float, Dev::float8_e5m2>,
                  "construction from float is explicit");

    roundtrip<Dev::float8_e4m3>();
    roundtrip<Dev::float8_e5m2>();

    // the values the definition names (include/fmi_dev.h)
    CHECK(Dev::float8_e4m3(464.0f).bits == 0x7E);  // tie to even: 448
    CHECK(Dev::float8_e4m3(465.0f).bits == 0x7F);  // NaN, not 448
    CHECK(Dev::float8_e4m3(-1e9f).bits == 0xFF);
    CHECK(Dev::float8_e4m3(INFINITY).bits == 0x7F);
    CHECK(Dev::float8_e5m2(61440.0f).bits == 0x7C);  // tie to even: inf
    CHECK(Dev::float8_e5m2(61439.9f).bits == 0x7B);
    CHECK(Dev::float8_e5m2(-INFINITY).bits == 0xFC);
    CHECK(Dev::float8_e4m3(-0.0f).bits == 0x80 && Dev::float8_e5m2(-0.0f).bits == 0x80);
    CHECK(Dev::float8_e4m3(0x1p-9f).bits == 0x01 && Dev::float8_e4m3(0x1p-10f).bits == 0x00);  // tie at half the smallest subnormal
    CHECK(Dev::float8_e4m3(0x1.8p-9f).bits == 0x02);  // 1.5 subnormal units: tie to even
    CHECK(Dev::float8_e5m2(0x1p-16f).bits == 0x01 && Dev::float8_e5m2(0x1p-17f).bits == 0x00);
    CHECK(std::isnan(static_cast<float>(Dev::float8_e4m3(NAN))) && std::isnan(static_cast<float>(Dev::float8_e5m2(NAN))));

    // operators: one combine = widen, op in float, narrow; max / min by `<` keep an operand's byte
    const Dev::float8_e4m3 a(1.0f), b(0.125f), big(448.0f);
    CHECK((a + b).bits == Dev::float8_e4m3(1.125f).bits);
    CHECK((a + Dev::float8_e4m3(0.0625f)).bits == a.bits);                       // 1.0625: tie to even
    CHECK(std::isnan(static_cast<float>(big + big)));                            // overflow shows: NaN, not 448
    CHECK(std::isinf(static_cast<float>(Dev::float8_e5m2(57344.0f) * Dev::float8_e5m2(2.0f))));
    CHECK(b < a && !(a < b) && a == Dev::float8_e4m3(1.0f));
    CHECK(Dev::float8_e4m3(0.0f) == Dev::float8_e4m3(-0.0f));
    CHECK(std::max(Dev::float8_e4m3(0.0f), Dev::float8_e4m3(-0.0f)).bits == 0x00);  // (a < b) ? b : a keeps a

    // Function: Accumulate::f32 and Op::avg are valid on both
    {
        Function<std::vector<Dev::float8_e4m3>> f(Op::sum, Accumulate::f32);
        CHECK(f.accumulate() == Accumulate::f32);
        CHECK((FMI::Communicator::device_dtype<Dev::float8_e4m3>(f)) == (FMI_F8E4M3 | FMI_ACC_F32));
        Function<std::vector<Dev::float8_e5m2>> g(Op::prod, Accumulate::f32);
        CHECK((FMI::Communicator::device_dtype<Dev::float8_e5m2>(g)) == (FMI_F8E5M2 | FMI_ACC_F32));
        Function<std::vector<Dev::float8_e5m2>> h(Op::sum);
        CHECK((FMI::Communicator::device_dtype<Dev::float8_e5m2>(h)) == FMI_F8E5M2);
        bool threw = false;
        try {
            Function<std::vector<std::uint8_t>> u(Op::sum, Accumulate::f32);
            (void)FMI::Communicator::device_dtype<std::uint8_t>(u);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
        Function<std::vector<Dev::float8_e4m3>> avg(Op::avg);  // would throw on an integer element type
        CHECK(avg.builtin() == Op::avg);
    }

    std::fprintf(stderr, "%d failed checks\n", g_failures);
    return g_failures ? 1 : 0;
}
