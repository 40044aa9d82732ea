// Op::avg on the C++ FMI surface: which element types take it, that it has no pairwise meaning (operator() and scan
// throw), and that reduce / allreduce over a channel built on pairwise combines (Loopback) give the sum's value times
// the rounded reciprocal of the peer count: one multiply, in f32 for Dev::bfloat16, rounded to storage once.
// Run by tests/test_avg_cpu.py and tests/test_gpu_avg.py.
//
//   test_avg                 the CPU side: scalars and std::vector payloads
//   test_avg --gpu           the same on Data<Dev::Bucket<A>> (the result finished by fmi_dev_mean_scale)
//   test_avg --dump P n      prints the float bits of a P-peer Loopback allreduce(Op::avg) over std::vector<float>,
//                            one hex word per line (peer 0's result), inputs x_p[i] = input_bits(p, i)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fmi/fmi.h"

using FMI::Communicator;
using FMI::Comm::Data;
using FMI::Utils::Accumulate;
using FMI::Utils::Function;
using FMI::Utils::Op;
using FMI::Utils::peer_num;
namespace Dev = FMI::Dev;

static std::atomic<int> g_failures{0};
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            ++g_failures;                                                                  \
            std::fprintf(stderr, "  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                                  \
    } while (0)

template <class Body>
static void with_peers(peer_num P, Body body) {
    auto mailbox = std::make_shared<FMI::Comm::Mailbox>();
    std::vector<std::thread> threads;
    std::vector<std::string> errors(P);
    for (peer_num p = 0; p < P; ++p)
        threads.emplace_back([&, p] {
            try {
                Communicator comm(p, P, "", "avg-test");
                comm.register_channel("Loopback", std::make_shared<FMI::Comm::Loopback>(mailbox, std::chrono::seconds(60)));
                body(comm, p);
            } catch (const std::exception& e) {
                errors[p] = e.what();
            }
        });
    for (auto& t : threads) t.join();
    for (peer_num p = 0; p < P; ++p)
        if (!errors[p].empty()) {
            ++g_failures;
            std::fprintf(stderr, "  peer %u threw: %s\n", p, errors[p].c_str());
        }
}

template <class F>
static bool throws(F f) {
    try {
        f();
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

// Finite floats of mixed sign over ~40 binades: sign, an exponent in [107, 146], 23 mantissa bits from a hash.
static uint32_t input_bits(unsigned p, uint32_t i) {
    const uint32_t h = (i * 2654435761u) ^ ((p + 1u) * 0x9E3779B9u);
    const uint32_t m = h * 2246822519u;
    return ((m >> 31) << 31) | ((107u + (h >> 8) % 40u) << 23) | (m & 0x007FFFFFu);
}
static float bits_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static std::vector<float> float_input(unsigned p, std::size_t n) {
    std::vector<float> v(n);
    for (std::size_t i = 0; i < n; ++i) v[i] = bits_float(input_bits(p, static_cast<uint32_t>(i)));
    return v;
}
static std::vector<Dev::bfloat16> bf16_input(unsigned p, std::size_t n) {
    std::vector<Dev::bfloat16> v(n);
    for (std::size_t i = 0; i < n; ++i)
        v[i] = Dev::bfloat16::from_bits(static_cast<uint16_t>(input_bits(p, static_cast<uint32_t>(i)) >> 16));
    return v;
}

static void which_types_take_it() {
    CHECK(throws([] { Function<int> f(Op::avg); }));
    CHECK(throws([] { Function<std::vector<int32_t>> f(Op::avg); }));
    CHECK(throws([] { Function<Dev::Bucket<int64_t>> f(Op::avg); }));
    CHECK(!throws([] { Function<double> f(Op::avg); }));
    CHECK(!throws([] { Function<std::vector<float>> f(Op::avg); }));
    CHECK(!throws([] { Function<std::vector<Dev::half>> f(Op::avg); }));
    CHECK(!throws([] { Function<Dev::Bucket<Dev::bfloat16>> f(Op::avg, Accumulate::f32); }));
    CHECK(Function<std::vector<float>>(Op::avg).builtin() == Op::avg);
    CHECK(static_cast<int>(Op::avg) == FMI_OP_AVG && FMI_OP_AVG == 5);
    CHECK(Function<Dev::Bucket<Dev::bfloat16>>(Op::avg, Accumulate::f32).accumulate() == Accumulate::f32);
}

static void no_pairwise_meaning() {
    CHECK(throws([] { (void)Function<double>(Op::avg)(1.0, 2.0); }));
    CHECK(throws([] { (void)Function<std::vector<float>>(Op::avg)({1.f}, {2.f}); }));
    std::atomic<int> thrown{0};
    with_peers(2, [&](Communicator& c, peer_num) {
        Data<std::vector<float>> a(std::vector<float>{1.f, 2.f}), r(2);
        if (throws([&] { c.scan(a, r, Function<std::vector<float>>(Op::avg)); })) ++thrown;
    });
    CHECK(thrown.load() == 2);
}

template <class A>
static bool same_bits(const A& a, const A& b) {
    return std::memcmp(&a, &b, sizeof(A)) == 0;
}

// allreduce and reduce with Op::avg equal the same call with Op::sum finished by one multiply with fl(1 / P).
template <class D, class A, class Make, class Mul>
static void mean_is_the_scaled_sum(peer_num P, std::size_t n, Make make, Mul mul) {
    std::vector<std::vector<A>> avg(P), sum(P), red_avg(P), red_sum(P);
    const peer_num root = P - 1;
    with_peers(P, [&](Communicator& c, peer_num p) {
        {
            Data<D> a(make(p, n)), r(n);
            c.allreduce(a, r, Function<D>(Op::avg));
            avg[p] = r.get();
        }
        {
            Data<D> a(make(p, n)), r(n);
            c.allreduce(a, r, Function<D>(Op::sum));
            sum[p] = r.get();
        }
        {
            Data<D> a(make(p, n)), r(n);
            c.reduce(a, r, root, Function<D>(Op::avg));
            if (p == root) red_avg[p] = r.get();
        }
        {
            Data<D> a(make(p, n)), r(n);
            c.reduce(a, r, root, Function<D>(Op::sum));
            if (p == root) red_sum[p] = r.get();
        }
    });
    for (peer_num p = 0; p < P; ++p) {
        CHECK(avg[p].size() == n && sum[p].size() == n);
        std::size_t bad = 0;
        for (std::size_t i = 0; i < n && i < avg[p].size(); ++i)
            if (!same_bits(avg[p][i], mul(sum[p][i], P))) ++bad;
        CHECK(bad == 0);
    }
    CHECK(red_avg[root].size() == n && red_sum[root].size() == n);
    std::size_t bad = 0;
    for (std::size_t i = 0; i < n && i < red_avg[root].size(); ++i)
        if (!same_bits(red_avg[root][i], mul(red_sum[root][i], P))) ++bad;
    CHECK(bad == 0);
}

static float mul_f32(float s, peer_num P) { return s * (1.0f / static_cast<float>(P)); }
static Dev::bfloat16 mul_bf16(Dev::bfloat16 s, peer_num P) {
    return Dev::bfloat16(static_cast<float>(s) * (1.0f / static_cast<float>(P)));
}

static void scalar_mean() {
    const double x[3] = {0.1, 0.2, 0.7};
    std::vector<double> got(3);
    with_peers(3, [&](Communicator& c, peer_num p) {
        Data<double> a(x[p]), r;
        c.allreduce(a, r, Function<double>(Op::avg));
        got[p] = r.get();
    });
    for (int p = 0; p < 3; ++p) CHECK(got[p] == got[0]);
    // one of the bracketings of the three-peer sum, times fl(1 / 3)
    const double third = 1.0 / 3.0;
    CHECK(got[0] == ((x[0] + x[1]) + x[2]) * third || got[0] == (x[0] + (x[1] + x[2])) * third ||
          got[0] == ((x[0] + x[2]) + x[1]) * third);
}

static int dump(peer_num P, std::size_t n) {
    std::vector<float> out;
    with_peers(P, [&](Communicator& c, peer_num p) {
        Data<std::vector<float>> a(float_input(p, n)), r(n);
        c.allreduce(a, r, Function<std::vector<float>>(Op::avg));
        if (p == 0) out = r.get();
    });
    if (g_failures.load() != 0 || out.size() != n) return 1;
    for (float f : out) std::printf("%08x\n", float_bits(f));
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--dump" && argc == 4)
        return dump(static_cast<peer_num>(std::atoi(argv[2])), static_cast<std::size_t>(std::atoll(argv[3])));
    try {
        which_types_take_it();
        no_pairwise_meaning();
        if (mode == "--gpu") {
            Dev::init(0);
            mean_is_the_scaled_sum<Dev::Bucket<float>, float>(3, 2061, float_input, mul_f32);
            mean_is_the_scaled_sum<Dev::Bucket<Dev::bfloat16>, Dev::bfloat16>(4, 2061, bf16_input, mul_bf16);
        } else {
            scalar_mean();
            mean_is_the_scaled_sum<std::vector<float>, float>(3, 2061, float_input, mul_f32);
            mean_is_the_scaled_sum<std::vector<float>, float>(8, 515, float_input, mul_f32);
            mean_is_the_scaled_sum<std::vector<Dev::bfloat16>, Dev::bfloat16>(3, 2061, bf16_input, mul_bf16);
        }
    } catch (const std::exception& e) {
        ++g_failures;
        std::fprintf(stderr, "  threw: %s\n", e.what());
    }
    std::fprintf(stderr, "%d failed checks\n", g_failures.load());
    return g_failures.load() == 0 ? 0 : 1;
}
