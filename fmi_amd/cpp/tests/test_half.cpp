// Tests of the 16-bit float element types of the C++ FMI surface (FMI::Dev::half, FMI::Dev::bfloat16): the
// structs' conversions, their C-ABI dtypes, and 3-peer collectives over the Loopback channel on host buckets
// (known answers from the definition in include/fmi_dev.h) and on device buckets (equal to the host path).
// Run by tests/test_half_cpu.py and tests/test_gpu_half.py.
//
//   test_half            the host tests
//   test_half --gpu      the device tests
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "fmi/fmi.h"

using FMI::Communicator;
using FMI::Comm::Data;
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

// Run body(comm, p) for P peers as threads sharing one Loopback mailbox.
template <class Body>
static void with_peers(peer_num P, Body body) {
    auto mailbox = std::make_shared<FMI::Comm::Mailbox>();
    std::vector<std::thread> threads;
    std::vector<std::string> errors(P);
    for (peer_num p = 0; p < P; ++p)
        threads.emplace_back([&, p] {
            try {
                Communicator comm(p, P, "", "half-test");
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

template <class A>
static std::vector<A> from_bits(const std::vector<uint16_t>& bits) {
    std::vector<A> v;
    for (uint16_t b : bits) v.push_back(A::from_bits(b));
    return v;
}
template <class A>
static std::vector<uint16_t> to_bits(const std::vector<A>& v) {
    std::vector<uint16_t> bits;
    for (const A& x : v) bits.push_back(x.bits);
    return bits;
}

static void dtypes_and_layout() {
    static_assert(Dev::dtype_of<Dev::half>() == FMI_F16 && Dev::dtype_of<Dev::bfloat16>() == FMI_BF16, "dtype_of");
    static_assert(Dev::dtype_of<uint16_t>() == FMI_U16 && Dev::dtype_of<int16_t>() == FMI_I16, "integers keep theirs");
    static_assert(Dev::device_type<Dev::half> && Dev::device_type<Dev::bfloat16>, "device types");
    CHECK(FMI_F16 == 10 && FMI_BF16 == 11);
    CHECK(fmi_abi_version() == 1);
}

static void bfloat16_round_trips() {
    using B = Dev::bfloat16;
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(B(1.0f).bits == 0x3F80 && static_cast<float>(B::from_bits(0x3F80)) == 1.0f);
    // ties to even, both ways: 1 + 2^-8 is halfway between 1 and 1 + 2^-7; 1 + 3 * 2^-8 between 1 + 2^-7 and 1 + 2^-6
    CHECK(B(1.0f + 0x1p-8f).bits == 0x3F80);
    CHECK(B(1.0f + 0x3p-8f).bits == 0x3F82);
    CHECK(B(1.0f + 0x1p-8f + 0x1p-20f).bits == 0x3F81);  // just above the tie
    CHECK(B(0x1.FFp127f).bits == 0x7F80);                 // rounds past the largest finite value
    CHECK(B(0x1.FEp127f).bits == 0x7F7F && B(inf).bits == 0x7F80 && B(-inf).bits == 0xFF80);
    CHECK(std::isnan(static_cast<float>(B(std::nanf("")))) && (B(std::nanf("")).bits & 0x7FC0) == 0x7FC0);
    // a signalling NaN whose payload sits in the dropped bits stays a NaN
    float snan;
    const uint32_t snan_bits = 0x7F800001u;
    std::memcpy(&snan, &snan_bits, 4);
    CHECK((B(snan).bits & 0x7FFF) > 0x7F80);
    CHECK(B(0x1p-133f).bits == 0x0001 && static_cast<float>(B::from_bits(0x0001)) == 0x1p-133f);  // smallest subnormal
    CHECK(B(0x1p-134f).bits == 0x0000 && B(0x3p-135f).bits == 0x0001);  // a tie to even (0), above the tie
    CHECK(B(-0.0f).bits == 0x8000 && B(0.0f).bits == 0x0000);
    for (uint32_t b = 0; b < 0x10000; ++b) {  // every pattern survives the round trip (NaNs: quieted)
        const B x = B::from_bits(static_cast<uint16_t>(b));
        const B y(static_cast<float>(x));
        if (std::isnan(static_cast<float>(x)))
            CHECK((y.bits | 0x0040) == (x.bits | 0x0040));
        else
            CHECK(y.bits == x.bits);
    }
}

static void half_round_trips() {
    using H = Dev::half;
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(H(1.0f).bits == 0x3C00 && static_cast<float>(H::from_bits(0x3C00)) == 1.0f);
    CHECK(H(1.0f + 0x1p-11f).bits == 0x3C00);  // ties to even, both ways
    CHECK(H(1.0f + 0x3p-11f).bits == 0x3C02);
    CHECK(H(1.0f + 0x1p-11f + 0x1p-20f).bits == 0x3C01);
    CHECK(H(65504.0f).bits == 0x7BFF && H(65519.0f).bits == 0x7BFF);  // below the tie to infinity
    CHECK(H(65520.0f).bits == 0x7C00 && H(1e10f).bits == 0x7C00 && H(-1e10f).bits == 0xFC00);
    CHECK(H(inf).bits == 0x7C00 && H(-inf).bits == 0xFC00);
    CHECK(std::isnan(static_cast<float>(H(std::nanf("")))) && (H(std::nanf("")).bits & 0x7E00) == 0x7E00);
    CHECK(H(0x1p-24f).bits == 0x0001 && static_cast<float>(H::from_bits(0x0001)) == 0x1p-24f);  // smallest subnormal
    CHECK(H(0x1p-25f).bits == 0x0000 && H(0x3p-26f).bits == 0x0001);  // a tie to even (0), above the tie
    CHECK(H(0x3p-25f).bits == 0x0002);                                // 1.5 units: a tie to even (2)
    CHECK(H(0x1p-14f).bits == 0x0400 && H(0x1.FFCp-15f).bits == 0x0400);  // subnormal rounding up into the normals
    CHECK(H(0x1p-16f).bits == 0x0100 && static_cast<float>(H::from_bits(0x0100)) == 0x1p-16f);
    CHECK(H(-0.0f).bits == 0x8000);
    for (uint32_t b = 0; b < 0x10000; ++b) {
        const H x = H::from_bits(static_cast<uint16_t>(b));
        const H y(static_cast<float>(x));
        if (std::isnan(static_cast<float>(x)))
            CHECK((y.bits | 0x0200) == (x.bits | 0x0200));
        else
            CHECK(y.bits == x.bits);
    }
    // operators go through the widened form
    CHECK((H::from_bits(0x3C00) + H::from_bits(0x1000)).bits == 0x3C00);                 // 1 + 2^-11: tie to even
    CHECK((H::from_bits(0x0C00) * H::from_bits(0x0C00)).bits == 0x0001);                 // 2^-12 squared: subnormal
    CHECK((Dev::bfloat16::from_bits(0x1F80) * Dev::bfloat16::from_bits(0x1F80)).bits == 0x0020);  // 2^-64 squared
    CHECK(std::max(H::from_bits(0x0000), H::from_bits(0x8000)).bits == 0x0000);          // (a < b) ? b : a keeps a
    CHECK(std::max(H::from_bits(0x8000), H::from_bits(0x0000)).bits == 0x8000);
    CHECK(H::from_bits(0x8000) == H::from_bits(0x0000));  // == on values
}

// Three peers' bf16 buckets (bit patterns) and every peer's expected result, written out from the definition:
// each combine is widen to f32, op, round to nearest even; the order is the reference's allreduce_no_order /
// scan_no_order for 3 peers. Columns: a double rounding tie, ties both ways, ±0 on different peers, overflow of
// max + max, and 2^-64 * ... kept for the sum of tiny values.
static const std::vector<std::vector<uint16_t>> kIn = {{0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x1F80},
                                                       {0x3B80, 0x3B80, 0x8000, 0x7F7F, 0x1F80},
                                                       {0x3B80, 0x3C40, 0x0000, 0x0001, 0x3F80}};
static const std::vector<std::vector<uint16_t>> kSumAllreduce = {{0x3F80, 0x3F82, 0x0000, 0x7F80, 0x3F80},
                                                                 {0x3F80, 0x3F82, 0x0000, 0x7F80, 0x3F80},
                                                                 {0x3F80, 0x3F82, 0x0000, 0x7F80, 0x3F80}};
static const std::vector<std::vector<uint16_t>> kSumScan = {{0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x1F80},
                                                            {0x3F80, 0x3F82, 0x0000, 0x7F80, 0x2000},
                                                            {0x3F80, 0x3F84, 0x0000, 0x7F80, 0x3F80}};
static const std::vector<std::vector<uint16_t>> kMaxAllreduce = {{0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x3F80},
                                                                 {0x3F80, 0x3F81, 0x8000, 0x7F7F, 0x3F80},
                                                                 {0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x3F80}};
static const std::vector<std::vector<uint16_t>> kMaxScan = {{0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x1F80},
                                                            {0x3F80, 0x3F81, 0x8000, 0x7F7F, 0x1F80},
                                                            {0x3F80, 0x3F81, 0x0000, 0x7F7F, 0x3F80}};

struct Results {
    std::vector<std::vector<uint16_t>> sum_ar{3}, sum_sc{3}, max_ar{3}, max_sc{3};
};

// The four collectives on payload D = std::vector<bfloat16> (host combine) or Dev::Bucket<bfloat16> (kernels).
template <class D>
static Results run_collectives(const std::vector<std::vector<uint16_t>>& in) {
    using B = Dev::bfloat16;
    Results res;
    const std::size_t n = in[0].size();
    with_peers(3, [&](Communicator& c, peer_num p) {
        for (Op op : {Op::sum, Op::max}) {
            Data<D> a(from_bits<B>(in[p])), r(n);
            c.allreduce(a, r, Function<D>(op));
            (op == Op::sum ? res.sum_ar : res.max_ar)[p] = to_bits(r.get());
            Data<D> s(from_bits<B>(in[p])), sr(n);
            c.scan(s, sr, Function<D>(op));
            (op == Op::sum ? res.sum_sc : res.max_sc)[p] = to_bits(sr.get());
        }
    });
    return res;
}

static void host_collectives_known_answers() {
    const Results r = run_collectives<std::vector<Dev::bfloat16>>(kIn);
    for (int p = 0; p < 3; ++p) {
        CHECK(r.sum_ar[p] == kSumAllreduce[p]);
        CHECK(r.sum_sc[p] == kSumScan[p]);
        CHECK(r.max_ar[p] == kMaxAllreduce[p]);
        CHECK(r.max_sc[p] == kMaxScan[p]);
    }
    // Dev::half host buckets through the same path: 1 + 2^-11 + 2^-11 rounds after every combine
    std::vector<std::vector<uint16_t>> got(3);
    with_peers(3, [&](Communicator& c, peer_num p) {
        using V = std::vector<Dev::half>;
        Data<V> a(from_bits<Dev::half>({static_cast<uint16_t>(p == 0 ? 0x3C00 : 0x1000)})), r(1);
        c.allreduce(a, r, Function<V>(Op::sum));
        got[p] = to_bits(r.get());
    });
    // peers 0, 1 double first (peer 2 folds into 0 before): ((1 + 2^-11) + 2^-11) = 1 for every peer
    for (int p = 0; p < 3; ++p) CHECK(got[p] == std::vector<uint16_t>{0x3C00});
}

// Device buckets: every combine is the kernel; equal to this program's own host-path results bit for bit, on
// the known-answer buckets and on longer ones (a vector body, and a sub-vector tail).
static void device_collectives_match_host_path() {
    Dev::init(0);
    std::vector<std::vector<uint16_t>> in(3);
    for (int p = 0; p < 3; ++p) {
        in[p] = kIn[p];
        for (uint32_t i = 0; i < 2061; ++i)  // finite values of mixed sign and magnitude; ±0 on different peers
            in[p].push_back(i % 7 == 0 ? static_cast<uint16_t>(p == 1 ? 0x8000 : 0x0000)
                                       : static_cast<uint16_t>(((i * 2654435761u + p * 40503u) >> 12) & 0xBFFFu));
    }
    const Results host = run_collectives<std::vector<Dev::bfloat16>>(in);
    const Results dev = run_collectives<Dev::Bucket<Dev::bfloat16>>(in);
    for (int p = 0; p < 3; ++p) {
        CHECK(dev.sum_ar[p] == host.sum_ar[p]);
        CHECK(dev.max_sc[p] == host.max_sc[p]);
        CHECK(dev.sum_sc[p] == host.sum_sc[p]);
        CHECK(dev.max_ar[p] == host.max_ar[p]);
    }
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    try {
        if (gpu) {
            device_collectives_match_host_path();
        } else {
            dtypes_and_layout();
            bfloat16_round_trips();
            half_round_trips();
            host_collectives_known_answers();
        }
    } catch (const std::exception& e) {
        ++g_failures;
        std::fprintf(stderr, "  threw: %s\n", e.what());
    }
    std::fprintf(stderr, "%d failed checks\n", g_failures.load());
    return g_failures.load() == 0 ? 0 : 1;
}
