// Function(Op, Accumulate::f32) on the 16-bit float element types of the C++ FMI surface: the flag travels in
// device_op::dtype as FMI_ACC_F32 for Dev::half / Dev::bfloat16, any other element type throws, and a channel built
// on pairwise combines (Loopback) gives the same bits with it as without: one combine is one rounding.
// Run by tests/test_half_acc_cpu.py and tests/test_gpu_half_acc.py.
//
//   test_half_acc         the CPU side: std::vector<Dev::bfloat16> payloads
//   test_half_acc --gpu   the same on Data<Dev::Bucket<Dev::bfloat16>>
#include <atomic>
#include <cstdint>
#include <cstdio>
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

// Run body(comm, p) for P peers as threads sharing one Loopback mailbox.
template <class Body>
static void with_peers(peer_num P, Body body) {
    auto mailbox = std::make_shared<FMI::Comm::Mailbox>();
    std::vector<std::thread> threads;
    std::vector<std::string> errors(P);
    for (peer_num p = 0; p < P; ++p)
        threads.emplace_back([&, p] {
            try {
                Communicator comm(p, P, "", "half-acc-test");
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

static void flag_is_carried_in_device_op() {
    using VB = std::vector<Dev::bfloat16>;
    CHECK(Function<VB>(Op::sum).accumulate() == Accumulate::storage);
    CHECK(Function<VB>(Op::sum, Accumulate::f32).accumulate() == Accumulate::f32);
    CHECK(Function<VB>(Op::sum, Accumulate::f32).builtin() == Op::sum);
    CHECK(Communicator::device_dtype<Dev::bfloat16>(Function<VB>(Op::sum)) == FMI_BF16);
    CHECK(Communicator::device_dtype<Dev::bfloat16>(Function<VB>(Op::sum, Accumulate::f32)) == (FMI_BF16 | FMI_ACC_F32));
    CHECK(Communicator::device_dtype<Dev::half>(Function<std::vector<Dev::half>>(Op::prod, Accumulate::f32)) ==
          (FMI_F16 | FMI_ACC_F32));
    CHECK(Communicator::device_dtype<Dev::half>(Function<Dev::Bucket<Dev::half>>(Op::max, Accumulate::f32)) ==
          (FMI_F16 | FMI_ACC_F32));
    CHECK(Communicator::device_dtype<float>(Function<std::vector<float>>(Op::sum, Accumulate::storage)) == FMI_F32);
}

static void wrong_element_type_throws() {
    bool threw = false;
    try {
        (void)Communicator::device_dtype<float>(Function<std::vector<float>>(Op::sum, Accumulate::f32));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw);
    // through a collective: the combine's raw function is built before anything is exchanged, on every peer
    std::atomic<int> thrown{0};
    auto mailbox = std::make_shared<FMI::Comm::Mailbox>();
    std::vector<std::thread> threads;
    for (peer_num p = 0; p < 2; ++p)
        threads.emplace_back([&, p] {
            Communicator comm(p, 2, "", "half-acc-test");
            comm.register_channel("Loopback", std::make_shared<FMI::Comm::Loopback>(mailbox, std::chrono::seconds(60)));
            Data<std::vector<int32_t>> a(std::vector<int32_t>{1, 2, 3}), r(3);
            try {
                comm.allreduce(a, r, Function<std::vector<int32_t>>(Op::sum, Accumulate::f32));
            } catch (const std::runtime_error&) {
                ++thrown;
            }
        });
    for (auto& t : threads) t.join();
    CHECK(thrown.load() == 2);
}

// A 3-peer Loopback allreduce with and without Accumulate::f32: bit for bit the same (pairwise combines).
template <class D>
static void loopback_is_unchanged() {
    using B = Dev::bfloat16;
    std::vector<std::vector<uint16_t>> in(3);
    // 1 + 2^-8 + 2^-8 (rounded per combine: 1; in f32: 1 + 2^-7), then values of mixed sign and magnitude
    const uint16_t head[3][2] = {{0x3F80, 0x5300}, {0x3B80, 0xD300}, {0x3B80, 0x3B80}};
    for (int p = 0; p < 3; ++p) {
        in[p] = {head[p][0], head[p][1]};
        for (uint32_t i = 0; i < 2059; ++i)
            in[p].push_back(static_cast<uint16_t>(((i * 2654435761u + p * 40503u) >> 12) & 0xBFFFu));
    }
    const std::size_t n = in[0].size();
    std::vector<std::vector<uint16_t>> plain(3), acc(3), plain_sc(3), acc_sc(3);
    with_peers(3, [&](Communicator& c, peer_num p) {
        for (int flagged = 0; flagged < 2; ++flagged) {
            const Function<D> f = flagged ? Function<D>(Op::sum, Accumulate::f32) : Function<D>(Op::sum);
            Data<D> a(from_bits<B>(in[p])), r(n);
            c.allreduce(a, r, f);
            (flagged ? acc : plain)[p] = to_bits(r.get());
            Data<D> s(from_bits<B>(in[p])), sr(n);
            c.scan(s, sr, f);
            (flagged ? acc_sc : plain_sc)[p] = to_bits(sr.get());
        }
    });
    for (int p = 0; p < 3; ++p) {
        CHECK(plain[p].size() == n && acc[p] == plain[p]);
        CHECK(plain_sc[p].size() == n && acc_sc[p] == plain_sc[p]);
    }
    CHECK(!plain[0].empty() && plain[0][0] == 0x3F80);  // rounded after every combine: (1 + 2^-8) + 2^-8 stays 1
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    try {
        flag_is_carried_in_device_op();
        wrong_element_type_throws();
        if (gpu) {
            Dev::init(0);
            loopback_is_unchanged<Dev::Bucket<Dev::bfloat16>>();
        } else {
            loopback_is_unchanged<std::vector<Dev::bfloat16>>();
        }
    } catch (const std::exception& e) {
        ++g_failures;
        std::fprintf(stderr, "  threw: %s\n", e.what());
    }
    std::fprintf(stderr, "%d failed checks\n", g_failures.load());
    return g_failures.load() == 0 ? 0 : 1;
}
