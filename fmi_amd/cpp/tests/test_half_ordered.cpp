// Ordered collectives on the 16-bit float element types of the C++ FMI surface: a Function flagged non-commutative
// selects the reference's reduce_ltr / scan_ltr, and Data<Dev::Bucket<Dev::bfloat16>> must come out of
// FMI::Communicator::allreduce and scan, 3 peers over the Loopback channel, with the bits of this program's own
// host path (std::vector<Dev::bfloat16>, every combine widen to f32, op, round to nearest even).
// Run by tests/test_gpu_half_fused.py.
//
//   test_half_ordered         the host path against known answers
//   test_half_ordered --gpu   device buckets against the host path
#include <atomic>
#include <cstdint>
#include <cstdio>
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
                Communicator comm(p, P, "", "half-ordered-test");
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

struct Results {
    std::vector<std::vector<uint16_t>> sum_ar{3}, sum_sc{3}, max_ar{3}, max_sc{3};
};

// allreduce and scan, sum and max, with a Function that is a built-in op but not commutative: the left-to-right
// forms. Payload D = std::vector<bfloat16> (host combine) or Dev::Bucket<bfloat16> (kernels).
template <class D>
static Results run_ordered(const std::vector<std::vector<uint16_t>>& in) {
    using B = Dev::bfloat16;
    Results res;
    const std::size_t n = in[0].size();
    with_peers(3, [&](Communicator& c, peer_num p) {
        for (Op op : {Op::sum, Op::max}) {
            Function<D> f(op);
            f.commutative = false;
            Data<D> a(from_bits<B>(in[p])), r(n);
            c.allreduce(a, r, f);
            (op == Op::sum ? res.sum_ar : res.max_ar)[p] = to_bits(r.get());
            Data<D> s(from_bits<B>(in[p])), sr(n);
            c.scan(s, sr, f);
            (op == Op::sum ? res.sum_sc : res.max_sc)[p] = to_bits(sr.get());
        }
    });
    return res;
}

// 1 + 2^-8 + 2^-8: left to right each add is a tie to even and stays 1 (the tree order of the unordered form gives
// the same here, the next column does not); 2^-8 + 2^-8 + 1 = 1 + 2^-7 left to right; ±0 on different peers.
static const std::vector<std::vector<uint16_t>> kIn = {{0x3F80, 0x3B80, 0x0000}, {0x3B80, 0x3B80, 0x8000}, {0x3B80, 0x3F80, 0x0000}};
static const std::vector<uint16_t> kSumLtr = {0x3F80, 0x3F81, 0x0000};
static const std::vector<std::vector<uint16_t>> kSumScanLtr = {{0x3F80, 0x3B80, 0x0000}, {0x3F80, 0x3C00, 0x0000}, {0x3F80, 0x3F81, 0x0000}};
static const std::vector<uint16_t> kMaxLtr = {0x3F80, 0x3F80, 0x0000};  // max(+0, -0) keeps the left operand

static void host_ordered_known_answers() {
    const Results r = run_ordered<std::vector<Dev::bfloat16>>(kIn);
    for (int p = 0; p < 3; ++p) {
        CHECK(r.sum_ar[p] == kSumLtr);
        CHECK(r.sum_sc[p] == kSumScanLtr[p]);
        CHECK(r.max_ar[p] == kMaxLtr);
    }
    CHECK(r.max_sc[2] == kMaxLtr);
}

static void device_ordered_matches_host_path() {
    Dev::init(0);
    std::vector<std::vector<uint16_t>> in(3);
    for (int p = 0; p < 3; ++p) {
        in[p] = kIn[p];
        for (uint32_t i = 0; i < 2061; ++i)  // finite values of mixed sign and magnitude; ±0 on different peers
            in[p].push_back(i % 7 == 0 ? static_cast<uint16_t>(p == 1 ? 0x8000 : 0x0000)
                                       : static_cast<uint16_t>(((i * 2654435761u + p * 40503u) >> 12) & 0xBFFFu));
    }
    const Results host = run_ordered<std::vector<Dev::bfloat16>>(in);
    const Results dev = run_ordered<Dev::Bucket<Dev::bfloat16>>(in);
    for (int p = 0; p < 3; ++p) {
        CHECK(dev.sum_ar[p] == host.sum_ar[p]);
        CHECK(dev.sum_sc[p] == host.sum_sc[p]);
        CHECK(dev.max_ar[p] == host.max_ar[p]);
        CHECK(dev.max_sc[p] == host.max_sc[p]);
    }
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::string(argv[1]) == "--gpu";
    try {
        if (gpu)
            device_ordered_matches_host_path();
        else
            host_ordered_known_answers();
    } catch (const std::exception& e) {
        ++g_failures;
        std::fprintf(stderr, "  threw: %s\n", e.what());
    }
    std::fprintf(stderr, "%d failed checks\n", g_failures.load());
    return g_failures.load() == 0 ? 0 : 1;
}
