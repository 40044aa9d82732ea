// Stochastic rounding through the C++ surface: Dev::reduce_tree_mx and Dev::mx_quantize with a trailing Dev::Sr, and
// Dev::mx_quantize_sr_host, through files, in the style of test_mxfp4. Run by tests/test_mx_sr_cpp.py (host, checks: no
// device) and tests/test_gpu_mx_sr_cpp.py (reduce, quantize), which compare the outputs with tests/_mx_sr.py.
//
//   KIND  e4m3 | e5m2 | e2m1 (packed: (N + 1) / 2 bytes for N elements);  SEED, FIRST  unsigned 64-bit, decimal
//   test_mx_sr host KIND N SEED FIRST SRC OUT OUT_SCALES            (no device)
//     SRC  N raw f32 values;  OUT, OUT_SCALES written: the MX bucket Dev::mx_quantize_sr_host gives
//   test_mx_sr checks                                               (no device)
//     the argument checks of the Dev::Sr overloads, on borrowed host memory that no call reaches; prints each refusal
//   test_mx_sr reduce KIND OP ALG P N SEED FIRST IN SCALES RESULT RESULT_SCALES
//     OP 0 SUM | 5 AVG;  ALG 0 ALLREDUCE | 1 REDUCE (root 0) | 2 REDUCE_LTR;  IN, SCALES: peer after peer
//   test_mx_sr quantize KIND N SEED FIRST SRC Q Q_SCALES
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fmi/fmi.h"

namespace Dev = FMI::Dev;
using F4 = Dev::float4_e2m1x2;
using E8 = Dev::float8_e8m0;

template <class T>
static std::vector<T> read_file(const char* path, std::size_t count) {
    std::vector<T> v(count);
    std::FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), count, f) != count) {
        std::fprintf(stderr, "cannot read %zu elements from %s\n", count, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

template <class T>
static void write_file(const char* path, const std::vector<T>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::fprintf(stderr, "cannot write %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

template <class A>
static std::size_t bytes_of(std::size_t n) {
    return std::is_same_v<A, F4> ? Dev::fp4_bytes(n) : n;
}

template <class A>
static int host(std::size_t n, std::uint64_t seed, std::uint64_t first, char** a) {
    const std::vector<float> src = read_file<float>(a[0], n);
    std::vector<A> out;
    std::vector<E8> scales;
    Dev::mx_quantize_sr_host(out, scales, src, seed, first);
    if (out.size() != bytes_of<A>(n) || scales.size() != Dev::mx_blocks(n)) return 1;
    write_file(a[1], out);
    write_file(a[2], scales);
    return 0;
}

// One call that must throw; prints what it said.
template <class F>
static bool refused(const char* what, F&& f) {
    try {
        f();
    } catch (const std::exception& e) {
        std::printf("refused %s: %s\n", what, e.what());
        return true;
    }
    std::printf("ACCEPTED %s\n", what);
    return false;
}

static int checks() {
    // host memory behind borrowed buckets: every call below is refused before anything reads it
    std::vector<Dev::float8_e4m3> e(64), eo(64);
    std::vector<F4> q(32), qo(32);
    std::vector<E8> sc(2), so(2);
    std::vector<float> f(64);
    std::vector<std::uint64_t> w(2);
    auto in8 = Dev::Bucket<Dev::float8_e4m3>::borrow(e.data(), 64), out8 = Dev::Bucket<Dev::float8_e4m3>::borrow(eo.data(), 64);
    auto in4 = Dev::Bucket<F4>::borrow(q.data(), 32), out4 = Dev::Bucket<F4>::borrow(qo.data(), 32);
    auto s_in = Dev::Bucket<E8>::borrow(sc.data(), 2), s_out = Dev::Bucket<E8>::borrow(so.data(), 2), s_short = Dev::Bucket<E8>::borrow(so.data(), 1);
    auto src = Dev::Bucket<float>::borrow(f.data(), 64);
    auto seed = Dev::Bucket<std::uint64_t>::borrow(w.data(), 1), two = Dev::Bucket<std::uint64_t>::borrow(w.data(), 2),
         null = Dev::Bucket<std::uint64_t>::borrow(nullptr, 1),
         odd = Dev::Bucket<std::uint64_t>::borrow(reinterpret_cast<std::uint64_t*>(reinterpret_cast<char*>(w.data()) + 4), 1);
    const std::vector<const Dev::Bucket<Dev::float8_e4m3>*> ins8{&in8, &in8};
    const std::vector<const Dev::Bucket<F4>*> ins4{&in4, &in4};
    const std::vector<const Dev::Bucket<E8>*> scs{&s_in, &s_in};
    bool ok = true;
    ok &= refused("a seed bucket of two words", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out8, s_out, ins8, scs, 0, nullptr, Dev::Sr{two, 0}); });
    ok &= refused("a null seed", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out8, s_out, ins8, scs, 0, nullptr, Dev::Sr{null, 0}); });
    ok &= refused("a misaligned seed", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out8, s_out, ins8, scs, 0, nullptr, Dev::Sr{odd, 0}); });
    ok &= refused("first = 16", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out8, s_out, ins8, scs, 0, nullptr, Dev::Sr{seed, 16}); });
    ok &= refused("first + n wraps", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out4, s_out, 64, ins4, scs, 0, nullptr, Dev::Sr{seed, ~std::uint64_t{0} - 31}); });
    ok &= refused("op MAX", [&] { Dev::reduce_tree_mx(FMI_OP_MAX, FMI_ALG_ALLREDUCE, out4, s_out, 64, ins4, scs, 0, nullptr, Dev::Sr{seed, 0}); });
    ok &= refused("short out_scales", [&] { Dev::reduce_tree_mx(FMI_OP_SUM, FMI_ALG_ALLREDUCE, out4, s_short, 64, ins4, scs, 0, nullptr, Dev::Sr{seed, 0}); });
    ok &= refused("quantize, first = 48", [&] { Dev::mx_quantize(out8, s_out, src, nullptr, Dev::Sr{seed, 48}); });
    ok &= refused("quantize, a seed bucket of two words", [&] { Dev::mx_quantize(out4, s_out, src, nullptr, Dev::Sr{two, 0}); });
    ok &= refused("quantize, size mismatch", [&] { Dev::mx_quantize(out8, s_short, src, nullptr, Dev::Sr{seed, 0}); });
    std::vector<F4> ho;
    std::vector<E8> hs;
    ok &= refused("host, first = 8", [&] { Dev::mx_quantize_sr_host(ho, hs, f, 1, 8); });
    Dev::mx_quantize_sr_host(ho, hs, std::vector<float>{}, 1, 0);  // n = 0 succeeds
    ok &= ho.empty() && hs.empty();
    std::printf(ok ? "checks ok\n" : "checks FAILED\n");
    return ok ? 0 : 1;
}

template <class A>
static int reduce(int op, int alg, int P, std::size_t n, std::uint64_t seed, std::uint64_t first, char** a) {
    const std::size_t nbytes = bytes_of<A>(n), nb = Dev::mx_blocks(n);
    const std::vector<A> in = read_file<A>(a[0], static_cast<std::size_t>(P) * nbytes);
    const std::vector<E8> sc = read_file<E8>(a[1], static_cast<std::size_t>(P) * nb);
    std::vector<Dev::Bucket<A>> buckets;
    std::vector<Dev::Bucket<E8>> scales;
    for (int p = 0; p < P; ++p) {
        buckets.emplace_back(std::vector<A>(in.begin() + p * nbytes, in.begin() + (p + 1) * nbytes));
        scales.emplace_back(std::vector<E8>(sc.begin() + p * nb, sc.begin() + (p + 1) * nb));
    }
    std::vector<const Dev::Bucket<A>*> ins;
    std::vector<const Dev::Bucket<E8>*> in_scales;
    for (int p = 0; p < P; ++p) ins.push_back(&buckets[p]), in_scales.push_back(&scales[p]);
    Dev::Bucket<std::uint64_t> word(std::vector<std::uint64_t>{seed});
    Dev::Bucket<A> res(nbytes);
    Dev::Bucket<E8> res_scales(nb);
    if constexpr (std::is_same_v<A, F4>)
        Dev::reduce_tree_mx(op, alg, res, res_scales, n, ins, in_scales, 0, nullptr, Dev::Sr{word, first});
    else
        Dev::reduce_tree_mx(op, alg, res, res_scales, ins, in_scales, 0, nullptr, Dev::Sr{word, first});
    Dev::sync();
    write_file(a[2], res.download());
    write_file(a[3], res_scales.download());
    return 0;
}

template <class A>
static int quantize(std::size_t n, std::uint64_t seed, std::uint64_t first, char** a) {
    Dev::Bucket<float> src(read_file<float>(a[0], n));
    Dev::Bucket<A> q(bytes_of<A>(n));
    Dev::Bucket<E8> q_scales(Dev::mx_blocks(n));
    Dev::Bucket<std::uint64_t> word(std::vector<std::uint64_t>{seed});
    Dev::mx_quantize(q, q_scales, src, nullptr, Dev::Sr{word, first});
    Dev::sync();
    write_file(a[1], q.download());
    write_file(a[2], q_scales.download());
    return 0;
}

template <class F>
static int by_kind(const std::string& kind, F&& f) {
    if (kind == "e4m3") return f.template operator()<Dev::float8_e4m3>();
    if (kind == "e5m2") return f.template operator()<Dev::float8_e5m2>();
    if (kind == "e2m1") return f.template operator()<F4>();
    std::fprintf(stderr, "KIND is e4m3, e5m2 or e2m1\n");
    return 2;
}

struct Host {
    std::size_t n;
    std::uint64_t seed, first;
    char** a;
    template <class A>
    int operator()() const { return host<A>(n, seed, first, a); }
};
struct Reduce {
    int op, alg, P;
    std::size_t n;
    std::uint64_t seed, first;
    char** a;
    template <class A>
    int operator()() const { return reduce<A>(op, alg, P, n, seed, first, a); }
};
struct Quantize {
    std::size_t n;
    std::uint64_t seed, first;
    char** a;
    template <class A>
    int operator()() const { return quantize<A>(n, seed, first, a); }
};

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 2 ? argv[2] : "";
    auto u64 = [&](int k) { return static_cast<std::uint64_t>(std::strtoull(argv[k], nullptr, 10)); };
    try {
        if (mode == "checks" && argc == 2) return checks();
        if (mode == "host" && argc == 9) return by_kind(kind, Host{static_cast<std::size_t>(u64(3)), u64(4), u64(5), argv + 6});
        if (mode == "reduce" && argc == 13) {
            Dev::init(0);
            return by_kind(kind, Reduce{std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), static_cast<std::size_t>(u64(6)), u64(7), u64(8), argv + 9});
        }
        if (mode == "quantize" && argc == 9) {
            Dev::init(0);
            return by_kind(kind, Quantize{static_cast<std::size_t>(u64(3)), u64(4), u64(5), argv + 6});
        }
        std::fprintf(stderr, "usage: test_mx_sr host KIND N SEED FIRST SRC OUT OUT_SCALES | checks | "
                             "reduce KIND OP ALG P N SEED FIRST IN SCALES RESULT RESULT_SCALES | quantize KIND N SEED FIRST SRC Q Q_SCALES\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
