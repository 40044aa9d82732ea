// Dev::reduce_tree_scaled of the C++ FMI surface (fmi_dev_reduce_tree_scaled) through files, in the style of
// test_fp8's file modes. Run by tests/test_gpu_fp8_scaled_cpp.py, which writes the inputs and compares the outputs with
// tests/_fp8_scaled.py.
//
//   test_fp8_scaled KIND ALG OUT P N IN SCALES T RESULT AMAX
//     KIND    e4m3 | e5m2               ALG   0 ALLREDUCE | 1 REDUCE (root 0) | 2 REDUCE_LTR
//     OUT     same | f32                P, N  peers, elements per peer
//     IN      P x N input bytes, peer after peer         SCALES  P raw f32 values
//     T       the output scale as a decimal, or "none"
//     RESULT  written: N bytes or N raw f32 values        AMAX    written: 4 bytes, the folded amax word (starts at 0)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fmi/fmi.h"

namespace Dev = FMI::Dev;

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

template <class A, class O>
static int run(int alg, int P, std::size_t n, char** a) {
    static_assert(sizeof(A) == 1);
    const std::vector<A> in = read_file<A>(a[0], static_cast<std::size_t>(P) * n);
    std::vector<Dev::Bucket<A>> buckets;
    std::vector<const Dev::Bucket<A>*> ins;
    for (int p = 0; p < P; ++p) buckets.emplace_back(std::vector<A>(in.begin() + p * n, in.begin() + (p + 1) * n));
    for (const auto& b : buckets) ins.push_back(&b);
    Dev::Bucket<float> scales(read_file<float>(a[1], P)), amax(std::vector<float>{0.0f});
    Dev::Bucket<O> out(n);
    if (std::string(a[2]) == "none") {
        Dev::reduce_tree_scaled(alg, out, ins, scales, nullptr, &amax);
    } else {
        Dev::Bucket<float> t(std::vector<float>{std::strtof(a[2], nullptr)});
        Dev::reduce_tree_scaled(alg, out, ins, scales, &t, &amax);
    }
    Dev::sync();
    write_file(a[3], out.download());
    write_file(a[4], amax.download());
    return 0;
}

template <class A>
static int by_out(const std::string& out, int alg, int P, std::size_t n, char** a) {
    if (out == "same") return run<A, A>(alg, P, n, a);
    if (out == "f32") return run<A, float>(alg, P, n, a);
    std::fprintf(stderr, "OUT is same or f32\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: test_fp8_scaled KIND ALG OUT P N IN SCALES T RESULT AMAX\n");
        return 2;
    }
    const std::string kind = argv[1];
    const int alg = std::atoi(argv[2]), P = std::atoi(argv[4]);
    const std::size_t n = std::strtoull(argv[5], nullptr, 10);
    try {
        Dev::init(0);
        if (kind == "e4m3") return by_out<Dev::float8_e4m3>(argv[3], alg, P, n, argv + 6);
        if (kind == "e5m2") return by_out<Dev::float8_e5m2>(argv[3], alg, P, n, argv + 6);
        std::fprintf(stderr, "KIND is e4m3 or e5m2\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
