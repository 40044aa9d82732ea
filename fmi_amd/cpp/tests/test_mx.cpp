// Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize of the C++ FMI surface (fmi_dev_reduce_tree_mx and its
// two conversions) through files, in the style of test_fp8_scaled. Run by tests/test_gpu_mx_cpp.py, which writes the
// inputs and compares the outputs with tests/_mx.py.
//
//   test_mx reduce KIND OP ALG OUT P N IN SCALES RESULT RESULT_SCALES
//     KIND    e4m3 | e5m2               OP    0 SUM | 5 AVG         ALG   0 ALLREDUCE | 1 REDUCE (root 0) | 2 REDUCE_LTR
//     OUT     same | f32                P, N  peers, elements per peer
//     IN      P x N element bytes, peer after peer       SCALES  P x ceil(N / 32) scale bytes, peer after peer
//     RESULT  written: N bytes or N raw f32 values        RESULT_SCALES  written: ceil(N / 32) bytes (OUT = same)
//   test_mx quantize KIND N SRC Q Q_SCALES BACK
//     SRC     N raw f32 values;  Q, Q_SCALES written: the MX bucket;  BACK written: N raw f32 values, Q dequantized
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

template <class A>
static int reduce(int op, int alg, const std::string& out, int P, std::size_t n, char** a) {
    static_assert(sizeof(A) == 1 && sizeof(Dev::float8_e8m0) == 1);
    const std::size_t nb = Dev::mx_blocks(n);
    const std::vector<A> in = read_file<A>(a[0], static_cast<std::size_t>(P) * n);
    const std::vector<Dev::float8_e8m0> sc = read_file<Dev::float8_e8m0>(a[1], static_cast<std::size_t>(P) * nb);
    std::vector<Dev::Bucket<A>> buckets;
    std::vector<Dev::Bucket<Dev::float8_e8m0>> scales;
    for (int p = 0; p < P; ++p) {
        buckets.emplace_back(std::vector<A>(in.begin() + p * n, in.begin() + (p + 1) * n));
        scales.emplace_back(std::vector<Dev::float8_e8m0>(sc.begin() + p * nb, sc.begin() + (p + 1) * nb));
    }
    std::vector<const Dev::Bucket<A>*> ins;
    std::vector<const Dev::Bucket<Dev::float8_e8m0>*> in_scales;
    for (int p = 0; p < P; ++p) ins.push_back(&buckets[p]), in_scales.push_back(&scales[p]);
    if (out == "f32") {
        Dev::Bucket<float> res(n);
        Dev::reduce_tree_mx(op, alg, res, ins, in_scales);
        Dev::sync();
        write_file(a[2], res.download());
    } else if (out == "same") {
        Dev::Bucket<A> res(n);
        Dev::Bucket<Dev::float8_e8m0> res_scales(nb);
        Dev::reduce_tree_mx(op, alg, res, res_scales, ins, in_scales);
        Dev::sync();
        write_file(a[2], res.download());
        write_file(a[3], res_scales.download());
    } else {
        std::fprintf(stderr, "OUT is same or f32\n");
        return 2;
    }
    return 0;
}

template <class A>
static int quantize(std::size_t n, char** a) {
    Dev::Bucket<float> src(read_file<float>(a[0], n)), back(n);
    Dev::Bucket<A> q(n);
    Dev::Bucket<Dev::float8_e8m0> q_scales(Dev::mx_blocks(n));
    Dev::mx_quantize(q, q_scales, src);
    Dev::mx_dequantize(back, q, q_scales);
    Dev::sync();
    write_file(a[1], q.download());
    write_file(a[2], q_scales.download());
    write_file(a[3], back.download());
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 2 ? argv[2] : "";
    const bool e4 = kind == "e4m3";
    if (!e4 && kind != "e5m2") {
        std::fprintf(stderr, "usage: test_mx reduce KIND OP ALG OUT P N IN SCALES RESULT RESULT_SCALES | test_mx quantize KIND N SRC Q Q_SCALES BACK\n");
        return 2;
    }
    try {
        Dev::init(0);
        if (mode == "reduce" && argc == 12) {
            const int op = std::atoi(argv[3]), alg = std::atoi(argv[4]), P = std::atoi(argv[6]);
            const std::size_t n = std::strtoull(argv[7], nullptr, 10);
            return e4 ? reduce<Dev::float8_e4m3>(op, alg, argv[5], P, n, argv + 8) : reduce<Dev::float8_e5m2>(op, alg, argv[5], P, n, argv + 8);
        }
        if (mode == "quantize" && argc == 8) {
            const std::size_t n = std::strtoull(argv[3], nullptr, 10);
            return e4 ? quantize<Dev::float8_e4m3>(n, argv + 4) : quantize<Dev::float8_e5m2>(n, argv + 4);
        }
        std::fprintf(stderr, "test_mx: wrong mode or argument count\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
