// Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize on MXFP6 buckets (Dev::float6_e2m3_packed /
// Dev::float6_e3m2_packed: four elements to three bytes, the element count explicit) through files, in the style of
// test_mxfp4, and the host pack / widen / narrow of a code. Run by tests/test_gpu_mxfp6_cpp.py, which writes the inputs
// and compares the outputs with tests/_mxfp6.py.
//
//   test_mxfp6 reduce KIND OP ALG OUT P N IN SCALES RESULT RESULT_SCALES
//     KIND  e2m3 | e3m2           OP    0 SUM | 5 AVG         ALG   0 ALLREDUCE | 1 REDUCE (root 0) | 2 REDUCE_LTR
//     OUT   same | f32 | sr:SEED:FIRST (the inputs' type, stochastic rounding)
//     P, N  peers, ELEMENTS per peer (P = 1 runs the fallback route)
//     IN      P x fp6_bytes(N) packed bytes, peer after peer      SCALES  P x ceil(N / 32) scale bytes, peer after peer
//     RESULT  written: fp6_bytes(N) bytes or N raw f32 values      RESULT_SCALES  written: ceil(N / 32) bytes (OUT != f32)
//   test_mxfp6 quantize KIND N SRC Q Q_SCALES BACK
//     SRC     N raw f32 values;  Q, Q_SCALES written: the MXFP6 bucket;  BACK written: N raw f32 values, Q dequantized
//   test_mxfp6 host KIND N SRC CODES TABLE PACKED HOSTSR HOSTSR_SCALES         (no device)
//     SRC     N raw f32 values, finite and of magnitude <= the largest element;  CODES written: N bytes, narrow of each;
//     TABLE   written: 64 raw f32 values, widen of every code;  PACKED written: fp6_pack of CODES;
//     HOSTSR, HOSTSR_SCALES written: Dev::mx_quantize_sr_host of SRC at seed 0x0123456789ABCDEF, first 64
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fmi/fmi.h"

namespace Dev = FMI::Dev;
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

template <class F6>
static int reduce(int op, int alg, const std::string& out, int P, std::size_t n, char** a) {
    static_assert(sizeof(F6) == 1 && sizeof(E8) == 1);
    const std::size_t nbytes = Dev::fp6_bytes(n), nb = Dev::mx_blocks(n);
    const std::vector<F6> in = read_file<F6>(a[0], static_cast<std::size_t>(P) * nbytes);
    const std::vector<E8> sc = read_file<E8>(a[1], static_cast<std::size_t>(P) * nb);
    std::vector<Dev::Bucket<F6>> buckets;
    std::vector<Dev::Bucket<E8>> scales;
    for (int p = 0; p < P; ++p) {
        buckets.emplace_back(std::vector<F6>(in.begin() + p * nbytes, in.begin() + (p + 1) * nbytes));
        scales.emplace_back(std::vector<E8>(sc.begin() + p * nb, sc.begin() + (p + 1) * nb));
    }
    std::vector<const Dev::Bucket<F6>*> ins;
    std::vector<const Dev::Bucket<E8>*> in_scales;
    for (int p = 0; p < P; ++p) ins.push_back(&buckets[p]), in_scales.push_back(&scales[p]);
    if (out == "f32") {
        Dev::Bucket<float> res(n);
        Dev::reduce_tree_mx(op, alg, res, n, ins, in_scales);
        Dev::sync();
        write_file(a[2], res.download());
        return 0;
    }
    Dev::Bucket<F6> res(nbytes);
    Dev::Bucket<E8> res_scales(nb);
    if (out == "same") {
        Dev::reduce_tree_mx(op, alg, res, res_scales, n, ins, in_scales);
    } else if (out.rfind("sr:", 0) == 0) {
        char* end = nullptr;
        const std::uint64_t seed = std::strtoull(out.c_str() + 3, &end, 0);
        const std::uint64_t first = std::strtoull(end + 1, nullptr, 0);
        Dev::Bucket<std::uint64_t> word(std::vector<std::uint64_t>{seed});
        Dev::reduce_tree_mx(op, alg, res, res_scales, n, ins, in_scales, 0, nullptr, Dev::Sr{word, first});
        Dev::sync();
    } else {
        std::fprintf(stderr, "OUT is same, f32 or sr:SEED:FIRST\n");
        return 2;
    }
    Dev::sync();
    write_file(a[2], res.download());
    write_file(a[3], res_scales.download());
    return 0;
}

template <class F6>
static int quantize(std::size_t n, char** a) {
    Dev::Bucket<float> src(read_file<float>(a[0], n)), back(n);
    Dev::Bucket<F6> q(Dev::fp6_bytes(n));
    Dev::Bucket<E8> q_scales(Dev::mx_blocks(n));
    Dev::mx_quantize(q, q_scales, src);
    Dev::mx_dequantize(back, q, q_scales);
    Dev::sync();
    write_file(a[1], q.download());
    write_file(a[2], q_scales.download());
    write_file(a[3], back.download());
    return 0;
}

template <class F6>
static int host(std::size_t n, char** a) {
    const std::vector<float> src = read_file<float>(a[0], n);
    std::vector<std::uint8_t> codes(n);
    for (std::size_t i = 0; i < n; ++i) codes[i] = F6::narrow(src[i]);
    std::vector<float> table(64);
    for (int c = 0; c < 64; ++c) {
        table[c] = F6::widen(static_cast<std::uint8_t>(c));
        if (F6::narrow(table[c]) != c) {
            std::fprintf(stderr, "narrow(widen(%d)) is %d\n", c, F6::narrow(table[c]));
            return 1;
        }
    }
    const std::vector<F6> packed = Dev::fp6_pack<F6>(codes);
    if (packed.size() != Dev::fp6_bytes(n) || Dev::fp6_unpack(packed, n) != codes || Dev::fp6_bytes(33) != 25 || Dev::fp6_bytes(4) != 3 ||
        Dev::dtype_of<F6>() != -1) {
        std::fprintf(stderr, "packing: n elements are ceil(3 n / 4) bytes and unpack inverts pack; no C-ABI dtype of its own\n");
        return 1;
    }
    std::vector<F6> sr;
    std::vector<E8> sr_scales;
    Dev::mx_quantize_sr_host(sr, sr_scales, src, 0x0123456789ABCDEFull, 64);
    write_file(a[1], codes);
    write_file(a[2], table);
    write_file(a[3], packed);
    write_file(a[4], sr);
    write_file(a[5], sr_scales);
    return 0;
}

template <class F6>
static int run(const std::string& mode, int argc, char** argv) {
    if (mode == "host" && argc == 10) return host<F6>(std::strtoull(argv[3], nullptr, 10), argv + 4);
    if (mode == "reduce" && argc == 12) {
        Dev::init(0);
        return reduce<F6>(std::atoi(argv[3]), std::atoi(argv[4]), argv[5], std::atoi(argv[6]), std::strtoull(argv[7], nullptr, 10), argv + 8);
    }
    if (mode == "quantize" && argc == 8) {
        Dev::init(0);
        return quantize<F6>(std::strtoull(argv[3], nullptr, 10), argv + 4);
    }
    std::fprintf(stderr, "usage: test_mxfp6 reduce KIND OP ALG OUT P N IN SCALES RESULT RESULT_SCALES | quantize KIND N SRC Q Q_SCALES BACK | "
                         "host KIND N SRC CODES TABLE PACKED HOSTSR HOSTSR_SCALES\n");
    return 2;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 2 ? argv[2] : "";
    try {
        if (kind == "e2m3") return run<Dev::float6_e2m3_packed>(mode, argc, argv);
        if (kind == "e3m2") return run<Dev::float6_e3m2_packed>(mode, argc, argv);
        std::fprintf(stderr, "KIND is e2m3 or e3m2\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
