// Dev::reduce_tree_mx, Dev::mx_quantize and Dev::mx_dequantize on MXFP4 buckets (Dev::float4_e2m1x2: two E2M1 elements
// to a byte, the element count explicit) through files, in the style of test_mx, and the host widen / narrow of a nibble.
// Run by tests/test_gpu_mxfp4_cpp.py, which writes the inputs and compares the outputs with tests/_mxfp4.py.
//
//   test_mxfp4 reduce OP ALG OUT P N IN SCALES RESULT RESULT_SCALES
//     OP    0 SUM | 5 AVG         ALG   0 ALLREDUCE | 1 REDUCE (root 0) | 2 REDUCE_LTR       OUT   same | f32
//     P, N  peers, ELEMENTS per peer
//     IN      P x (N + 1) / 2 packed bytes, peer after peer      SCALES  P x ceil(N / 32) scale bytes, peer after peer
//     RESULT  written: (N + 1) / 2 bytes or N raw f32 values      RESULT_SCALES  written: ceil(N / 32) bytes (OUT = same)
//   test_mxfp4 quantize N SRC Q Q_SCALES BACK
//     SRC     N raw f32 values;  Q, Q_SCALES written: the MXFP4 bucket;  BACK written: N raw f32 values, Q dequantized
//   test_mxfp4 host N SRC CODES TABLE         (no device)
//     SRC     N raw f32 values, finite and of magnitude <= 6;  CODES written: N bytes, narrow of each;
//     TABLE   written: 16 raw f32 values, widen of every code
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

static int reduce(int op, int alg, const std::string& out, int P, std::size_t n, char** a) {
    static_assert(sizeof(F4) == 1 && sizeof(E8) == 1);
    const std::size_t nbytes = Dev::fp4_bytes(n), nb = Dev::mx_blocks(n);
    const std::vector<F4> in = read_file<F4>(a[0], static_cast<std::size_t>(P) * nbytes);
    const std::vector<E8> sc = read_file<E8>(a[1], static_cast<std::size_t>(P) * nb);
    std::vector<Dev::Bucket<F4>> buckets;
    std::vector<Dev::Bucket<E8>> scales;
    for (int p = 0; p < P; ++p) {
        buckets.emplace_back(std::vector<F4>(in.begin() + p * nbytes, in.begin() + (p + 1) * nbytes));
        scales.emplace_back(std::vector<E8>(sc.begin() + p * nb, sc.begin() + (p + 1) * nb));
    }
    std::vector<const Dev::Bucket<F4>*> ins;
    std::vector<const Dev::Bucket<E8>*> in_scales;
    for (int p = 0; p < P; ++p) ins.push_back(&buckets[p]), in_scales.push_back(&scales[p]);
    if (out == "f32") {
        Dev::Bucket<float> res(n);
        Dev::reduce_tree_mx(op, alg, res, n, ins, in_scales);
        Dev::sync();
        write_file(a[2], res.download());
    } else if (out == "same") {
        Dev::Bucket<F4> res(nbytes);
        Dev::Bucket<E8> res_scales(nb);
        Dev::reduce_tree_mx(op, alg, res, res_scales, n, ins, in_scales);
        Dev::sync();
        write_file(a[2], res.download());
        write_file(a[3], res_scales.download());
    } else {
        std::fprintf(stderr, "OUT is same or f32\n");
        return 2;
    }
    return 0;
}

static int quantize(std::size_t n, char** a) {
    Dev::Bucket<float> src(read_file<float>(a[0], n)), back(n);
    Dev::Bucket<F4> q(Dev::fp4_bytes(n));
    Dev::Bucket<E8> q_scales(Dev::mx_blocks(n));
    Dev::mx_quantize(q, q_scales, src);
    Dev::mx_dequantize(back, q, q_scales);
    Dev::sync();
    write_file(a[1], q.download());
    write_file(a[2], q_scales.download());
    write_file(a[3], back.download());
    return 0;
}

static int host(std::size_t n, char** a) {
    const std::vector<float> src = read_file<float>(a[0], n);
    std::vector<std::uint8_t> codes(n);
    for (std::size_t i = 0; i < n; ++i) codes[i] = F4::narrow(src[i]);
    std::vector<float> table(16);
    for (int c = 0; c < 16; ++c) {
        table[c] = F4::widen(static_cast<std::uint8_t>(c));
        if (F4::narrow(table[c]) != c) {
            std::fprintf(stderr, "narrow(widen(%d)) is %d\n", c, F4::narrow(table[c]));
            return 1;
        }
    }
    const F4 pair = F4::from_codes(0x3, 0xE);
    if (pair.bits != 0xE3 || pair.lo() != 0x3 || pair.hi() != 0xE || Dev::fp4_bytes(33) != 17 || Dev::dtype_of<F4>() != -1) {
        std::fprintf(stderr, "packing: element 2k is bits 3:0, element 2k + 1 bits 7:4; no C-ABI dtype of its own\n");
        return 1;
    }
    write_file(a[1], codes);
    write_file(a[2], table);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "host" && argc == 6) return host(std::strtoull(argv[2], nullptr, 10), argv + 3);
        if (mode == "reduce" && argc == 11) {
            Dev::init(0);
            return reduce(std::atoi(argv[2]), std::atoi(argv[3]), argv[4], std::atoi(argv[5]), std::strtoull(argv[6], nullptr, 10), argv + 7);
        }
        if (mode == "quantize" && argc == 7) {
            Dev::init(0);
            return quantize(std::strtoull(argv[2], nullptr, 10), argv + 3);
        }
        std::fprintf(stderr, "usage: test_mxfp4 reduce OP ALG OUT P N IN SCALES RESULT RESULT_SCALES | quantize N SRC Q Q_SCALES BACK | "
                             "host N SRC CODES TABLE\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
