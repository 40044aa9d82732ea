/*
 * fmi_dev.h — C-ABI of the MI355X (gfx950) bucket-reduction engine behind FMI's collectives.
 *
 * This is the drop-in boundary for FMI's local element-wise bucket reduction. In the reference the
 * reduction is an opaque host closure, `raw_func = std::function<void(char*, char*)>`
 * (reference include/comm/Channel.h:16-23), built by Communicator::convert_to_raw_function
 * (reference include/Communicator.h:170-189) and applied by the PeerToPeer collectives as
 * `f.f(inout, in)` (reference src/comm/PeerToPeer.cpp:51,72,103,119,147,160,179).
 * Here the same combine is a HIP kernel launch on device-resident buckets, addressed by an explicit
 * op/dtype descriptor because the reference's closure carries neither.
 *
 * Conventions:
 *   - every entry point returns int: 0 = success, negative = fmi_status_t error; the message of the
 *     last failure on the calling thread is available from fmi_last_error(). No exception ever
 *     crosses this boundary; the C++ layer (fmi_amd/cpp/include/fmi/) rethrows std::runtime_error.
 *   - plain pointers and element counts only; no torch / HIP types in signatures. A stream is an
 *     opaque handle (hipStream_t underneath); NULL means the library's default stream of the device
 *     selected by fmi_dev_init.
 *   - the caller owns every buffer passed in; the library owns only its streams, events and scratch.
 *   - `inout`/`in` follow raw_func: argument 0 is overwritten, argument 1 is read-only, equal length.
 *   - all launches are asynchronous on the given stream; fmi_stream_sync / fmi_dev_sync wait.
 *
 * Element semantics match the reference's built-in ops (reference python/PythonCommunicator.h:116-149):
 *   SUM = a + b (std::plus), PROD = a * b (std::multiplies), MAX = std::max(a,b) = (a < b) ? b : a,
 *   MIN = std::min(a,b) = (b < a) ? b : a. Integer SUM/PROD wrap modulo 2^bits (two's complement), as
 *   the reference's int32 13! test relies on (reference tests/channels.cpp:419-465). Floats use IEEE
 *   round-to-nearest-even with denormals preserved and no contraction: a single device combine is
 *   bit-identical to the host one.
 */
#ifndef FMI_DEV_H
#define FMI_DEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMI_DEV_ABI_VERSION 1

/* ---- status ------------------------------------------------------------------------------------ */
typedef enum {
    FMI_OK = 0,
    FMI_ERR_INVALID = -1,     /* bad argument (null pointer, unknown op/dtype, P out of range ...) */
    FMI_ERR_HIP = -2,         /* a HIP runtime call failed; message names the call */
    FMI_ERR_NO_DEVICE = -3,   /* no gfx950 device visible / fmi_dev_init not called */
    FMI_ERR_UNSUPPORTED = -4, /* combination not implemented */
    FMI_ERR_ALLOC = -5,       /* device or pinned allocation failed */
    FMI_ERR_COMM = -6,        /* a communicator / transport (RCCL) call failed */
    FMI_ERR_TIMEOUT = -7      /* a peer did not arrive within the communicator's timeout (the reference's
                                 FMI::Utils::Timeout, include/utils/Common.h:11-15, raised by its channels
                                 when a peer stays away, src/comm/Direct.cpp:28-30,40-42). The communicator
                                 is aborted: later calls on it fail with FMI_ERR_COMM; destroy it. */
} fmi_status_t;

/* ---- op / dtype / algorithm descriptors -------------------------------------------------------- */
/* Op ids mirror the reference Python enum SUM/PROD/MAX/MIN (reference python/PythonCommunicator.h:13-15). */
typedef enum { FMI_OP_SUM = 0, FMI_OP_PROD = 1, FMI_OP_MAX = 2, FMI_OP_MIN = 3, FMI_OP_AVG = 5 } fmi_op_t;
/* FMI_OP_AVG = 5: the mean over the peers. Id 4 stays unassigned in the C-ABI: the reference's Python enum gives 4
 * to CUSTOM. Additive: fmi_abi_version() stays 1. A call with FMI_OP_AVG over P peers stores
 *     out = store( fl_V( S x r_P ) )
 *   V    the value type: f32 for FMI_F32, FMI_F16, FMI_BF16, FMI_F8E4M3 and FMI_F8E5M2 (with or without FMI_ACC_F32);
 *        f64 for FMI_F64.
 *   S    what the same call with FMI_OP_SUM and the same `alg` holds in V just before its store. Plain dtypes: S is
 *        the SUM result itself (for f16 / bf16 already rounded to storage after every combine; it is widened).
 *        With FMI_ACC_F32: S is the f32 program value, not yet narrowed, so the result is
 *        narrow(F32sum(widen(x)) x r_P), one rounding to storage in all.
 *   r_P  fl_V(1 / P), the correctly rounded reciprocal in V. The product is one IEEE multiply (round-to-nearest-even,
 *        subnormals kept, no contraction).
 *   store  identity for f32 / f64; for the 16-bit types the narrowing every combine ends with.
 * Multiplying by the reciprocal, not dividing, is deliberate: it is what RCCL's own average does, it costs one VALU
 * op per element, and it equals S / P exactly for P = 2^k, the usual GPU counts. For other P it differs from the
 * division in the last bit on some elements (about a third of random f32 sums at P = 3). P = 1 stays the copy, bits
 * unchanged. A NaN result is some NaN.
 * Valid: float dtypes only, and only in calls that produce a reduction result:
 *   fmi_dev_reduce_tree at FMI_ALG_ALLREDUCE / _REDUCE / _REDUCE_LTR                 divisor P
 *   fmi_comm_allreduce on every path, fmi_comm_allreduce_host, fmi_comm_reduce        divisor nranks
 *     (the shard step is the fmi_dev_reduce_tree call above with P = nranks; FMI_PATH_RCCL runs its reduce-scatter
 *     with SUM, scales its shard, then all-gathers: no new RCCL call, and its bound is the SUM bound times r_P plus
 *     one ulp of the result; a one-rank communicator stays the copy)
 * FMI_ERR_INVALID, with a message naming the op and the reason:
 *   integer dtypes;
 *   fmi_dev_reduce_pair, _batch, fmi_dev_combine, fmi_host_reduce_pair (a pairwise mean does not compose);
 *   fmi_dev_scan_peers, fmi_comm_scan, and the scan algorithms passed to fmi_dev_reduce_tree (a prefix has no mean);
 *   fmi_comm_reduce_sendbuf (the partials it leaves in the sendbufs are sums).
 * At 2 <= P <= 16 on 16-B aligned buckets the call is ONE fused kernel (P reads, one store): the SUM program with the
 * value scaled in registers just before its store. Every other call (P > 16, unaligned buckets) runs the unchanged SUM
 * program and then the scale kernel of fmi_dev_mean_scale in place on `out`: the same bits by the definition above.
 * With FMI_ACC_F32 beyond 16 peers or on unaligned buckets the f32 result temporary is scaled before it is narrowed:
 * still one rounding to storage. */
/* Element types. The reference's buckets are Data<std::vector<A>> for any fundamental A
 * (include/comm/Data.h:50-73); f32 / f64 / i32 / i64 run every kernel, including the fused P-way ones.
 * The other integer widths run the pairwise kernel, and their P-way programs run as pairwise passes in
 * the same order (integer results do not depend on it). Integer sum / prod wrap, as the reference's
 * std::plus / std::multiplies do after conversion back to A.
 *
 * FMI_F16 (IEEE binary16) and FMI_BF16 (the upper 16 bits of binary32). One combine widens both operands to
 * f32 (exact), applies the op in f32 (round-to-nearest-even, subnormals kept) and narrows the result to the
 * storage type (round-to-nearest-even, subnormals kept, NaN stays NaN). The result is rounded to the storage
 * type after EVERY combine of a P-way program, in the program's own order: what the reference's
 * f.f(mine, received) computes at a 16-bit float element type (std::plus<__bf16>). For bf16 this widened form
 * is the definition (a correctly rounded bf16 product differs from it deep in the subnormal range); for f16 it
 * equals native binary16 arithmetic. MAX / MIN are the selections above: the kept operand's 16 bits come out
 * unchanged (±0, NaN payloads, subnormals). A NaN made by SUM / PROD is some NaN (sign and payload unspecified).
 * The two have every single-pass kernel f32 has: fmi_dev_reduce_tree and fmi_dev_scan_peers at all five algorithms
 * and any P on 16-B aligned buckets (fused up to 31 peers, the one-pass chains, blocked trees, pre-fold allreduces
 * and blocked scans beyond, superblocks past 128), and with them the shard kernels of fmi_comm_allreduce / reduce /
 * scan and fmi_comm_reduce_sendbuf's partials at any number of ranks. Only unaligned buckets run as pairwise passes
 * in the same order (the 16-bit integers' path), bit for bit the same values. Additive: fmi_abi_version() stays 1.
 *
 * FMI_F8E4M3 and FMI_F8E5M2: the two OCP 8-bit floats (gfx950's own encodings, not MI300's fnuz ones). Buckets are
 * arrays of bytes.
 *   FMI_F8E4M3 = 12  OCP E4M3 (e4m3fn): bias 7, no infinities, NaN = S.1111.111 only, largest finite 448, subnormals
 *                    down to 2^-9.
 *   FMI_F8E5M2 = 13  OCP E5M2: bias 15, IEEE-style infinities and NaNs, largest finite 57344, subnormals down to 2^-16.
 * Widen (fp8 -> f32) is exact for every one of the 256 patterns; a NaN widens to some NaN.
 * Narrow (f32 -> fp8) rounds to nearest even at the format's precision, keeps subnormals and the zero's sign, and does
 * NOT saturate: if the rounded magnitude exceeds the largest finite value, or the input is +-inf, E5M2 gives +-inf and
 * E4M3 gives NaN; NaN stays NaN (E4M3: 464 -> 0x7E, the tie to even, 448; 465 -> 0x7F, NaN. E5M2: 61440 -> 0x7C, the
 * tie to even, inf; 61439.9 -> 0x7B). This is what tensor.to(torch.float8_e4m3fn / float8_e5m2) computes on the CPU.
 * Deliberate: a reduction that overflows its storage type should show it, not return 448. A NaN result is some NaN.
 * One combine follows the f16 / bf16 rule: widen both operands, apply the op in f32 (round-to-nearest-even, subnormals
 * kept, no contraction), narrow; after EVERY combine of a plain P-way program, in the program's own order. The f32
 * intermediate is part of the definition (an E5M2 sum is not always exact in f32; an E4M3 sum is). MAX / MIN are
 * selections on the widened compare: the kept operand's byte comes out unchanged, so +-0 and NaN depend on the rank as
 * for f32.
 * Every pairwise entry point serves them (fmi_dev_reduce_pair, _batch, fmi_dev_combine, fmi_host_reduce_pair,
 * fmi_dev_mean_scale, fmi_dev_fill_synthetic*). With FMI_ACC_F32 (below), SUM / PROD / FMI_OP_AVG at 2 <= P <= 16 on
 * 16-B aligned buckets run ONE fused kernel at all five algorithms and for reduce partials: the form a gradient bucket
 * wants. PLAIN 8-bit float P-way programs (no flag) have no fused kernel, on purpose: at any P and algorithm they run
 * as pairwise passes in the program's own order, per-rank MAX / MIN included (the path unaligned 16-bit buckets
 * take), and round the running value to 4 (E4M3) or 3 (E5M2) significant bits per combine; the form exists because it
 * is what the reference's template computes at such an element type. FMI_OP_AVG is valid on both, plain and with the
 * flag, by its definition: V = f32, store = narrow. fmi_dev_convert (below) moves f32 / f16 / bf16 data into and out
 * of such buckets. Additive: fmi_abi_version() stays 1.
 *
 * FMI_F4E2M1 = 15: the OCP 4-bit float E2M1, the element of an MXFP4 bucket. 1 sign bit, 2 exponent bits (bias 1),
 * 1 mantissa bit: the magnitudes of codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 is the sign (so -0 exists); no
 * inf, no NaN. Two elements to a byte: a bucket of n elements is ceil(n / 2) bytes, element 2k in bits 3:0 of byte k,
 * element 2k + 1 in bits 7:4; for odd n the last byte's high nibble is ignored on input and written as 0 on output.
 * Widen is the 16-entry table (exact). Narrow (f32 -> E2M1) is round-to-nearest on the eight magnitudes with ties to
 * the even CODE (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), the sign kept (-0.2 -> 0x8);
 * it is defined for finite |y| <= 6 only, which is all the MX calls feed it.
 * The type is valid ONLY as the `dtype` of the four MX calls (fmi_dev_reduce_tree_mx, fmi_dev_mx_quantize,
 * fmi_dev_mx_dequantize, fmi_comm_allreduce_mx; there FMI_ACC_F32 on it is accepted and dropped). Every other entry
 * point that takes a dtype answers FMI_ERR_INVALID with a message naming FMI_F4E2M1, on the host. Additive:
 * fmi_abi_version() stays 1, no new symbol.
 *
 * FMI_F6E2M3 = 16, FMI_F6E3M2 = 17: the two OCP 6-bit floats, the elements of an MXFP6 bucket. Six bits per element:
 * bit 5 is the sign (so -0 exists, code 0x20); no inf, no NaN; the magnitude codes 0..31 ascend in value.
 *   E2M3: 2 exponent bits (bias 1), 3 mantissa bits. Exponent field 0: m / 8 (0, 0.125 .. 0.875); otherwise
 *         (1 + m / 8) * 2^(e - 1). The largest value is 7.5 = 1.875 * 2^2.
 *   E3M2: 3 exponent bits (bias 3), 2 mantissa bits. Exponent field 0: m / 16 (0, 0.0625, 0.125, 0.1875); otherwise
 *         (1 + m / 4) * 2^(e - 3). The largest value is 28 = 1.75 * 2^4.
 * Packing: the bucket is a little-endian bit string, element i in bits 6 i .. 6 i + 5, bit j of the string being bit
 * j mod 8 of byte j div 8. Four elements are three bytes, a block of 32 is 24 bytes, n elements take ceil(3 n / 4)
 * bytes; the unused high bits of the last byte are ignored on input and written as 0 on output. Widen is the 64-entry
 * table (exact in f32). Narrow is round-to-nearest on the 32 magnitudes with ties to the even CODE, the sign kept; it is
 * defined for finite |y| <= the largest element only, which is all the MX calls feed it.
 * Like FMI_F4E2M1, both are valid ONLY as the `dtype` of the MX calls (FMI_ACC_F32 on them is accepted and dropped
 * there); every other entry point that takes a dtype, fmi_dev_fill_synthetic* included, answers FMI_ERR_INVALID with a
 * message naming the type, on the host. Additive: fmi_abi_version() stays 1, no new symbol. */
typedef enum {
    FMI_F32 = 0, FMI_F64 = 1, FMI_I32 = 2, FMI_I64 = 3,
    FMI_U32 = 4, FMI_U64 = 5, FMI_I8 = 6, FMI_U8 = 7, FMI_I16 = 8, FMI_U16 = 9,
    FMI_F16 = 10, FMI_BF16 = 11, FMI_F8E4M3 = 12, FMI_F8E5M2 = 13,
    FMI_F4E2M1 = 15, FMI_F6E2M3 = 16, FMI_F6E3M2 = 17
} fmi_dtype_t;
/* Reserved, NOT an fmi_dtype_t: FMI_F8E8M0 = 14 is the label the Python binding gives the scale bytes of an MX bucket
 * (DType.F8E8M0, bytes over np.uint8; fmi_dev_reduce_tree_mx below). No C-ABI call takes it as a dtype: every one
 * answers "unknown dtype". The scale arrays of the MX calls are plain byte pointers. */

/* f32 accumulation: a modifier bit on the dtype ARGUMENT of a call, valid only on FMI_F16, FMI_BF16, FMI_F8E4M3 and
 * FMI_F8E5M2 (with any other dtype: FMI_ERR_INVALID naming the dtype). The buckets keep their storage type; a P-way
 * program at T | FMI_ACC_F32
 *   1. widens every input element to f32 (exact),
 *   2. runs the SAME program in the SAME order (the bracketing of `alg`) with f32 combines: IEEE round-to-nearest-
 *      even, subnormals kept, no contraction, exactly what the FMI_F32 kernels compute,
 *   3. narrows every value the call STORES to T once (round-to-nearest-even, subnormals kept, NaN stays NaN; for the
 *      8-bit floats the non-saturating narrowing defined at fmi_dtype_t): the
 *      result of fmi_dev_reduce_tree, every prefix of fmi_dev_scan_peers, every partial fmi_comm_reduce_sendbuf leaves
 *      in a sendbuf, each its own f32 value rounded once.
 * In one line: out = narrow(F32_program(widen(x))). What a gradient bucket that travels in bf16 wants: the plain
 * dtypes round the running value to 8 (bf16) or 11 (f16) significant bits after every combine.
 * MAX / MIN are selections, which f32 accumulation cannot change: the flag is accepted and dropped, and the plain
 * kernels run (per-rank bits as before). A single combine is already "widen, op, round once": the pairwise calls
 * (fmi_dev_reduce_pair, _batch, fmi_dev_combine, fmi_host_reduce_pair) accept the flag and drop it, and P = 1 stays
 * the copy. A NaN made by SUM / PROD is some NaN. Entry points that only store (fmi_dev_fill_synthetic*) take the
 * plain dtype and answer the flag with FMI_ERR_INVALID.
 * SUM / PROD at 2 <= P <= 16 on 16-B aligned buckets run one fused kernel (P reads, the stores, nothing else), at
 * all five algorithms and for reduce partials. Any other call (P > 16, unaligned buckets) widens every input into an
 * f32 temporary, runs the library's own FMI_F32 program on those and narrows every stored output: the same
 * definition by construction, at P * n * 4 bytes of temporaries (+ n * 4 for fmi_dev_reduce_tree's result) in an
 * allocation of the library's own (FMI_ERR_ALLOC if it cannot be had).
 * The communicator calls (fmi_comm_allreduce on paths TREE and DIRECT, _allreduce_host, _reduce, _reduce_sendbuf,
 * _scan) accept it: the wire keeps the storage type (16-bit or 8-bit) and only the shard step changes; every rank passes the same dtype argument,
 * as every other argument. FMI_PATH_RCCL with the flag (SUM / PROD) is FMI_ERR_UNSUPPORTED: RCCL's reduction has its
 * own order and rounding. Additive: fmi_abi_version() stays 1, no new symbol. */
#define FMI_ACC_F32 0x100   /* valid only on FMI_F16, FMI_BF16, FMI_F8E4M3 and FMI_F8E5M2 (and dropped by the MX calls) */

/* Evaluation orders reproduced by the P-way kernels; each is the combine order of one reference
 * collective, so a P-bucket reduction on one device is bit-identical to the distributed one. */
typedef enum {
    FMI_ALG_ALLREDUCE = 0,  /* recursive doubling + non-power-of-2 fold: PeerToPeer.cpp:96-130   */
    FMI_ALG_REDUCE = 1,     /* binomial tree toward root (transformed ids): PeerToPeer.cpp:59-84  */
    FMI_ALG_REDUCE_LTR = 2, /* gather + sequential left fold at root: PeerToPeer.cpp:44-57         */
    FMI_ALG_SCAN = 3,       /* binomial up/down sweep, own-op-received: PeerToPeer.cpp:154-184     */
    FMI_ALG_SCAN_LTR = 4    /* linear chain, prefix-op-own: PeerToPeer.cpp:141-152                 */
} fmi_alg_t;

typedef void* fmi_stream_t;
typedef void* fmi_event_t;

/* ---- library / device -------------------------------------------------------------------------- */
int fmi_abi_version(void);
/* Message of the last failed call on this thread ("" if none). Valid until the next failing call. */
const char* fmi_last_error(void);
/* Number of visible HIP devices (0 on a host without a GPU; never fails for lack of a device). */
int fmi_dev_count(int* count);
/* Select the device for this thread and create the library's default stream for it.
 * Fails with FMI_ERR_NO_DEVICE if the device is missing or is not gfx950. */
int fmi_dev_init(int device);
/* Release the library's streams and scratch (mirrors Channel::finalize, reference
 * include/comm/Channel.h:106). Buffers allocated by the caller are not touched. */
int fmi_dev_finalize(void);
/* Wait for all work on the selected device. */
int fmi_dev_sync(void);
/* Device name + arch string (e.g. "AMD Instinct MI355X gfx950"), CU count, HBM size, and the number of
 * fmi_host_reduce_pair staging sets ("host_pipelines=N idle=M": one per calling thread alive, idle ones are
 * those of exited threads, reused by the next new caller), NUL-terminated into buf. */
int fmi_dev_describe(char* buf, size_t len);
/* PCI bus id ("dddd:bb:dd.f") of a visible device, NUL-terminated into buf (hipDeviceGetPCIBusId): with
 * fmi_comm_query, lets the ranks of a communicator show they sit on distinct GPUs. */
int fmi_dev_pci_bus_id(int device, char* buf, size_t len);

/* ---- memory (replaces the reference's new[]/std::vector bucket storage, include/comm/Data.h:50-97)
 * fmi_dev_alloc: device memory, 4 KiB aligned: a plain hipMalloc (the pairwise kernel's best placement), or with
 * FMI_TUNE_ALLOC_SLOTS = 1 buckets of >= 1 MiB in rotating 4 KiB slots. Free with fmi_dev_free only (a slotted
 * pointer lies inside its hipMalloc, up to 60 KiB past its base, so it is not a hipIpcGetMemHandle base either:
 * memory shared across processes comes from fmi_comm_window_alloc). */
int fmi_dev_alloc(void** ptr, size_t bytes);
/* fmi_dev_alloc_group: `count` buckets of `bytes` each that one kernel streams together (a fused kernel's P
 * inputs and its outputs). Buckets of >= 1 MiB are carved from ONE allocation at a stride of `bytes` rounded up to
 * 64 KiB plus 4 KiB, so bucket j sits in 4 KiB slot j mod 16 (modulo 64 KiB) whatever was allocated before and
 * whatever FMI_TUNE_ALLOC_SLOTS says, and the group's streams never collide in HBM; smaller ones are
 * plain allocations. All or nothing: on failure every ptrs[j] is NULL. Free each with fmi_dev_free, in any order: a
 * carved group's memory is released with its last bucket. */
int fmi_dev_alloc_group(void** ptrs, int count, size_t bytes);
int fmi_dev_free(void* ptr);
int fmi_host_pin_alloc(void** ptr, size_t bytes);  /* page-locked host memory for recv buffers */
int fmi_host_pin_free(void* ptr);
/* Page-lock an existing host range in place (hipHostRegister, mapped), e.g. a channel recv buffer that is
 * reused across collectives (reference include/comm/Data.h:50-73 std::vector storage), so that
 * fmi_host_reduce_pair combines it zero-copy and the host pipelines move it at DMA rate. Registering
 * costs about as much as one copy of the range: worth it only for buffers used more than once. The range
 * must stay allocated until fmi_host_unregister(ptr) with the same ptr. A bucket handed to
 * fmi_host_reduce_pair must lie wholly inside one page-locked range or wholly outside any
 * (FMI_ERR_INVALID otherwise). */
int fmi_host_register(void* ptr, size_t bytes);
int fmi_host_unregister(void* ptr);
/* The device address of [host, host + bytes), a range wholly inside one page-locked, device-mapped range
 * (fmi_host_pin_alloc / fmi_host_register): what a caller hands to fmi_dev_reduce_pair to combine host recv
 * buffers in place over PCIe. FMI_ERR_INVALID for pageable or straddling ranges. */
int fmi_host_device_ptr(const void* host, size_t bytes, void** dev);
/* 1 if [host, host + bytes) lies wholly inside one page-locked, device-mapped range, else 0 (also before
 * fmi_dev_init). A query, not a request: it never sets fmi_last_error (the Communicator asks it per host combine,
 * where a pageable bucket is the ordinary answer, ChannelPolicy::host_combine_on_device). */
int fmi_host_page_locked(const void* host, size_t bytes);
int fmi_dev_h2d_async(void* dst, const void* src, size_t bytes, fmi_stream_t stream);
int fmi_dev_d2h_async(void* dst, const void* src, size_t bytes, fmi_stream_t stream);
int fmi_dev_d2d_async(void* dst, const void* src, size_t bytes, fmi_stream_t stream);
int fmi_dev_memset_async(void* dst, int value, size_t bytes, fmi_stream_t stream);

/* ---- streams / events (timing is taken on the stream the kernels run on) ----------------------- */
int fmi_stream_create(fmi_stream_t* stream);
int fmi_stream_destroy(fmi_stream_t stream);
int fmi_stream_sync(fmi_stream_t stream);
int fmi_event_create(fmi_event_t* event);
int fmi_event_destroy(fmi_event_t event);
int fmi_event_record(fmi_event_t event, fmi_stream_t stream);
int fmi_event_sync(fmi_event_t event);
/* Work enqueued on `stream` after this call waits for `event`'s last record (cross-stream ordering, e.g.
 * a combine on one stream feeding a collective on another). */
int fmi_stream_wait_event(fmi_stream_t stream, fmi_event_t event);
int fmi_event_elapsed_ms(float* ms, fmi_event_t start, fmi_event_t stop);

/* ---- HIP graphs: a launch-bound sequence (many small bucket combines, e.g. FMI's 1 MiB messages) is
 * recorded once and replayed as one submission. Between capture_begin and capture_end on a stream made by
 * fmi_stream_create, calls on that stream are recorded, not run. Capture-safe: fmi_dev_reduce_pair,
 * fmi_dev_combine, the d2d / memset copies, and fmi_dev_reduce_tree / fmi_dev_scan_peers up to 16 peers
 * (one fused kernel each) on 16-B aligned f32 / f64 / i32 / i64 / f16 / bf16 buckets, at every algorithm: for
 * FMI_F16 / FMI_BF16 that includes FMI_ALG_REDUCE_LTR and FMI_ALG_SCAN_LTR. FMI_ACC_F32 calls at P <= 16 on aligned buckets are capture-safe (one fused
 * kernel each); beyond 16 peers or on unaligned buckets they need the f32 temporaries and are not. FMI_OP_AVG at
 * P <= 16 on aligned buckets is capture-safe (one fused kernel); beyond that it is capture-safe exactly where the
 * FMI_OP_SUM call is (the scale runs in place and needs no temporary), and with FMI_ACC_F32 beyond 16 peers or on
 * unaligned buckets it is not. fmi_dev_mean_scale and fmi_dev_convert are capture-safe. The 8-bit floats: the pairwise
 * calls are capture-safe, and so are the FMI_ACC_F32 calls (FMI_OP_AVG with the flag included) at P <= 16 on aligned
 * buckets (one fused kernel each); PLAIN FMI_F8E4M3 / FMI_F8E5M2 P-way calls at P > 1 run as pairwise passes through
 * the scratch arena and are not. Beyond 16 peers a call on such buckets
 * is capture-safe exactly where it needs no temporary bucket, which at FMI_TUNE_BLOCKS_ONE_PASS = 1 (the default)
 * is, the same for the six dtypes: FMI_ALG_ALLREDUCE at P <= 31 and P = 32, 48, 64, 80, 96, 112; FMI_ALG_REDUCE at
 * P <= 128; FMI_ALG_SCAN at P <= 143; FMI_ALG_SCAN_LTR at any P; FMI_ALG_REDUCE_LTR at P <= 128, and beyond when
 * `out` is none of ins[128..P). Everything else (host-ingress paths, communicators, other P-way programs, unaligned
 * buckets and the 8/16-bit integers at P > 1, which may allocate or synchronise) is not: that call or capture_end
 * fails, the graph is discarded, and the stream must be destroyed and replaced (HIP leaves a stream whose capture
 * was invalidated unusable). Pointers and sizes are frozen in the graph; replays recompute the same buckets. */
typedef void* fmi_graph_t;
int fmi_graph_capture_begin(fmi_stream_t stream);
int fmi_graph_capture_end(fmi_stream_t stream, fmi_graph_t* graph);
int fmi_graph_launch(fmi_graph_t graph, fmi_stream_t stream);
int fmi_graph_destroy(fmi_graph_t graph);

/* ---- the hot path ------------------------------------------------------------------------------ */
/* Pairwise bucket combine: inout[i] = op(inout[i], in[i]) for i < n.
 * Replaces one application of the raw_func built by Communicator::convert_to_raw_function
 * (reference include/Communicator.h:180-189) at the PeerToPeer combine sites
 * (reference src/comm/PeerToPeer.cpp:51,72,103,119,147,160,179). inout == in is allowed. */
int fmi_dev_reduce_pair(int op, int dtype, void* inout, const void* in, size_t n, fmi_stream_t stream);

/* Batched pairwise combine: for every descriptor k, descs[k].inout[i] = op(inout[i], in[i]) for
 * i < descs[k].n, all of them in as few launches as possible (up to 64 descriptors per launch): the same
 * bits as `count` calls of fmi_dev_reduce_pair, without a launch and its ramp per bucket — for many small
 * buckets (FMI's 1 MiB messages). `descs` is host memory, read during the call. A descriptor's inout must
 * not overlap another descriptor's inout or in (FMI_ERR_INVALID); inout == in is allowed. n = 0 entries are
 * skipped; unaligned or very large buckets are combined by their own launch. Graph-capturable. */
typedef struct {
    void* inout;
    const void* in;
    size_t n;
} fmi_pair_desc_t;
int fmi_dev_reduce_pair_batch(int op, int dtype, const fmi_pair_desc_t* descs, int count, fmi_stream_t stream);

/* Out-of-place pairwise combine: out[i] = op(a[i], b[i]); out may alias a or b. */
int fmi_dev_combine(int op, int dtype, void* out, const void* a, const void* b, size_t n,
                    fmi_stream_t stream);

/* P-way reduction of P device buckets in one pass with the evaluation order of `alg`
 * (FMI_ALG_ALLREDUCE / FMI_ALG_REDUCE / FMI_ALG_REDUCE_LTR): out = the value peer `rank` holds at the
 * end of the reference collective (for FMI_ALG_REDUCE `rank` is the root; for ALLREDUCE it selects
 * whose operand order is reproduced, which differs only for float MAX/MIN on signed zeros).
 * Replaces the whole chain of f.f calls of reference PeerToPeer::allreduce_no_order / reduce_no_order /
 * reduce_ltr (src/comm/PeerToPeer.cpp:96-130, :59-84, :44-57) for buckets that sit on one device.
 * ins[p] = bucket of peer p (p < P); out may alias any ins[p]. Any P >= 1 (no peer cap, as in the
 * reference). One fused kernel (a single
 * pass over the P buckets) for P <= 16, and for ALLREDUCE up to 31; larger P as fused sub-programs of the
 * identical order over blocks of 16 peers (every input read once, plus one write and one read per block
 * value). The single-pass kernels exist for f32 / f64 / i32 / i64 / f16 / bf16; unaligned buckets and the 8/16-bit
 * integers run the same order as pairwise passes. */
int fmi_dev_reduce_tree(int op, int dtype, int alg, void* out, const void* const* ins, int P, int rank,
                        size_t n, fmi_stream_t stream);

/* The scale step of FMI_OP_AVG alone, in place: inout[i] = store(fl_V(value(inout[i]) x r_P)), r_P = fl_V(1 / P), as
 * defined at FMI_OP_AVG, for callers who ran FMI_OP_SUM through an exchange of their own. dtype: FMI_F32, FMI_F64,
 * FMI_F16, FMI_BF16, FMI_F8E4M3 or FMI_F8E5M2 (anything else, FMI_ACC_F32 included: FMI_ERR_INVALID); P >= 1 (P = 1 leaves the bits
 * unchanged); any alignment (16-B nontemporal accesses on a 16-B aligned bucket, one element per thread otherwise);
 * n = 0 succeeds. One launch, graph-capturable. */
int fmi_dev_mean_scale(int dtype, void* inout, size_t n, int P, fmi_stream_t stream);

/* Element-type conversion: dst[i] = narrow_dst(widen_src(src[i])) for i < n. Both dtypes are among FMI_F32, FMI_F16,
 * FMI_BF16, FMI_F8E4M3, FMI_F8E5M2 (anything else, FMI_ACC_F32 included: FMI_ERR_INVALID). The value goes through f32:
 * widening is exact, so there is one rounding in all, the narrowing defined at fmi_dtype_t (round-to-nearest-even,
 * subnormals kept, NaN stays NaN; to the 8-bit floats non-saturating). Equal dtypes: a copy of the bits. dst == src is
 * allowed at equal element size; otherwise the two must not overlap. Any alignment (16-B nontemporal accesses where
 * both pointers are 16-B aligned, one element per thread otherwise); n = 0 succeeds. One launch, graph-capturable.
 * It is FMI_ACC_F32's fallback conversion made public: how f32 / bf16 data gets into an 8-bit float bucket. */
int fmi_dev_convert(int dst_dtype, void* dst, int src_dtype, const void* src, size_t n, fmi_stream_t stream);

/* Scaled P-way sum of 8-bit float buckets: what an FP8 gradient bucket with per-producer scales needs, in one pass.
 * dtype: FMI_F8E4M3 or FMI_F8E5M2, the storage type of every ins[p] (FMI_ACC_F32 is accepted and dropped: the call is
 * f32-valued by definition). in_scales: P f32 values in DEVICE memory, in_scales[p] the scale of ins[p]; out_scale
 * (NULL = 1.0f) and amax (NULL = not wanted): one f32 each in device memory. They live on the device so that a captured
 * graph picks up new scales on replay and delayed-scaling code never synchronises. Per element, with s_p = in_scales[p]
 * and t = *out_scale:
 *     v_p  = fl32( widen(x_p) * s_p )                  one IEEE f32 multiply per input
 *     S    = F32_program_alg( v_0 .. v_{P-1} )         the FMI_F32 SUM program of `alg`, the same bracketing
 *     amax = umax over the elements of bits(|S|), folded into what *amax held
 *     out  = narrow_dtype( fl32( S * t ) )             if out_dtype == dtype (the non-saturating narrowing above)
 *     out  =               fl32( S * t )               if out_dtype == FMI_F32
 * Every operation is round-to-nearest-even with subnormals kept and no contraction: the multiply by s_p is not fused
 * into the add that follows it, the multiply by t not into the narrowing. amax is of S, BEFORE the output scale (the
 * convention of delayed scaling), and is defined on the bit patterns of |S| compared as unsigned integers: it does not
 * depend on any order (deterministic), and a NaN in S wins and gives some NaN. *amax is read-modify-written: the caller
 * zeroes it and may accumulate over several buckets; it must hold a non-negative float or a NaN on entry.
 * Valid: op FMI_OP_SUM only (FMI_OP_AVG: FMI_ERR_INVALID, fold 1/P into out_scale; PROD / MAX / MIN: FMI_ERR_INVALID);
 * alg FMI_ALG_ALLREDUCE, _REDUCE or _REDUCE_LTR with `rank` as in fmi_dev_reduce_tree; out_dtype == dtype or FMI_F32;
 * P >= 1, and P = 1 is NOT a copy: out = narrow(fl32(fl32(widen(x) * s_0) * t)). All of it is checked on the host before
 * a device is needed. out may alias an ins[p] only where out_dtype == dtype.
 * 2 <= P <= 16 with every bucket 16-B aligned: ONE fused kernel (P reads, one store, at most one atomic per
 * workgroup), graph-capturable. Any other call (P = 1, P > 16, unaligned buckets) widens and scales every input into an
 * f32 temporary (FMI_ACC_F32's allocation: not capturable), runs the library's own FMI_F32 program on those and one
 * finishing kernel (amax, x t, narrow or store): the same bits by construction. Additive: fmi_abi_version() stays 1. */
int fmi_dev_reduce_tree_scaled(int op, int dtype, int alg, int out_dtype, void* out, const void* const* ins,
                               const float* in_scales, const float* out_scale, float* amax, int P, int rank, size_t n,
                               fmi_stream_t stream);

/* Block-scaled (MX) 8-bit float buckets: the OCP Microscaling layout, one power-of-two scale byte (E8M0) per 32
 * consecutive elements. An MX bucket of n elements is two arrays: n element bytes (FMI_F8E4M3 or FMI_F8E5M2, the
 * encodings above) and ceil(n / 32) scale bytes; block b covers elements 32 b .. min(32 b + 31, n - 1), so the last
 * block may be ragged. A scale byte e decodes to the f32 scale32(e):
 *     e in 1..254: the f32 with bits e << 23, 2^(e - 127);   e = 0: bits 0x00400000, 2^-127 (an f32 subnormal);
 *     e = 255: NaN                                            (torch.float8_e8m0fnu -> float32 on every byte)
 * fmi_dev_reduce_tree_mx: the sum or mean of P MX buckets in one pass. Per element i of block b:
 *     v_p   = fl32( widen(x_p[i]) * scale32(e_p[b]) )      exact, or +-inf on overflow, or NaN (e = 255)
 *     S     = F32_program_alg( v_0 .. v_{P-1} )             the FMI_F32 SUM program of `alg`, the same bracketing
 *     S     = fl32( S * r_P )                               FMI_OP_AVG only, r_P = fl32(1 / P) as at FMI_OP_AVG
 *     out_dtype == FMI_F32:   out[i] = S                    no output scales
 *     out_dtype == dtype:     per block b
 *         A      = umax over the block's existing elements of bits(|S|)     unsigned compare, a NaN wins
 *         f, m   = A >> 23, A & 0x7FFFFF
 *         e_out  = 255                                   if f == 255 (the block holds an inf or a NaN)
 *                = max( f - EMAX + (m > 0x600000), 0 )   otherwise;  EMAX = 8 for E4M3, 15 for E5M2
 *         out_scales[b] = e_out
 *         out[i] = 0x7F                                          if e_out == 255 (the whole block is NaN, as MX says)
 *                = narrow( fl32( S * bits((254 - e_out) << 23) ) )   otherwise: the non-saturating narrowing above
 * e_out is the smallest power of two that brings the block's largest magnitude to at most the largest finite element
 * (448 = 1.75 * 2^8, 57344 = 1.75 * 2^15: mantissa bits 0x600000): the round-up rule of MXFP8 recipes, not the floor of
 * the OCP example, under which elements in (448, 512) * 2^E would need a saturating narrowing. With round-up no
 * element of a finite block overflows, nothing is clipped at the block's maximum, e_out stays within 0..247 (0..240)
 * and the inverse scale is a normal f32. Every operation is round-to-nearest-even with subnormals kept and no
 * contraction; the result does not depend on any order beyond the program's bracketing (deterministic, no atomics).
 * Valid: op FMI_OP_SUM or FMI_OP_AVG (PROD / MAX / MIN: FMI_ERR_INVALID); alg FMI_ALG_ALLREDUCE, _REDUCE or _REDUCE_LTR
 * with `rank` as in fmi_dev_reduce_tree (the scans: FMI_ERR_INVALID); dtype one of the two 8-bit floats, or FMI_F4E2M1
 * (MXFP4, below) (FMI_ACC_F32 is accepted and dropped); out_dtype == dtype or FMI_F32; out_scales may be NULL only with FMI_F32; P >= 1, and P = 1 is
 * NOT a copy: it requantizes. All of it is checked on the host before a device is needed. ins[p] / in_scales[p]: peer
 * p's elements and scale bytes. out may alias an ins[p], and out_scales an in_scales[p], where out_dtype == dtype.
 * 2 <= P <= 16 with the element buckets 16-B aligned (scale arrays: any alignment): ONE fused kernel, graph-capturable,
 * no atomics, no temporaries. Any other call (P = 1, P > 16, unaligned buckets) dequantizes every input into an f32
 * temporary (FMI_ACC_F32's allocation: not capturable), runs the library's own FMI_F32 program and quantizes: the same
 * bits by construction. Additive: fmi_abi_version() stays 1.
 *
 * MXFP4: dtype FMI_F4E2M1 (the encoding and packing at fmi_dtype_t). An MXFP4 bucket of n elements is ceil(n / 2)
 * element bytes and ceil(n / 32) scale bytes; n counts ELEMENTS in every MX call. The text above holds with three
 * type-specific pieces:
 *   - widen is the 16-entry table; v_p = fl32(widen(x) * scale32(e)) is exact except 2 * 2^127 and above, which give
 *     +-inf; e = 255 gives NaN for every nibble, zeros included; e = 0 is 2^-127, so 0.5 * 2^-127 is the subnormal 2^-128;
 *   - EMAX = 2: the largest finite element is 6 = 1.5 * 2^2 (mantissa bits 0x400000), so
 *         e_out = 255 if f == 255, otherwise max( f - 2 + (m > 0x400000), 0 )
 *     e_out <= 253 for a finite block, the inverse scale is a normal f32 and |S * inv| <= 6 for every element;
 *   - a block with e_out == 255 stores the scale byte 255 and every element nibble as 0 (E2M1 has no NaN; by the MX
 *     rule a NaN scale makes the block NaN, and dequantizing it gives NaN by the multiply above).
 * out_dtype == FMI_F4E2M1 or FMI_F32; the fused kernel needs the element buckets 16-B aligned (a block of 32 elements is
 * one 16-B word); the fallback and the two conversions take any BYTE alignment. out may alias an input where the types
 * agree. No byte beyond ceil(n / 2) and no scale byte beyond ceil(n / 32) is touched.
 *
 * MXFP6: dtype FMI_F6E2M3 or FMI_F6E3M2 (the encodings and the packing at fmi_dtype_t). A bucket of n elements is
 * ceil(3 n / 4) element bytes and ceil(n / 32) scale bytes; n counts ELEMENTS in every MX call. The text above holds
 * with these type-specific pieces:
 *   - widen is the 64-entry table; e = 255 gives NaN for every code, zeros included; e = 0 is 2^-127;
 *   - E2M3: e_out = 255 if f == 255, otherwise max( f - 2 + (m > 0x700000), 0 )   (7.5 = 1.875 * 2^2)
 *     E3M2: e_out = 255 if f == 255, otherwise max( f - 4 + (m > 0x600000), 0 )   (28 = 1.75 * 2^4)
 *     so a finite block has e_out <= 253 (E2M3) or <= 251 (E3M2), a normal inverse scale, and |S * inv| <= the largest
 *     element;
 *   - a block with e_out == 255 stores the scale byte 255 and every code 0; it dequantizes to NaN through the scale;
 *   - stochastic rounding (below): narrow_sr with (M, EMIN) = (3, 0) for E2M3 and (2, -2) for E3M2; the stream
 *     positions, first % 32 == 0 and the scale bytes are as for the other types.
 * out_dtype == dtype or FMI_F32; the fused kernel needs the element buckets 16-B aligned (a lane takes two blocks, 48 B);
 * the fallback and the two conversions take any BYTE alignment. out may alias an input where the types agree. No byte
 * beyond ceil(3 n / 4) and no scale byte beyond ceil(n / 32) is touched. */
int fmi_dev_reduce_tree_mx(int op, int dtype, int alg, int out_dtype, void* out, void* out_scales, const void* const* ins,
                           const void* const* in_scales, int P, int rank, size_t n, fmi_stream_t stream);
/* The fallback's two kernels made public, as fmi_dev_convert is. The non-MX side (src_dtype / dst_dtype) is FMI_F32,
 * FMI_F16 or FMI_BF16. Quantize: the out_dtype == dtype branch above applied to S = widen(src[i]) (exact). Dequantize:
 * dst[i] = narrow_dst( fl32( widen(src[i]) * scale32(src_scales[i / 32]) ) ). Any alignment, n = 0 succeeds, one launch
 * each, graph-capturable. dtype FMI_F4E2M1: the packed MXFP4 side, n counting elements ((n + 1) / 2 bytes; an odd
 * bucket's last high nibble is written 0 by quantize and ignored by dequantize), any byte alignment. */
int fmi_dev_mx_quantize(int dtype, void* out, void* out_scales, int src_dtype, const void* src, size_t n, fmi_stream_t stream);
int fmi_dev_mx_dequantize(int dst_dtype, void* dst, int dtype, const void* src, const void* src_scales, size_t n, fmi_stream_t stream);

/* Stochastic rounding (SR) for the MX calls: fmi_dev_reduce_tree_mx with out_dtype == dtype, and fmi_dev_mx_quantize,
 * with the last step alone changed. v_p, the f32 program S, the mean's r_P, the block's scale byte e_out (so every scale
 * byte equals the round-to-nearest call's) and y = fl32(S * 2^(127 - e_out)) are as defined above; narrow(y) becomes
 * narrow_sr(y, r), r a 16-bit random integer that belongs to the ELEMENT, a pure function of (seed, stream position):
 *     element i of the output has the stream position j = first + i (u64);  q = j >> 3
 *     (W0, W1, W2, W3) = Philox4x32-10( counter (q & 0xFFFFFFFF, q >> 32, 0, 0), key (seed & 0xFFFFFFFF, seed >> 32) )
 *         one round: (c0, c1, c2, c3) <- ( hi32(M1 c2) ^ c1 ^ k0, lo32(M1 c2), hi32(M0 c0) ^ c3 ^ k1, lo32(M0 c0) ), then
 *         k0 += 0x9E3779B9, k1 += 0xBB67AE85;  M0 = 0xD2511F53, M1 = 0xCD9E8D57;  ten rounds
 *         (counter 0, key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8)
 *     r = ( W[(j & 7) >> 1] >> (16 * (j & 1)) ) & 0xFFFF            one Philox call serves 8 consecutive elements
 * narrow_sr, for the finite |y| <= the largest finite element that the scale rule guarantees (SR cannot overflow): G the
 * ascending non-negative finite magnitudes of the type (E2M1: 8; E4M3: codes 0x00..0x7E; E5M2: codes 0x00..0x7B);
 *     lo = max{ g in G : g <= |y| };  |y| == lo: the magnitude is lo, whatever the seed (a grid value never moves);
 *     otherwise hi = the next element of G, T = 65536 (|y| - lo) / (hi - lo)  (exact), and the magnitude is hi if
 *     r + 0.5 < T, else lo.  The code's sign bit is y's, -0 included.
 * So P(up) = round(T) / 65536 and the expectation lies within 2^-17 of a grid step of |y|. A block with e_out == 255
 * stores what the round-to-nearest call stores (0x7F bytes, zero nibbles). An equal form in integers: with (M, EMIN) =
 * (1, 0) for E2M1, (3, -6) for E4M3, (2, -14) for E5M2, e the unbiased exponent of |y| (-126 for a subnormal) and sig its
 * 24-bit significand (no implicit bit for a subnormal):
 *     d = 23 - M + max(EMIN - e, 0);  D = sig mod 2^d;  up = ((2 r + 1) << (d - 17)) < D  (never once d - 17 >= 24);
 *     the result's significand is (sig >> d) + up at the exponent max(e, EMIN).
 * The result does not depend on the access policy, the grid, the fused / fallback route, or on how a bucket is split
 * between calls at multiples of 32 elements (the second call passes first + the elements before it).
 * fmi_dev_reduce_tree_mx_sr: fmi_dev_reduce_tree_mx's dtypes, ops, algs, P, rank and aliasing rules, the output of the
 * input's dtype (an f32 output has nothing to round). seed: ONE u64 in DEVICE memory, 8-byte aligned (the kernels read
 * it with one load), so a captured graph replays with whatever the word then holds and nobody synchronises; first: a
 * host value. FMI_ERR_INVALID on the host, before a device is needed: seed == NULL or not 8-byte aligned, first % 32 != 0,
 * first + n wrapping 2^64, and everything the round-to-nearest call refuses. n = 0 succeeds. 2 <= P <= 16 with 16-B
 * aligned element buckets: one fused kernel, graph-capturable; any other call runs dequantize, the f32 program and
 * fmi_dev_mx_quantize_sr at the same `first`.
 * fmi_dev_mx_quantize_sr: fmi_dev_mx_quantize with narrow_sr; the same checks. Additive: fmi_abi_version() stays 1. */
int fmi_dev_reduce_tree_mx_sr(int op, int dtype, int alg, void* out, void* out_scales, const void* const* ins,
                              const void* const* in_scales, const uint64_t* seed, uint64_t first, int P, int rank, size_t n,
                              fmi_stream_t stream);
int fmi_dev_mx_quantize_sr(int dtype, void* out, void* out_scales, int src_dtype, const void* src, size_t n, const uint64_t* seed,
                           uint64_t first, fmi_stream_t stream);
/* fmi_dev_mx_quantize_sr from FMI_F32 on HOST memory, in plain C++ from the functions the kernels use: the same bytes.
 * `seed` is the value itself. Needs no device: a CPU check of the definition above. dtype, first and n are checked as
 * there; out holds n bytes (FMI_F4E2M1: ceil(n / 2), an odd bucket's last high nibble written 0), out_scales
 * ceil(n / 32). */
int fmi_host_mx_quantize_sr(int dtype, void* out, void* out_scales, const float* src, size_t n, uint64_t seed, uint64_t first);

/* Peer-axis inclusive scan of P device buckets: outs[k] = x0 (+) ... (+) xk with the evaluation order
 * of `alg` (FMI_ALG_SCAN or FMI_ALG_SCAN_LTR). Replaces reference PeerToPeer::scan_no_order / scan_ltr
 * (src/comm/PeerToPeer.cpp:154-184, :141-152) and Communicator::scan (include/Communicator.h:135-150)
 * when the P buckets sit on one device. outs[k] may alias ins[k]. Any P >= 1: one fused pass up to 31
 * peers; beyond, every input is read at most twice (block totals, then the blocks continued from their
 * carry). The same dtypes as fmi_dev_reduce_tree have these kernels (f16 / bf16 included, at both algorithms);
 * unaligned buckets and the 8/16-bit integers run the same order as pairwise passes. */
int fmi_dev_scan_peers(int op, int dtype, int alg, void* const* outs, const void* const* ins, int P,
                       size_t n, fmi_stream_t stream);

/* Host-resident pairwise combine through the device: pinned (or pageable) host `inout`/`in` are
 * streamed through device staging in chunks (H2D, kernel, D2H overlapped on two streams).
 * This is the path a recv buffer arriving over a host channel takes (reference
 * src/comm/Direct.cpp:36-45 → PeerToPeer.cpp:119). Synchronous: returns when inout is updated. */
int fmi_host_reduce_pair(int op, int dtype, void* inout, const void* in, size_t n);

/* ---- sharded device collectives across GPUs (one process per GPU, RCCL over xGMI) ----------------
 * The reference's collectives exchange whole buckets peer to peer over host sockets
 * (src/comm/PeerToPeer.cpp). Between MI355X GPUs the same collectives run sharded, so every GPU's 7
 * xGMI links carry traffic at once, with the combine done by the fused kernels above in the reference's
 * order:
 *   allreduce (path TREE): all-to-all of N shards -> fused P-way kernel over the N partials of this
 *       GPU's shard (allreduce_no_order / reduce_ltr order) -> all-gather. Bit-identical to the
 *       reference's N-peer allreduce on every rank, each rank with its OWN operand order: for float
 *       max/min (whose ±0 ties and NaNs depend on it) the shard owner computes its shard in every rank's
 *       order and an all-to-all replaces the all-gather, so rank r receives what reference peer r holds.
 *   allreduce (path RCCL): RCCL reduce-scatter + all-gather (RCCL's order; within (N-1)*u*sum|x|).
 *   reduce: all-to-all -> fused kernel in reduce_no_order / reduce_ltr order for `root` -> gather.
 *   scan:   all-to-all -> fused peer-axis scan -> all-to-all back.
 * One rank = one peer = one GPU. Transports: FMI_TRANSPORT_RCCL (librccl, loaded on first use; with
 * torch imported first it is torch's copy), FMI_TRANSPORT_LOCAL (ranks are threads of ONE process
 * sharing one device: the same schedules over device-to-device copies — used to test the multi-rank
 * schedules on a single GPU and to serve several peers co-resident on one GPU) and FMI_TRANSPORT_PROC
 * (ranks are processes of one node, on the same or different GPUs: data staged through a page-locked
 * POSIX shared-memory segment, windows mapped with HIP IPC — the same schedules again, so multi-process
 * runs, FMI_PATH_DIRECT's cross-process mappings included, are testable on a single GPU).
 * All calls enqueue on `stream` (NULL = library stream); results are valid after fmi_stream_sync.
 * Buckets are device pointers; recv may alias send.
 * Side effect on `send` — a deliberate divergence from the reference: the reference's commutative
 * allreduce / scan leave the result in the caller's sendbuf and its reduce leaves partials in interior
 * peers' sendbufs (src/comm/PeerToPeer.cpp:72,103,119,160,179). Here `send` is never modified by
 * allreduce, reduce or scan, so a C-ABI caller that relied on the clobber passes recv == send (allreduce,
 * scan) to get it. The C++ channel FMI::Comm::Rccl (fmi_amd/cpp/include/fmi/comm/Rccl.h) restores the
 * reference's side effects itself, so Communicator callers see the reference behaviour. */
#define FMI_COMM_ID_BYTES 128
typedef void* fmi_comm_t;
typedef enum { FMI_TRANSPORT_RCCL = 0, FMI_TRANSPORT_LOCAL = 1, FMI_TRANSPORT_PROC = 2 } fmi_transport_t;
/* FMI_PATH_DIRECT: no RCCL data movement. `send` must lie in a window (fmi_comm_window_alloc) at the SAME
 * byte offset and with the same n on every rank: rank k reads every peer's window at its own offset (windows
 * are equal-sized, so a mismatch reads wrong data, never outside a window). With FMI_CHECK_DIRECT=1 in the
 * environment every call first compares the (offset, n) pairs across ranks (a blocking all-reduce) and a
 * mismatch fails the call on every rank with FMI_ERR_INVALID. Rank k's fused kernel reads shard k of every rank's window over xGMI (IPC-mapped peer
 * memory) and reduces it in the reference's order, then every rank reads the N reduced shards from the
 * peers' windows. Bit-identical to FMI_PATH_TREE. */
typedef enum { FMI_PATH_TREE = 0, FMI_PATH_RCCL = 1, FMI_PATH_DIRECT = 2 } fmi_path_t;

/* A fresh communicator id (FMI_COMM_ID_BYTES) made by one rank and handed to the others by any host
 * channel (FMI: Communicator::bcast over the host channel, reference include/Communicator.h:43-47). */
int fmi_comm_unique_id(int transport, void* id, size_t len);
/* Timeouts. Every wait of a communicator for its peers is bounded by its timeout: the rendezvous of
 * fmi_comm_init (RCCL: non-blocking ncclCommInitRankConfig, polled), the transport's own host-side waits
 * (PROC / LOCAL barriers and mailboxes, RCCL barriers and window setup) and fmi_comm_sync. On expiry the
 * call returns FMI_ERR_TIMEOUT and the communicator is aborted (RCCL: ncclCommAbort, which also ends its
 * kernels still waiting for the absent peer). fmi_comm_init uses FMI_COMM_TIMEOUT_S from the environment
 * (seconds; for PROC also FMI_PROC_TIMEOUT_S), default 300; fmi_comm_init_timeout takes it explicitly
 * (timeout_s <= 0: that default). An asynchronous transport error seen while waiting (RCCL
 * ncclCommGetAsyncError: a peer's connection failed) also aborts the communicator, with FMI_ERR_COMM. */
int fmi_comm_init(fmi_comm_t* comm, const void* id, int nranks, int rank);
int fmi_comm_init_timeout(fmi_comm_t* comm, const void* id, int nranks, int rank, double timeout_s);
int fmi_comm_destroy(fmi_comm_t comm);
int fmi_comm_size(fmi_comm_t comm, int* nranks, int* rank);
/* Wait until the work enqueued on `stream` (NULL = library stream) has completed — the blocking point of
 * the collectives, which enqueue asynchronously — within the communicator's timeout, polling the transport
 * for asynchronous errors (FMI_ERR_TIMEOUT / FMI_ERR_COMM as above). */
int fmi_comm_sync(fmi_comm_t comm, fmi_stream_t stream);
/* What the transport itself reports: RCCL ncclCommCount / ncclCommUserRank / ncclCommCuDevice (the device
 * RCCL bound this rank to); LOCAL / PROC the communicator's size, rank and the calling thread's device.
 * Lets a caller prove the topology it runs on (bench.py: RCCL saw N ranks on N distinct GPUs). */
int fmi_comm_query(fmi_comm_t comm, int* count, int* rank, int* device);
/* The librccl the RCCL transport uses (loaded on first use: with torch imported first, torch's copy): its
 * ncclGetVersion (0 if it lacks the symbol) and the real path of the mapped object, NUL-terminated into
 * path. FMI_ERR_COMM if librccl cannot be loaded. Lets a failed multi-GPU run name the RCCL it ran on. */
int fmi_comm_rccl_info(int* version, char* path, size_t len);
/* Symmetric window for FMI_PATH_DIRECT (collective: every rank calls it with the same `bytes`). Returns a
 * device bucket of `bytes` that every peer of the communicator can read directly (RCCL transport: HIP IPC
 * handles exchanged by all-gather, mapped with peer access over xGMI). All-or-nothing: if any rank cannot
 * allocate, export or map, every rank gets an error. Freed (collectively) by fmi_comm_window_free or with
 * the communicator: both first wait for all work on this rank's device (any stream may still be reading
 * a peer's window through its mapping), then barrier with the peers, then unmap and free. */
int fmi_comm_window_alloc(fmi_comm_t comm, size_t bytes, void** ptr);
int fmi_comm_window_free(fmi_comm_t comm, void* ptr);
/* Live timing of the collectives' shard kernels (the fused P-way kernel each rank runs on its shard, path
 * TREE / DIRECT allreduce): while enabled, an event pair is recorded around every such launch on the stream
 * it runs on (up to 8192 launches). fmi_comm_timing_read waits for them and returns the summed kernel time
 * and the launch count, then starts a new tally. Enabling also starts a new tally. */
int fmi_comm_timing(fmi_comm_t comm, int enable);
int fmi_comm_timing_read(fmi_comm_t comm, float* total_ms, int* launches);
/* alg: FMI_ALG_ALLREDUCE (commutative+associative) or FMI_ALG_REDUCE_LTR (ordered) */
int fmi_comm_allreduce(fmi_comm_t comm, int op, int dtype, int alg, int path, const void* send, void* recv, size_t n,
                       fmi_stream_t stream);
/* The sharded allreduce of scaled 8-bit float buckets (fmi_dev_reduce_tree_scaled above): path TREE, unpipelined, on
 * every transport. op: FMI_OP_SUM; dtype, out_dtype as there; alg: FMI_ALG_ALLREDUCE or FMI_ALG_REDUCE_LTR. `send` holds
 * n elements of dtype, `recv` n of out_dtype; in_scale is this rank's ONE scale, out_scale (NULL = 1.0f) and amax (NULL =
 * not wanted) one f32 each, all in device memory. The input shards travel as 8-bit bytes; the N scales are all-gathered
 * (4 bytes per rank) into rank order; each owner runs fmi_dev_reduce_tree_scaled at P = N, rank 0, on its shard's true
 * length (no padding reaches amax); the result shards are all-gathered at out_dtype's element size; the owners' shard
 * amax words are all-gathered and folded, with what *amax held, into *amax: every rank ends with the same amax. Every
 * rank's recv is the program of `alg` over v_p in rank order. out_scale must hold the same value on every rank. `send`
 * is not modified. A one-rank communicator runs the P = 1 form. */
int fmi_comm_allreduce_scaled(fmi_comm_t comm, int op, int dtype, int alg, int out_dtype, const void* send,
                              const float* in_scale, void* recv, const float* out_scale, float* amax, size_t n,
                              fmi_stream_t stream);
/* The sharded allreduce of MX buckets (fmi_dev_reduce_tree_mx above): path TREE, unpipelined, on every transport. op:
 * FMI_OP_SUM or FMI_OP_AVG; dtype, out_dtype as there; alg: FMI_ALG_ALLREDUCE or FMI_ALG_REDUCE_LTR. `send` holds n
 * elements and send_scales ceil(n / 32) scale bytes; `recv` n elements of out_dtype and recv_scales ceil(n / 32) bytes
 * (NULL only with FMI_F32). The element shards travel as they do in fmi_comm_allreduce_scaled; the scale bytes travel
 * in a second all-to-all of shard / 32 bytes per shard: shards are multiples of 64 elements, so no block is split
 * between owners. Each owner runs fmi_dev_reduce_tree_mx at P = N, rank 0, on its shard's TRUE length (padding never
 * enters a block's amax); element and scale shards are then all-gathered. Every rank's recv / recv_scales is the
 * definition over the ranks' buckets in rank order. send / send_scales are not modified. A one-rank communicator runs
 * the P = 1 form. FMI_F4E2M1: the same route at half the element bytes (a shard of 64 k elements is 32 k bytes); only the
 * last non-empty shard can have an odd true length. FMI_F6E2M3 / FMI_F6E3M2: the same route at three quarters of the
 * element bytes (a shard of 64 k elements is 48 k bytes: whole blocks, whole bytes, 16-B aligned); only the last
 * non-empty shard can be ragged. */
int fmi_comm_allreduce_mx(fmi_comm_t comm, int op, int dtype, int alg, int out_dtype, const void* send,
                          const void* send_scales, void* recv, void* recv_scales, size_t n, fmi_stream_t stream);
/* fmi_comm_allreduce_mx with stochastic rounding (fmi_dev_reduce_tree_mx_sr above): the same route, the output of the
 * input's dtype. Each owner runs the device call on its shard at first + the shard's offset in the bucket (shards are
 * multiples of 64 elements, so that stays a multiple of 32). Every rank must hold the same value in its device word
 * `seed` and pass the same `first`; every rank's recv / recv_scales is then the single-device call over the ranks'
 * buckets at (seed, first). seed == NULL or misaligned, first % 32 != 0 and first + n wrapping 2^64 are FMI_ERR_INVALID, checked with
 * the other arguments before a device is needed. */
int fmi_comm_allreduce_mx_sr(fmi_comm_t comm, int op, int dtype, int alg, const void* send, const void* send_scales, void* recv,
                             void* recv_scales, size_t n, const uint64_t* seed, uint64_t first, fmi_stream_t stream);
/* Host-ingress allreduce (BASELINE config C5): `send` / `recv` are HOST buckets, i.e. the channel recv
 * buffers FMI's transports deliver into (reference src/comm/Direct.cpp:36-45, PeerToPeer.cpp:110-129).
 * The bucket streams through the GPU in chunks of `chunk` elements (0 = FMI_TUNE_HOST_CHUNK bytes):
 * H2D of chunk k+1, the sharded allreduce of chunk k and D2H of chunk k-1 overlap on three streams.
 * Every rank must pass the same n and chunk. Page-locked buckets (fmi_host_pin_alloc) move at PCIe DMA
 * rate; pageable ones work but copy synchronously. Element-wise results are identical to
 * fmi_comm_allreduce over the whole bucket. Blocking: returns when `recv` holds the result. */
int fmi_comm_allreduce_host(fmi_comm_t comm, int op, int dtype, int alg, int path, const void* send, void* recv,
                            size_t n, size_t chunk);
/* alg: FMI_ALG_REDUCE or FMI_ALG_REDUCE_LTR; recv is used on root only (may be NULL elsewhere) */
int fmi_comm_reduce(fmi_comm_t comm, int op, int dtype, int alg, const void* send, void* recv, size_t n, int root,
                    fmi_stream_t stream);
/* fmi_comm_reduce with the reference's side effect on every rank's sendbuf (src/comm/PeerToPeer.cpp:59-84,
 * combine site :72): after the call rank r's `send` holds what reference peer r leaves in its sendbuf —
 * for FMI_ALG_REDUCE the partial it forwarded up the binomial tree (a leaf's own bucket, the root's
 * result), for FMI_ALG_REDUCE_LTR its own bucket unchanged (:44-57). recv (root only) gets the result, as
 * with fmi_comm_reduce. Costs N shard writes on each owner and an all-to-all back instead of a gather. */
int fmi_comm_reduce_sendbuf(fmi_comm_t comm, int op, int dtype, int alg, void* send, void* recv, size_t n, int root,
                            fmi_stream_t stream);
/* alg: FMI_ALG_SCAN or FMI_ALG_SCAN_LTR; rank k receives x0 (+) ... (+) xk */
int fmi_comm_scan(fmi_comm_t comm, int op, int dtype, int alg, const void* send, void* recv, size_t n,
                  fmi_stream_t stream);
int fmi_comm_bcast(fmi_comm_t comm, void* buf, size_t bytes, int root, fmi_stream_t stream);
/* recv holds nranks * bytes on root (rank order); scatter sends root's nranks * bytes */
int fmi_comm_gather(fmi_comm_t comm, const void* send, void* recv, size_t bytes, int root, fmi_stream_t stream);
int fmi_comm_scatter(fmi_comm_t comm, const void* send, void* recv, size_t bytes, int root, fmi_stream_t stream);
int fmi_comm_send(fmi_comm_t comm, const void* buf, size_t bytes, int peer, fmi_stream_t stream);
int fmi_comm_recv(fmi_comm_t comm, void* buf, size_t bytes, int peer, fmi_stream_t stream);
int fmi_comm_barrier(fmi_comm_t comm, fmi_stream_t stream);

/* ---- synthetic buckets (identical on host and device: SURVEY.md §8d generator) ------------------
 * h = splitmix64(seed ^ ((uint64)peer << 40) ^ i);  f32 = (float)((h >> 40) * 2^-24) * 2 - 1,
 * f64 = (double)((h >> 11) * 2^-53) * 2 - 1,  i32 = (int32)(h >> 32),  i64 = (int64)h.
 * The narrow floats take values exact in their storage type: f16 = (h >> 53) * 2^-11 * 2 - 1 (multiples of 2^-10),
 * bf16 = (h >> 56) * 2^-8 * 2 - 1 (multiples of 2^-7), E4M3 = (h >> 60) * 2^-4 * 2 - 1 (multiples of 2^-3),
 * E5M2 = (h >> 61) * 2^-3 * 2 - 1 (multiples of 2^-2): all in [-1, 1), each narrowed without rounding. */
int fmi_dev_fill_synthetic(int dtype, void* buf, size_t n, uint64_t seed, uint32_t peer,
                           fmi_stream_t stream);
/* Elements [first, first + n) of the same synthetic bucket (i runs from `first`): lets a rank rebuild any
 * window of every peer's bucket locally, e.g. to check a sharded collective's result on sampled ranges. */
int fmi_dev_fill_synthetic_at(int dtype, void* buf, size_t n, uint64_t seed, uint32_t peer, uint64_t first,
                              fmi_stream_t stream);

/* ---- schedule introspection (host-only logic, no device needed) --------------------------------
 * Writes the symbolic combine expression peer `rank` ends with, e.g. "((x0+x1)+(x2+x3))", as the
 * fused kernels evaluate it. Used by the parity tests to pin the order against the reference's. */
int fmi_schedule_expr(int alg, int P, int rank, char* buf, size_t len);

/* ---- tuning knobs (performance only, never semantics) ------------------------------------------ */
typedef enum {
    FMI_TUNE_PAIR_VARIANT = 0, /* 0 = one-shot tiles, 1 = grid-stride, 2 = nontemporal tiles (default),
                                  3 = tiles with nontemporal loads only, 4 = nontemporal stores only */
    FMI_TUNE_PAIR_UNROLL = 1,  /* 16-B vectors per thread per operand: 1, 2, 4, 8 */
    FMI_TUNE_BLOCK = 2,        /* threads per workgroup: 256, 512, 1024 */
    FMI_TUNE_GRID_PER_CU = 3,  /* workgroups per CU for the grid-stride variant */
    FMI_TUNE_HOST_CHUNK = 4,   /* bytes per chunk of fmi_host_reduce_pair's staged pipeline */
    FMI_TUNE_HOST_ZERO_COPY = 5, /* 1: page-locked host buckets are combined in place over PCIe by the
                                   kernel (no staging); 0: always the staged H2D/kernel/D2H pipeline */
    FMI_TUNE_FUSED_INFLIGHT_KIB = 6, /* fused P-way kernels (tree, scan): budget of peer-load bytes in
                                       flight per CU, in KiB; a workgroup of the P-way kernel loads
                                       4 KiB x P, so at most max(2, ceil(budget / (4 P))) workgroups stay
                                       resident per CU (an LDS reservation enforces it); 0 = no cap. Default 64
                                       (fewer concurrent HBM streams at large P) */
    FMI_TUNE_BLOCKS_ONE_PASS = 7, /* P-way programs beyond 31 peers in one pass over every input (default 1):
                                    scan_no_order over 32..143 peers, reduce_no_order over 17..128 peers
                                    (beyond: superblocks of 128, one pass each, up to 16384 peers),
                                    allreduce_no_order over 32 / 48 / 64 / 80 / 96 / 112 / 128
                                    peers (2^k >= 128 peers: superblocks of 64), scan_ltr and
                                    reduce_ltr over 32..128 peers (beyond: segments of 127 continued
                                    from the running value, any P);
                                    0 = the blocked launches (block values through temps; the scan reads
                                    the inputs of blocks >= 1 twice). Same bits either way */
    FMI_TUNE_COMM_A2A = 8,        /* RCCL transport all-to-all: 0 = ncclAllToAll where librccl has it (default),
                                    1 = grouped ncclSend / ncclRecv to every peer. Same bytes either way.
                                    EVERY rank of a communicator must use the same value: the two forms post
                                    different RCCL operations, and ranks that disagree hang (until the
                                    communicator's timeout) */
    FMI_TUNE_COMM_GATHER = 9,     /* RCCL transport all-gather: 0 = ncclAllGather (default), 1 = grouped
                                    ncclSend / ncclRecv of this rank's shard to every peer (each peer link
                                    carries one shard, no ring). Same bytes either way. EVERY rank must use the
                                    same value (as FMI_TUNE_COMM_A2A) */
    FMI_TUNE_COMM_PIPELINE = 10,  /* EXPERIMENTAL (not yet run over RCCL with more than one rank). Path TREE
                                    allreduce in K chunks (0 or 1 = off, default; 2..64): chunk k's
                                    all-gather runs on a second stream and a second communicator (made
                                    once: a fresh id broadcast over the first, then a bounded init)
                                    while chunk k + 1's all-to-all and kernel run; chunks of >= 1 MiB per
                                    rank only. If the second communicator cannot be made, the unpipelined path runs.
                                    Same bits (element-wise); EVERY rank must set the same K */
    FMI_TUNE_FUSED_POLICY = 11,   /* fused P-way kernels (tree, scan; <= 16 peers), 16-B accesses: 2 = buffer
                                    loads nt with sc1 (tree) / nt sc1 (scan) stores; 0 = global_load /
                                    global_store nt; 1 = auto (default): 2 for trees of >= 4 and scans of
                                    >= 8 peers, 0 otherwise (tools/ab_fused_policy.py). Same bits always */
    FMI_TUNE_PAIR_SC1_OF_8 = 12,  /* pairwise kernel (16-B aligned buckets, one-shot tiles): tiles t with
                                    t % 8 < k store with sc1 instead of nontemporal (k = 0..8). Consecutive
                                    workgroups are dispatched to different XCDs, so k of the 8 XCDs store sc1.
                                    Default 1 (tools/ab_pair_sc1.py, measured with no MALL re-use). Same bits
                                    always */
    FMI_TUNE_COMM_ONE_RANK_EXCHANGE = 13, /* 1: a ONE-rank communicator runs the full sharded schedule —
                                    all-to-all, shard kernel, all-gather / gather / all-to-all back, RCCL
                                    reduce-scatter, window mapping, the pipelined split — exchanging with
                                    itself, instead of the reference's P = 1 copy. Same bits; exists so that
                                    a 1-GPU box runs the RCCL transport's real collectives (tests). Default 0 */
    FMI_TUNE_ALLOC_SLOTS = 14     /* fmi_dev_alloc of >= 1 MiB: 0 (default since round 6) = plain hipMalloc;
                                    1 = place successive buckets in successive of 16 4-KiB slots (modulo 64 KiB)
                                    of a hipMalloc 64 KiB larger (round 5). The buckets of one fused kernel belong
                                    in one fmi_dev_alloc_group, which places them whatever this says.
                                    fmi_dev_free takes either. Same bits */,
    FMI_TUNE_COMM_SHARD_SKEW = 15 /* sharded collectives (path TREE allreduce): 1 (default) = the all-to-all lands
                                    the N shards the fused shard kernel streams together in distinct 4 KiB slots
                                    (stride: the shard rounded up to 64 KiB plus 4 KiB), its output in the next one,
                                    where the transport posts a receive per peer anyway (LOCAL, PROC, RCCL's grouped
                                    form, FMI_TUNE_COMM_A2A set to 1; never ncclAllToAll); 0 = back to back. Shards under
                                    1 MiB stay back to back. Ranks may differ (only local placement changes). Same
                                    bits */
} fmi_tune_key_t;
int fmi_tune_set(int key, long long value);
int fmi_tune_get(int key, long long* value);

#ifdef __cplusplus
}
#endif

#endif /* FMI_DEV_H */
