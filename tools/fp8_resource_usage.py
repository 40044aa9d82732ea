#!/usr/bin/env python3
"""Register and scratch use of the 8-bit float kernels: the fused f32-accumulating P-way units
(fmi_amd/csrc/fmi_fused_fp8_acc32_*.hip) and the conversions (fmi_acc32_convert.hip), read from the compiler's own
remarks as tools/half_resource_usage.py does it (each unit compiled device-only for gfx950 with
-Rpass-analysis=kernel-resource-usage). Exits 1 if any kernel uses scratch.

    python3 tools/fp8_resource_usage.py                  # every fp8_acc_kernel at P = 8 and P = 16, and the conversions
    python3 tools/fp8_resource_usage.py --all            # every P
    python3 tools/fp8_resource_usage.py --mx             # the fused MX units (fmi_fused_mx_*.hip) and fmi_mx.hip instead:
                                                         # fp8_mx_kernel / mxfp4_kernel at P = 8 and 16, the quantize / dequantize kernels
    python3 tools/fp8_resource_usage.py --isa            # instruction counts of the 8-way allreduce SUM kernels' loop
                                                         # (e4m3, e5m2 and the bf16 acc32 kernel beside them)

Lines: fp8_acc_kernel<op, dtype, alg, P, scan>: vgpr .. agpr .. scratch .. occupancy ..
(alg: 0 allreduce, 1 reduce, 2 reduce_ltr, 3 scan, 4 scan_ltr, 8 reduce partials);
fp8_mx_kernel<dtype, alg, P, out32>, mx_quantize_kernel<dtype, source>, mx_dequantize_kernel<dtype, destination>;
mxfp4_kernel<alg, P, out32>, mxfp4_quantize_kernel<source>, mxfp4_dequantize_kernel<destination> (the MXFP4 units,
fmi_fused_mxfp4_*.hip, are part of --mx). These are the round-to-nearest instantiations: fp8_mx_kernel and mxfp4_kernel
have the rounding as one more, last, template argument, the quantize kernels the stochastic-rounding arguments as a
trailing parameter pack, and a line shows neither. The stochastic-rounding instantiations of the same kernels
(fmi_fused_mx_sr_*.hip, fmi_fused_mxfp4_sr_*.hip, and in fmi_mx.hip) are compiled with the rest and not listed.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from half_resource_usage import CSRC, parse, remarks  # noqa: E402

FP8 = {"6f8e4m3": "e4m3", "6f8e5m2": "e5m2"}
OTHER = {"f": "f32", "DF16_": "f16", "DF16b": "bf16"}


def describe(mangled):
    m = re.search(r"14fp8_acc_kernelINS\d*_\d(Op[A-Z][a-z]+)ENS\d*_(6f8e4m3|6f8e5m2)ELi(\d+)ELi(\d+)ELb([01])EEE", mangled)
    if m:
        return "fp8_acc_kernel", int(m.group(4)), f"{m.group(1)}, {FP8[m.group(2)]}, {m.group(3)}, {m.group(4)}, " \
                                                  f"{'true' if m.group(5) == '1' else 'false'}"
    m = re.search(r"14convert_kernelI(.+?)Lb([01])EEE", mangled)
    if m and "f8e" in m.group(1):
        types = re.findall(r"NS\d*_(6f8e4m3|6f8e5m2)E|S\d*_|(DF16_|DF16b|f)", m.group(1))
        names = [FP8.get(a) or OTHER.get(b) or "same" for a, b in types]
        return "convert_kernel", 0, ", ".join(names + ["nt" if m.group(2) == "1" else "plain"])
    # the MX kernels' last template argument is the rounding: Lb0E, round to nearest, is listed (without it); Lb1E is not
    m = re.search(r"13fp8_mx_kernelINS\d*_(6f8e4m3|6f8e5m2)ELi(\d+)ELi(\d+)ELb([01])ELb0EEE", mangled)
    if m:
        return "fp8_mx_kernel", int(m.group(3)), f"{FP8[m.group(1)]}, {m.group(2)}, {m.group(3)}, {'true' if m.group(4) == '1' else 'false'}"
    m = re.search(r"\d+(mx_quantize_kernel|mx_dequantize_kernel)INS\d*_(6f8e4m3|6f8e5m2)E(DF16_|DF16b|f)(?:JE)?EE", mangled)
    if m:
        return m.group(1), 0, f"{FP8[m.group(2)]}, {OTHER[m.group(3)]}"
    m = re.search(r"12mxfp4_kernelILi(\d+)ELi(\d+)ELb([01])ELb0EEE", mangled)
    if m:
        return "mxfp4_kernel", int(m.group(2)), f"{m.group(1)}, {m.group(2)}, {'true' if m.group(3) == '1' else 'false'}"
    m = re.search(r"\d+(mxfp4_quantize_kernel|mxfp4_dequantize_kernel)I(DF16_|DF16b|f)(?:JE)?EE", mangled)
    if m:
        return m.group(1), 0, OTHER[m.group(2)]
    return None


ISA_KERNELS = [("fmi_fused_fp8_acc32_allreduce.hip", "fp8_acc_kernelINS0_5OpSumENS0_6f8e4m3ELi0ELi8ELb0", "e4m3 acc32"),
               ("fmi_fused_fp8_acc32_allreduce.hip", "fp8_acc_kernelINS0_5OpSumENS0_6f8e5m2ELi0ELi8ELb0", "e5m2 acc32"),
               ("fmi_fused_acc32_allreduce.hip", "tree_kernelINS0_5OpSumENS0_5Acc32IDF16bEELi0ELi8ELb0", "bf16 acc32")]


def isa():
    """Per lane group (8 x 16 B in, 16 B out) of the buffer-policy loop, first buffer load to the buffer store."""
    import collections
    import subprocess
    import tempfile
    texts = {}
    for src, label, name in ISA_KERNELS:
        if src not in texts:
            with tempfile.NamedTemporaryFile(suffix=".s") as f:
                subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++20", "-O3", "--offload-arch=gfx950",
                                "-fno-gpu-rdc", "-ffp-contract=off", "--cuda-device-only", "-S", src, "-o", f.name],
                               cwd=CSRC, check=True, capture_output=True)
                texts[src] = open(f.name).read().split("\n")
        lines = texts[src]
        start = next(k for k, l in enumerate(lines) if label in l and l.rstrip().endswith(":") is False and l.startswith("_Z"))
        body = lines[start:next(k for k in range(start, len(lines)) if "s_endpgm" in lines[k])]
        lo = next(k for k, l in enumerate(body) if "buffer_load_dwordx4" in l)
        hi = next(k for k, l in enumerate(body) if "buffer_store_dwordx4" in l)
        c = collections.Counter(m.group(1) for l in body[lo:hi + 1] if (m := re.match(r"\s+([a-z]+_[a-z0-9_]+)", l)))
        valu = sum(v for k, v in c.items() if k.startswith("v_"))
        print(f"8-way allreduce sum {name}: VALU {valu} ({valu / 8:.1f} per 16 B of input): " +
              ", ".join(f"{k} {v}" for k, v in sorted(c.items()) if k.startswith("v_") or k.startswith("buffer_")))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", action="store_true", help="instruction counts of the 8-way allreduce kernels instead")
    ap.add_argument("--all", action="store_true", help="every P, not P = 8 and 16 alone")
    ap.add_argument("--mx", action="store_true", help="the MX units (fmi_fused_mx_*.hip, fmi_mx.hip) instead")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 8))
    a = ap.parse_args()
    if a.isa:
        return isa()
    if a.mx:
        srcs = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "fmi_fused_mx_*.hip")) +
                      glob.glob(os.path.join(CSRC, "fmi_fused_mxfp4_*.hip"))) + ["fmi_mx.hip"]
    else:
        srcs = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "fmi_fused_fp8_acc32_*.hip"))) + ["fmi_acc32_convert.hip"]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        kernels = [k for t in ex.map(remarks, srcs) for k in parse(t)]
    shown = spilled = 0
    for k in kernels:
        d = describe(k["name"])
        if d is None or (d[0].endswith("mx_kernel") or d[0].startswith("mx")) != a.mx:
            continue
        spilled += k["scratch"] != 0
        if d[0] in ("fp8_acc_kernel", "fp8_mx_kernel", "mxfp4_kernel") and not a.all and d[1] not in (8, 16):
            continue
        shown += 1
        print(f"{d[0]}<{d[2]}>: vgpr {k['vgpr']} agpr {k['agpr']} scratch {k['scratch']} occupancy {k['occ']}")
    print(f"{shown} kernels shown, {spilled} 8-bit float kernels with scratch")
    return 1 if spilled else 0


if __name__ == "__main__":
    sys.exit(main())
