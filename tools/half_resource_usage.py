#!/usr/bin/env python3
"""Register and scratch use of the 16-bit float kernels (fmi_amd/csrc/fmi_fused_half_*.hip, and the f32-accumulating
ones of FMI_ACC_F32: fmi_fused_acc32_*.hip with the fallback's conversions in fmi_acc32_convert.hip), read from the
compiler's own remarks: each unit is compiled device-only for gfx950 with -Rpass-analysis=kernel-resource-usage,
and every kernel's VGPRs / AGPRs / scratch / occupancy are collected. Exits 1 if any kernel uses scratch.

    python3 tools/half_resource_usage.py                 # compile (a few minutes), print the summary per family
    python3 tools/half_resource_usage.py --logs DIR      # parse remark logs kept from a build instead
    python3 tools/half_resource_usage.py --core          # the f32 kernels of the core units, for the comparison
    python3 tools/half_resource_usage.py --acc32         # the FMI_ACC_F32 units alone
    python3 tools/half_resource_usage.py --avg           # the FMI_OP_AVG units (fmi_fused_avg_*.hip, fmi_scale.hip), every dtype

The summary groups kernels by family, dtype and op and gives the range over P.
"""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fmi_amd", "csrc")
FLAGS = ["-std=c++20", "-O3", "--offload-arch=gfx950", "-fno-gpu-rdc", "-ffp-contract=off", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
CORE = ["fmi_fused_allreduce.hip", "fmi_fused_allreduce_wide.hip", "fmi_fused_reduce.hip", "fmi_fused_scan.hip",
        "fmi_fused_scan_wide.hip", "fmi_fused_chain.hip", "fmi_fused_tree_blocked.hip", "fmi_fused_scan_blocked.hip",
        "fmi_fused_scan_blocked_wide.hip"]
FIELD = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ"}


def remarks(src):
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, src], cwd=CSRC, capture_output=True,
                       text=True)
    if r.returncode != 0:
        sys.exit(f"{src}: {r.stderr[-2000:]}")
    return r.stderr


def parse(text):
    """[{name, vgpr, agpr, scratch, occ}] from the remark lines of one compilation."""
    out, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+): (\d+) \[-Rpass", line)
        if m and cur is not None and m.group(1).strip() in FIELD:
            cur[FIELD[m.group(1).strip()]] = int(m.group(2))
    return [k for k in out if "vgpr" in k]


DTYPES = {"DF16_": "f16", "DF16b": "bf16", "f": "f32", "d": "f64", "i": "i32", "l": "i64"}


def describe(mangled):
    """(kernel, dtype, op, the remaining template arguments) from a kernel's Itanium-mangled name, e.g.
    _ZN3fmi3dev11tree_kernelINS0_5OpSumEDF16_Li7ELi32ELb0EEEv...: tree_kernel<OpSum, _Float16, 7, 32, false>."""
    m = re.search(r"(?<=\d)(scale_kernel)I(DF16_|DF16b|[fd])E", mangled)
    if m:  # fmi_scale.hip: one kernel per float dtype
        return m.group(1), DTYPES[m.group(2)], "", ""
    m = re.search(r"(?<=\d)([a-z_]+_kernel)INS\d*_\d(Op[A-Z][a-z]+)E(NS\d*_5Acc32I)?(DF16_|DF16b|[fdil])(?(3)EE)((?:L[ib]\d+E)*)E",
                  mangled)
    if not m:
        return None
    if m.group(3):  # Acc32<T>: 16-bit storage, f32 values (FMI_ACC_F32)
        args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(5))]
        return m.group(1) + "_acc32", DTYPES[m.group(4)], m.group(2), ", ".join(args)
    args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(5))]
    return m.group(1), DTYPES[m.group(4)], m.group(2), ", ".join(args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", help="directory of remark logs (one per unit) to parse instead of compiling")
    ap.add_argument("--core", action="store_true", help="the core units' f32 kernels instead of the half units")
    ap.add_argument("--acc32", action="store_true", help="the FMI_ACC_F32 units alone")
    ap.add_argument("--avg", action="store_true", help="the FMI_OP_AVG units alone, every dtype")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 8))
    ap.add_argument("--all", action="store_true", help="print every kernel, not the summary")
    a = ap.parse_args()
    if a.logs:
        texts = [open(f).read() for f in sorted(glob.glob(os.path.join(a.logs, "*.log")))]
    else:
        units = lambda pat: sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, pat)))  # noqa: E731
        acc32 = units("fmi_fused_acc32_*.hip") + ["fmi_acc32_convert.hip"]
        avg = units("fmi_fused_avg_*.hip") + ["fmi_scale.hip"]
        srcs = CORE if a.core else acc32 if a.acc32 else avg if a.avg else units("fmi_fused_half_*.hip") + acc32
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            texts = list(ex.map(remarks, srcs))
    kernels = [k for t in texts for k in parse(t)]
    groups = collections.defaultdict(list)
    for k in kernels:
        d = describe(k["name"])
        if d is None or (a.core and d[1] != "f32") or (not a.core and not a.avg and d[1] not in ("f16", "bf16")):
            continue
        kern, dtype, op, detail = d
        if a.all:
            print(f"{kern}<{op}, {dtype}, {detail}>: vgpr {k['vgpr']} agpr {k['agpr']} scratch {k['scratch']} occupancy {k['occ']}")
        fused = kern in ("tree_kernel", "scan_kernel", "tree_kernel_acc32", "scan_kernel_acc32")
        alg = detail.split(",")[0] if fused else ""
        ranked = kern in ("tree_kernel", "tree_blocks_kernel", "prefold_blocks_kernel") and detail.endswith("true")
        if kern == "tree_kernel_acc32":
            detail = detail.rsplit(",", 1)[0]  # no rank-selecting form
        wide = ""
        if fused:
            wide = "P>16" if int(detail.split(",")[1]) > 16 else "P<=16"
        groups[(kern, alg, wide, "ranked" if ranked else "", dtype, op)].append(k)
    rng = lambda xs: f"{min(xs)}" if min(xs) == max(xs) else f"{min(xs)}-{max(xs)}"
    print("kernel | alg | P | form | dtype | op | kernels | VGPRs | AGPRs | scratch | waves/SIMD")
    for key in sorted(groups):
        ks = groups[key]
        print(" | ".join(key) + f" | {len(ks)} | {rng([k['vgpr'] for k in ks])} | {rng([k['agpr'] for k in ks])} | "
              f"{rng([k['scratch'] for k in ks])} | {rng([k['occ'] for k in ks])}")
    spilled = [k for k in kernels if k["scratch"] != 0]
    print(f"{len(kernels)} kernels, {len(spilled)} with scratch")
    for k in spilled:
        print("  scratch", k["scratch"], "B/lane:", k["name"])
    return 1 if spilled else 0


if __name__ == "__main__":
    sys.exit(main())
