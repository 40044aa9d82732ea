#!/usr/bin/env python3
"""Is the device code of a source-only change the same, kernel by kernel? Compiles translation units of fmi_amd/csrc from
a base revision and from the working tree to gfx950 assembly and diffs every kernel.

    python3 tools/isa_identity.py BASE unit.hip [unit.hip ...] [--jobs N]

BASE's fmi_amd/csrc and include are exported with `git archive` into a temporary directory. Each unit is compiled from
both trees, device only, to assembly, with the HIPFLAGS of the tree's own fmi_amd/csrc/Makefile. The kernels of all
units are pooled per tree (a kernel may have moved between units), every base kernel is paired with the new kernel whose
demangled name, without parameters, equals the base kernel's after RENAMES, and a pair is identical when the function
body (its label to the end of the function) and the .amdhsa_* descriptor block are equal line for line once comments
are stripped, every mangled symbol is replaced by its (renamed) demangled name and the per-function numbers of local
labels are dropped. Nothing else is looked at: the tool diffs, it does not judge instructions.

Prints, per base unit, "kernels paired" and "kernels identical", then every unpaired kernel of either side and the first
differing line of every pair that differs, with both instruction counts. Exit status 1 unless every kernel of both sides
is paired and every pair is identical. A unit that one of the trees does not have counts as holding no kernel there.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("fmi_amd", "csrc")

# Base name -> new name, on demangled names without parameters; the first rule that matches is applied. These are the
# renames of the fold of the MX stochastic-rounding kernels into the round-to-nearest ones (a rounding flag as the last
# template argument); a later comparison with other renames edits this table.
RENAMES = [
    (r"\b(fp8_mx|mxfp4)_sr_kernel<(.*)>$", r"\1_kernel<\2, false, true>"),
    (r"\b(fp8_mx|mxfp4)_kernel<(.*)>$", r"\1_kernel<\2, false>"),
    # the quantize kernels take the stochastic-rounding arguments as a parameter pack: empty for round to nearest
    (r"\b(mx|mxfp4)_quantize_sr_kernel<(.*)>$", r"\1_quantize_kernel<\2, fmi::dev::(anonymous namespace)::SrStream>"),
]


def rename(name):
    for pattern, to in RENAMES:
        if re.search(pattern, name):
            return re.sub(pattern, to, name)
    return name


def hipflags(csrc):
    """HIPFLAGS of the tree's Makefile, $(ARCH) expanded."""
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    return re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["HIPFLAGS"]).split()


def assembly(job):
    csrc, unit, out = job
    if not os.path.exists(os.path.join(csrc, unit)):
        return ""
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *hipflags(csrc), "--cuda-device-only", "-S", unit, "-o", out],
                   cwd=csrc, check=True, capture_output=True)
    return open(out).read()


def kernels(text):
    """{mangled name: (body lines, descriptor lines)} of one assembly file, comments and blank lines stripped."""
    lines = [l for l in (re.sub(r"\s*;.*$", "", l).strip() for l in text.split("\n")) if l]
    found = {}
    for k, l in enumerate(lines):
        if l.startswith(".amdhsa_kernel "):
            name = l.split()[1]
            start = lines.index(name + ":")
            body = lines[start:next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))]
            found[name] = (body, lines[k:lines.index(".end_amdhsa_kernel", k)])
    return found


def demangle(names):
    """{mangled: demangled without parameters}. binutils' c++filt does not know _Float16 (DF16_) and __bf16 (DF16b): they
    go through it as two other builtin types no kernel here uses (builtin types take no part in substitutions)."""
    names = sorted(names)
    stand_in = "\n".join(n.replace("DF16_", "Dd").replace("DF16b", "De") for n in names)
    out = subprocess.run(["c++filt", "-p"], input=stand_in, capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.replace("decimal64", "_Float16").replace("decimal128", "__bf16").split("\n")))


def normalised(kernel, names):
    """One kernel's lines with every mangled symbol replaced by names[symbol] and local labels' function numbers dropped."""
    body, descriptor = kernel
    text = "\n".join(body + ["--"] + descriptor)
    text = re.sub(r"_Z[\w.$]+", lambda m: "{" + names.get(m.group(0), m.group(0)) + "}", text)
    return re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", text).split("\n")


def instructions(lines):
    return sum(1 for l in lines[:lines.index("--")] if not l.startswith(".") and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base", help="the revision to compare the working tree with")
    ap.add_argument("units", nargs="+", help="translation units of fmi_amd/csrc, by file name")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 8))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "archive", a.base, CSRC, "include"], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=archive, check=True)
        jobs = [(os.path.join(tree, CSRC), u, os.path.join(tmp, f"{side}_{u}.s")) for u in a.units for side, tree in (("base", tmp), ("new", ROOT))]
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            texts = list(ex.map(assembly, jobs))
    base = {u: kernels(t) for (_, u, _), t in zip(jobs[0::2], texts[0::2])}
    new = {name: k for t in texts[1::2] for name, k in kernels(t).items()}
    base_names = {m: rename(d) for m, d in demangle({name for ks in base.values() for name in ks}).items()}
    new_names = demangle(new)
    new_by_name = {}
    for m, d in new_names.items():
        new_by_name.setdefault(d, []).append(m)
    bad = 0
    taken = set()
    for unit in a.units:
        paired = same = 0
        notes = []
        for m, kernel in base[unit].items():
            partners = new_by_name.get(base_names[m], [])
            if len(partners) != 1 or partners[0] in taken:
                notes.append(f"  unpaired base kernel: {base_names[m]} ({len(partners)} candidates)")
                continue
            taken.add(partners[0])
            paired += 1
            old, now = normalised(kernel, base_names), normalised(new[partners[0]], new_names)
            if old == now:
                same += 1
                continue
            k = next((j for j, (x, y) in enumerate(zip(old, now)) if x != y), min(len(old), len(now)))
            notes.append(f"  differs: {base_names[m]}: {instructions(old)} -> {instructions(now)} instructions, {len(old)} -> {len(now)} lines; "
                         f"first at line {k}: {old[k] if k < len(old) else '(end)'!r} -> {now[k] if k < len(now) else '(end)'!r}")
        bad += len(base[unit]) - same
        print(f"{unit}: {len(base[unit])} base kernels, {paired} paired, {same} identical")
        print("\n".join(notes), end="\n" if notes else "")
    left = sorted(new_names[m] for m in new if m not in taken)
    for d in left:
        print(f"unpaired new kernel: {d}")
    print(f"{sum(len(ks) for ks in base.values())} base kernels, {len(new)} new kernels, {len(taken)} paired, "
          f"{sum(len(ks) for ks in base.values()) - bad} identical, {len(left)} new kernels unpaired")
    return 1 if bad or left else 0


if __name__ == "__main__":
    sys.exit(main())
