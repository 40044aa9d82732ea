"""The pairwise-pass plan of a P-way program (fmi_amd/csrc/fmi_schedule.h plan_stepwise) on the host.

run_program_stepwise (fmi_dev.hip) runs a program's live steps as pairwise kernels over temporaries in the scratch
arena, in the slots this plan assigns; a slot recycled too early would let one step overwrite a value a later step
reads, and only the shapes the GPU tests sample would show it. tests/stepwise_plan_check.cpp executes the plan for
every algorithm the stepwise path serves (allreduce for ranks 0, P / 2 and P - 1, reduce, reduce_ltr, scan, scan_ltr,
reduce partials) and P = 1…40, 64, 100, 257 and 1000 on slots that hold value ids, and checks that every operand is
resident when read, that no step overwrites a value still to be read or an output, that every output is resident at
the end, and that the slot count is the peak number of live temporaries.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "stepwise_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fmi_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "stepwise_plan_check.cpp")], check=True)
    return exe


def test_stepwise_plans_keep_every_operand_and_output(checker):
    r = subprocess.run([checker, "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 352 plans"), r.stdout
