"""Without a GPU: the plan and the storage of the sorts of 32-bit keys with 64-bit values (vrdx_plan.h, PlanWideValueSort;
vrdx_layout.h, MakeWideValueLayout) through tests/native/wide_value_plan_check.cpp, compiled here with g++: the form at every
size where it changes, the steps and their slots, A, B, C inside the requirement on their 128-byte lines for every storage
address, `smallSort == false` moving n <= 8192 to the gather form; and the same program built as the always-gather and the
always-two-sorts variants of the measurement, whose constant comes from the compiler's command line."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "wide_value_plan_check.cpp")


def _run(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *flags, SOURCE,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    done = re.search(r"wide value plan: (\d+) cases, 0 failures", r.stdout)
    assert done and int(done.group(1)) > 2000, r.stdout[-1000:]
    return int(re.search(r"two sorts from (\d+), one workgroup up to 8192", r.stdout).group(1))


def test_the_plan_at_every_size_where_the_form_changes(tmp_path):
    constant = _run(tmp_path, "wide_value_plan_check")
    text = open(os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc", "vrdx_plan.h")).read()
    default = re.search(r"#ifndef VRDX_WIDE_VALUE_TWO_SORTS_FROM\n#define VRDX_WIDE_VALUE_TWO_SORTS_FROM \(1u << (\d+)\)\n#endif", text)
    assert default and constant == 1 << int(default.group(1)) and constant > 8193


def test_the_constant_comes_from_the_command_line_for_the_variants(tmp_path):
    assert _run(tmp_path, "late", "-DVRDX_WIDE_VALUE_TWO_SORTS_FROM=100000u") == 100000
