"""Without a GPU: the plans of the ordered 32-bit sorts (vrdx_plan.h, PlanOrderedSort and the order word of
PlanSegmentedSort's 4-byte keys) through tests/native/ordered_sort_plan_check.cpp, compiled here with g++: order 0 is the
twin's plan field for field, a valid order is the twin's steps with the ordered one-workgroup kernel or between the two
transform steps at slots [0,1] and [13,14], an invalid word is refused."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "ordered_sort_plan_check.cpp")


def test_the_ordered_plans_at_every_size_where_the_plan_changes(tmp_path):
    exe = tmp_path / "ordered_sort_plan_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SOURCE,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    done = re.search(r"ordered sort plan: (\d+) cases, 0 failures", r.stdout)
    assert done and int(done.group(1)) > 5000, r.stdout[-1000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("cus ")]
    assert len(lines) == 8
    for line in lines:   # one workgroup ends at 16384 everywhere, and with the one-atomic ranking an MSD plan follows the hybrid one
        edges = [int(x) for x in line.split("behind")[1].split("(")[0].split()]
        assert edges and edges[0] == 16384, line
        assert len(edges) >= (3 if " atomic 1 " in line else 2), line
