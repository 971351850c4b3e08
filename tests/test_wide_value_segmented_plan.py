"""Without a GPU: the plan and the layout of the segmented sort of 32-bit keys with 64-bit values (vrdx_plan.h,
PlanWideValueSortSegmented; vrdx_layout.h, MakeSegmentedWideLayout) through tests/native/wide_value_segmented_plan_check.cpp,
compiled here with g++: which steps exist at every size where a class begins, their slots and grids at every segment count
around the CU count and the 2^20 cap, the list caps, and the lists and both scratch arrays inside the unchanged wide-value
requirement for every storage address."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "wide_value_segmented_plan_check.cpp")


def test_steps_grids_caps_and_layout_at_every_size_count_and_address(tmp_path):
    exe = tmp_path / "wide_value_segmented_plan_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SOURCE,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    done = re.search(r"wide value segmented plan: (\d+) cases, 0 failures", r.stdout)
    # 2 CU counts x 2 rankings x 11 sizes x 8 segment counts x 8 addresses x 9 checks, and the empty calls
    assert done and int(done.group(1)) >= 2 * 2 * 11 * 8 * 8 * 9, r.stdout[-1000:]


def test_the_plan_is_a_function_of_its_own_next_to_the_flat_one():
    """not a sixth mode of PlanSegmentedSort: that function and its name table are what they were"""
    text = open(os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc", "vrdx_plan.h")).read()
    assert text.index("PlanWideValueSort(const PlanContext") < text.index("PlanWideValueSortSegmented(const PlanContext")
    body = text[text.index("static inline SegmentedPlan PlanSegmentedSort("):text.index("// ---- the 64-bit sorts")]
    assert "wide" + "_kernel" not in body and "kNames[5][4]" in body
