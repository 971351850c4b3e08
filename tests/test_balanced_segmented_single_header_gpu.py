"""The balanced segmented sort through the single-header distribution: the generated `vk_radix_sort.h` compiles on its own
with plain g++ (no hipcc, no libvrdx_hip.so), its implementation unit exports the four new entry points, and on the GPU
tests/native/balanced_segmented_single_header.cpp sorts 300007 elements in six segments, two of them spread, keys-only and
key+value, against a stable reference of its own -- the split, count, scan, scatter and copy-back kernels found by mangled
name in the embedded code object."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
SOURCE = os.path.join(ROOT, "tests", "native", "balanced_segmented_single_header.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
KERNELS = ("segmented_split_kernel", "segmented_piece_count_kernel", "segmented_piece_scan_kernel",
           "segmented_piece_scatter_kernel", "segmented_piece_copy_back_kernel")


def _header():
    """The generated header, regenerated when it is older than what it is made from."""
    sources = [os.path.join(ROOT, "include", "vk_radix_sort.h"), os.path.join(ROOT, "tools", "generate_single_header.py")]
    csrc = os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc")
    sources += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("vrdx_")]
    if not os.path.exists(HEADER) or os.path.getmtime(HEADER) < max(os.path.getmtime(s) for s in sources):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", HEADER], check=True)
    return HEADER


def test_single_header_serves_the_balanced_entry_points(tmp_path):
    """CPU: the program compiles against the generated header alone, and the object defines the four entry points"""
    header = _header()
    text = open(header).read()
    for kernel in KERNELS:   # every new launch is in the one launch list, so the single header has its name
        assert kernel in text, kernel
    obj = tmp_path / "balanced_segmented_single_header.o"
    subprocess.run(GXX + ["-I" + os.path.dirname(header), "-c", SOURCE, "-o", str(obj)], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    for name in ("vrdxHipCmdBalancedSortSegmented", "vrdxHipCmdBalancedSortSegmentedKeyValue",
                 "vrdxHipDescribeBalancedSegmentedPlan", "vrdxHipReadBalancedSplit"):
        assert f" T {name}\n" in nm, name


@pytest.mark.gpu
def test_single_header_sorts_spread_segments(tmp_path):
    header = _header()
    exe = tmp_path / "balanced_segmented_single_header"
    subprocess.run(GXX + ["-I" + os.path.dirname(header), SOURCE, "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                          "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ldd = subprocess.run(["ldd", str(exe)], capture_output=True, text=True, check=True).stdout
    assert "libvrdx_hip" not in ldd and "libamdhip64" in ldd
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "2 cases, status 0, 0 mismatches, 4 spread" in r.stdout, r.stdout + r.stderr
