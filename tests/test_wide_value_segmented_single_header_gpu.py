"""The segmented sort of 32-bit keys with 64-bit values through the single-header distribution: the generated
`vk_radix_sort.h` holds the six new kernels' names, its implementation unit compiles with plain g++ (no hipcc, no
libvrdx_hip.so) and exports the new entry point, and on the GPU tests/native/wide_value_segmented_single_header.cpp sorts
segments of all three classes against a stable reference of its own -- the new kernels found by mangled name in the embedded
code object."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
SOURCE = os.path.join(ROOT, "tests", "native", "wide_value_segmented_single_header.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
KERNELS = ("segmented_small_wide_kernel", "segmented_mid_wide_kernel", "segmented_large_wide_kernel")


def _header():
    """The generated header, regenerated when it is older than what it is made from."""
    sources = [os.path.join(ROOT, "include", "vk_radix_sort.h"), os.path.join(ROOT, "tools", "generate_single_header.py")]
    csrc = os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc")
    sources += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.startswith("vrdx_")]
    if not os.path.exists(HEADER) or os.path.getmtime(HEADER) < max(os.path.getmtime(s) for s in sources):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", HEADER], check=True)
    return HEADER


def test_the_generator_finds_the_six_new_kernels():
    """no header is built: the list the generator checks the code object against names both rankings of the three kernels,
    behind every row the list had"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_single_header", os.path.join(ROOT, "tools", "generate_single_header.py"))
    generator = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(generator)
    names = generator.expected_kernels()
    new = [n for n in names if re.search(r"segmented_(small|mid|large)_wide_kernel", n)]
    assert len(new) == 6 and names[-6:] == new and len(set(names)) == len(names)
    assert [bool(re.search(r"ILb1E", n)) for n in new] == [False, True] * 3


def test_single_header_serves_the_entry_point(tmp_path):
    """CPU: the program compiles against the generated header alone, and the object defines the entry point"""
    header = _header()
    text = open(header).read()
    for kernel in KERNELS:
        assert kernel in text, kernel
    obj = tmp_path / "wide_value_segmented_single_header.o"
    subprocess.run(GXX + ["-I" + os.path.dirname(header), "-c", SOURCE, "-o", str(obj)], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    assert " T vrdxHipCmdWideValueSortSegmented\n" in nm


@pytest.mark.gpu
def test_single_header_sorts_segments_with_wide_values(tmp_path):
    header = _header()
    exe = tmp_path / "wide_value_segmented_single_header"
    subprocess.run(GXX + ["-I" + os.path.dirname(header), SOURCE, "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                          "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ldd = subprocess.run(["ldd", str(exe)], capture_output=True, text=True, check=True).stdout
    assert "libvrdx_hip" not in ldd and "libamdhip64" in ldd
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "2 cases, status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
