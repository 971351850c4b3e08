"""CPU-only checks of the segmented sort (vrdxHipCmdSortSegmented[KeyValue]): the C-ABI surface, the header in C and C++,
the single header's implementation object, the kernels in the gfx950 code object, the storage carving and the host-side
argument checks of vulkan_radix_sort_amd.segmented."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
SINGLE_HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
NAMES = ("vrdxHipCmdSortSegmented", "vrdxHipCmdSortSegmentedKeyValue")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(vrdx[A-Z]\w+)\s*\(", text))


def _single_header():
    if not os.path.exists(SINGLE_HEADER):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", SINGLE_HEADER],
                       check=True)
    return SINGLE_HEADER


def test_header_library_and_python_agree_on_the_segmented_entry_points():
    import vulkan_radix_sort_amd as vrdx
    declared = _declared()
    lib = vrdx.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in vrdx.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None, name
    assert vrdx.STATUS_SEGMENTS_INVALID == 0x4
    text = open(HEADER).read()
    assert re.search(r"#define VRDX_HIP_STATUS_SEGMENTS_INVALID\s+0x00000004u", text)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_segmented_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize,\n"
        "               VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortSegmented;\n"
        "  void (*pairs)(VkCommandBuffer, VrdxSorter, uint32_t, uint32_t, VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize,\n"
        "                VkBuffer, VkDeviceSize, VkBuffer, VkDeviceSize, VkQueryPool, uint32_t) = vrdxHipCmdSortSegmentedKeyValue;\n"
        "  return (keys != 0 && pairs != 0 && VRDX_HIP_STATUS_SEGMENTS_INVALID == 4u) ? 0 : 1;\n}\n")
    obj = tmp_path / "s.o"
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                   check=True)


def test_single_header_implementation_exports_the_segmented_entry_points(tmp_path):
    header = _single_header()
    (tmp_path / "impl.cc").write_text('#define VRDX_IMPLEMENTATION\n#include "%s"\n' % header)
    gxx = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    subprocess.run(gxx + ["-c", str(tmp_path / "impl.cc"), "-o", str(tmp_path / "impl.o")], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(tmp_path / "impl.o")], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name


def test_code_object_holds_every_kernel_the_launcher_asks_for():
    """The gfx950 code object embedded in the single header (cross-compiled here) contains every mangled name
    expected_kernels() lists -- the segmented kernels among them, both ranking modes, keys-only and key+value -- and no
    kernel the list (vrdx_launch.inc) leaves out."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import generate_single_header as gen
    finally:
        sys.path.pop(0)
    names = gen.expected_kernels()
    for kernel in ("segmented_small_kernel", "segmented_mid_kernel", "segmented_large_kernel"):
        assert sum(kernel in n for n in names) == 4, kernel
    text = open(_single_header()).read()
    array = text.split("static const unsigned char kVrdxCodeObject[] = {", 1)[1].split("};", 1)[0]
    blob = bytes(int(x) for x in array.replace("\n", "").split(","))
    missing = [n for n in names if n.encode() not in blob]
    assert not missing, missing
    kernels = {k.decode() for k in re.findall(rb"(_ZN4vrdx\w+)\.kd\x00", blob)}
    assert kernels == set(names) and len(names) == len(kernels), (sorted(kernels ^ set(names)), len(names))


def test_segmented_storage_carving_fits_every_count(tmp_path):
    """vrdx_layout.h MakeSegmentedLayout: the two lists and the scratch arrays stay inside the reference's storage
    requirement (keys-only and key+value) for every count from 1 to 2^21 and sampled counts up to 2^30 - 4, at every
    16-byte alignment of the storage within a 128-byte line."""
    src = tmp_path / "fit.cc"
    src.write_text(
        '#include <cstdio>\n#include "vrdx_layout.h"\n'
        "int main() {\n"
        "  unsigned long bad = 0, seen = 0;\n"
        "  auto check = [&](uint32_t n) {\n"
        "    for (uint64_t a = 0; a < 128; a += 16) {\n"
        "      const vrdx::SegmentedLayout s = vrdx::MakeSegmentedLayout(n, 16, false, a);\n"
        "      const bool fitsKeyValue = vrdx::MakeSegmentedLayout(n, 16, true, a).fits;\n"
        "      ++seen;\n"
        "      const bool listsOk = s.midCap == n / 4097 && s.largeCap == n / 16385 && s.midListOffset >= 16 + 4096 &&\n"
        "                           s.keysScratchOffset >= s.largeListOffset + 4ull * s.largeCap && (a + s.keysScratchOffset) % 128 == 0;\n"
        "      if (!s.fits || !fitsKeyValue || !listsOk) { if (bad++ < 5) std::printf(\"n=%u a=%u\\n\", n, (unsigned)a); }\n"
        "    }\n"
        "  };\n"
        "  for (uint32_t n = 1; n <= (1u << 21); ++n) check(n);\n"
        "  for (uint64_t n = (1u << 21); n < 0x3FFFFFFCu; n += 65521) check((uint32_t)n);\n"
        "  check(0x3FFFFFFCu);\n"
        '  std::printf("%lu layouts, %lu failures\\n", seen, bad);\n'
        "  return bad != 0;\n}\n")
    exe = tmp_path / "fit"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout


def test_sort_segments_rejects_bad_arguments_on_the_host():
    """Wrong dtypes, shapes and layouts are refused before anything is recorded (no sorter call is reached, so no GPU
    is needed to see it)."""
    import torch
    from vulkan_radix_sort_amd.segmented import sort_segments
    keys = torch.zeros(16, dtype=torch.int32)
    offsets = torch.tensor([0, 8, 16], dtype=torch.int32)
    with pytest.raises(TypeError):
        sort_segments(None, keys.to(torch.int64), offsets)
    with pytest.raises(TypeError):
        sort_segments(None, keys.to(torch.float32), offsets)
    with pytest.raises(TypeError):
        sort_segments(None, keys.to(torch.int16), offsets)
    with pytest.raises(TypeError):
        sort_segments(None, keys.numpy(), offsets)
    with pytest.raises(ValueError):
        sort_segments(None, keys.view(4, 4), offsets)
    with pytest.raises(ValueError):
        sort_segments(None, torch.zeros(32, dtype=torch.int32)[::2], offsets)
    with pytest.raises(ValueError):  # not on a GPU
        sort_segments(None, keys, offsets)
    if torch.cuda.is_available():
        dk, do = keys.cuda(), offsets.cuda()
        with pytest.raises(TypeError):
            sort_segments(None, dk, do.to(torch.int64))
        with pytest.raises(ValueError):
            sort_segments(None, dk, do[:0])
        with pytest.raises(ValueError):
            sort_segments(None, dk, do.view(1, 3))
        with pytest.raises(TypeError):
            sort_segments(None, dk, do, values=dk.to(torch.float32))
        with pytest.raises(ValueError):
            sort_segments(None, dk, do, values=dk[:8])
