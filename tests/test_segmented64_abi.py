"""CPU-only checks of the segmented sort of 64-bit keys (vrdxHipCmdSortSegmented64[KeyValue]): the C-ABI surface, the
header's text, the single header's implementation object, the kernels in the launch list, the storage carving and the
host-side argument checks of vulkan_radix_sort_amd.sort_segments64."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vk_radix_sort.h")
SINGLE_HEADER = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
NAMES = ("vrdxHipCmdSortSegmented64", "vrdxHipCmdSortSegmented64KeyValue")
KEYS_PARAMS = ["VkCommandBuffer", "VrdxSorter", "uint32_t", "uint32_t", "VkBuffer", "VkDeviceSize", "VkBuffer", "VkDeviceSize",
               "VkBuffer", "VkDeviceSize", "VkQueryPool", "uint32_t"]
PAIRS_PARAMS = KEYS_PARAMS[:8] + ["VkBuffer", "VkDeviceSize"] + KEYS_PARAMS[8:]
KEYS_NAMES = ["commandBuffer", "sorter", "maxElementCount", "segmentCount", "offsetsBuffer", "offsetsOffset", "keysBuffer",
              "keysOffset", "storageBuffer", "storageOffset", "queryPool", "query"]
PAIRS_NAMES = KEYS_NAMES[:8] + ["valuesBuffer", "valuesOffset"] + KEYS_NAMES[8:]


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _single_header():
    if not os.path.exists(SINGLE_HEADER):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", SINGLE_HEADER],
                       check=True)
    return SINGLE_HEADER


def test_header_declares_both_entry_points_with_the_documented_parameters():
    code = _code(open(HEADER).read())
    for name, types, names in ((NAMES[0], KEYS_PARAMS, KEYS_NAMES), (NAMES[1], PAIRS_PARAMS, PAIRS_NAMES)):
        m = re.search(r"\bvoid\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        params = [p.split() for p in m.group(1).replace("\n", " ").split(",")]
        assert [p[0] for p in params] == types, name
        assert [p[1] for p in params] == names, name


def test_library_and_python_agree_on_the_entry_points():
    import vulkan_radix_sort_amd as vrdx
    lib = vrdx.load_library()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    keys = [vp, vp, u32, u32, vp, u64, vp, u64, vp, u64, vp, u32]
    pairs = keys[:8] + [vp, u64] + keys[8:]
    for name, argtypes in zip(NAMES, (keys, pairs)):
        assert name in vrdx.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is None and list(fn.argtypes) == argtypes, name
    nm = subprocess.run(["nm", "-D", "--defined-only", vrdx.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name
    assert callable(vrdx.Sorter.cmd_sort_segmented64) and callable(vrdx.Sorter.cmd_sort_segmented64_key_value)
    assert "sort_segments64" in vrdx.__all__ and callable(vrdx.sort_segments64)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_declarations_compile_as_c_and_cpp(tmp_path, compiler, lang):
    src = tmp_path / ("s.c" if lang == "c" else "s.cc")
    src.write_text(
        '#include "vk_radix_sort.h"\n'
        "int main(void) {\n"
        "  void (*keys)(%s) = vrdxHipCmdSortSegmented64;\n"
        "  void (*pairs)(%s) = vrdxHipCmdSortSegmented64KeyValue;\n"
        "  return (keys != 0 && pairs != 0) ? 0 : 1;\n}\n" % (", ".join(KEYS_PARAMS), ", ".join(PAIRS_PARAMS)))
    subprocess.run([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_single_header_implementation_defines_both_entry_points(tmp_path):
    header = _single_header()
    (tmp_path / "impl.cc").write_text('#define VRDX_IMPLEMENTATION\n#include "%s"\n' % header)
    gxx = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    subprocess.run(gxx + ["-c", str(tmp_path / "impl.cc"), "-o", str(tmp_path / "impl.o")], check=True)
    nm = subprocess.run(["nm", "-g", "--defined-only", str(tmp_path / "impl.o")], capture_output=True, text=True,
                        check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in nm, name


def test_launch_list_holds_every_form_of_the_three_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import generate_single_header as gen
    finally:
        sys.path.pop(0)
    names = gen.expected_kernels()
    for kernel in ("segmented_small64_kernel", "segmented_mid64_kernel", "segmented_large64_kernel"):
        assert sum(kernel in n for n in names) == 4, kernel  # keys-only / key+value x ballot / one-atomic ranking
    blob = open(_single_header()).read()
    array = blob.split("static const unsigned char kVrdxCodeObject[] = {", 1)[1].split("};", 1)[0]
    code = bytes(int(x) for x in array.replace("\n", "").split(","))
    assert not [n for n in names if "64_kernel" in n and n.encode() + b".kd\x00" not in code]


def test_out_of_scope_sentence_no_longer_lists_segmented_64_bit_sorts():
    text = open(HEADER).read()
    m = re.search(r"Out of scope, each left to the caller:(.*?)\*/", text, flags=re.S)
    assert m
    assert "segmented" not in m.group(1).split("Many independent arrays")[0].lower()
    assert "segmented 64-bit sorts;" not in text


LAYOUT_CHECK = r"""
#include <cstdio>
#include "vrdx_layout.h"
int main() {
  const uint32_t counts[] = {1u, 2u, 4096u, 4097u, 8192u, 8193u, 16384u, 16385u, (1u << 20) + 3u, 0x3FFFFFFCu};
  unsigned long bad = 0, seen = 0;
  for (uint32_t n : counts)
    for (int kv = 0; kv < 2; ++kv)
      for (uint64_t a = 0; a < 128; a += 16) {
        const vrdx::SegmentedLayout s = vrdx::MakeSegmented64Layout(n, 16, kv != 0, a);
        const vrdx::Sort64Layout w = vrdx::MakeSort64Layout(n, 16, a);
        const uint64_t size = kv ? w.keyValueSize : w.keysOnlySize;  // vrdxHipGetSorter64[KeyValue]StorageRequirements
        ++seen;
        bool ok = s.fits;
        // the header, then the counters on lines of their own, then the lists, then the arrays: no two overlap
        ok = ok && s.midCountOffset >= 16 && s.largeCountOffset >= s.midCountOffset + 128;
        ok = ok && s.midListOffset >= s.largeCountOffset + 4 && s.largeListOffset == s.midListOffset + 4ull * s.midCap;
        ok = ok && s.midCap == n / 4097u && s.largeCap == n / (kv ? 8193u : 16385u);
        ok = ok && s.keysScratchOffset >= s.largeListOffset + 4ull * s.largeCap;
        ok = ok && (a + s.keysScratchOffset) % 128 == 0 && s.keysScratchOffset + 8ull * n <= size;
        if (kv) {
          ok = ok && s.valuesScratchOffset >= s.keysScratchOffset + 8ull * n && (a + s.valuesScratchOffset) % 128 == 0;
          ok = ok && s.valuesScratchOffset + 4ull * n <= size;
        }
        if (!ok && bad++ < 8) std::printf("n=%u kv=%d a=%u\n", n, kv, (unsigned)a);
      }
  std::printf("%lu layouts, %lu failures\n", seen, bad);
  return bad != 0;
}
"""


def test_storage_carving_stays_inside_the_64_bit_requirements(tmp_path):
    """vrdx_layout.h MakeSegmented64Layout for N in {1, 2, 4096, 4097, 16385, 2^20 + 3, 2^30 - 4} (and the key+value class
    bound): inside vrdxHipGetSorter64[KeyValue]StorageRequirements(N), its arrays clear of the header, the lists and each
    other, at every 16-byte phase of the storage within a 128-byte line."""
    src = tmp_path / "fit64.cc"
    src.write_text(LAYOUT_CHECK)
    exe = tmp_path / "fit64"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "vulkan_radix_sort_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout


def test_sort_segments64_rejects_bad_arguments_on_the_host():
    """The refusals that host tensors can show, with the exception types of sort_segments: keys of a wrong type, dtype,
    shape or layout, and keys that are not on a GPU, before anything is recorded.  The checks behind the keys' (offsets,
    values, storage) need device tensors and a sorter: tests/test_segmented64_gpu.py,
    test_sort_segments64_rejects_bad_device_arguments."""
    import torch
    from vulkan_radix_sort_amd import sort_segments64
    keys = torch.zeros(16, dtype=torch.int64)
    offsets = torch.tensor([0, 8, 16], dtype=torch.int32)
    with pytest.raises(TypeError):
        sort_segments64(None, keys.to(torch.int32), offsets)
    with pytest.raises(TypeError):
        sort_segments64(None, keys.to(torch.float64), offsets)
    with pytest.raises(TypeError):
        sort_segments64(None, keys.numpy(), offsets)
    with pytest.raises(ValueError):
        sort_segments64(None, keys.view(4, 4), offsets)
    with pytest.raises(ValueError):
        sort_segments64(None, torch.zeros(32, dtype=torch.int64)[::2], offsets)
    with pytest.raises(ValueError):  # not on a GPU
        sort_segments64(None, keys, offsets)
    if torch.cuda.is_available():
        import vulkan_radix_sort_amd as vrdx
        dk, do = keys.cuda(), offsets.cuda()
        with pytest.raises(TypeError):
            sort_segments64(None, dk, do.to(torch.int64))
        with pytest.raises(ValueError):
            sort_segments64(None, dk, do[:0])
        with pytest.raises(ValueError):
            sort_segments64(None, dk, offsets)  # offsets on the host
        with pytest.raises(TypeError):
            sort_segments64(None, dk, do, values=dk)
        with pytest.raises(ValueError):
            sort_segments64(None, dk, do, values=torch.zeros(8, dtype=torch.int32, device="cuda"))
        with vrdx.Sorter() as s:
            need = s.storage_requirements64(16).size
            with pytest.raises(ValueError):
                sort_segments64(s, dk, do, storage=torch.empty(need - 16, dtype=torch.uint8, device="cuda"))
