"""Without a GPU: the plan of the bit-range sorts (vrdx_plan.h, PlanSortBits) through tests/native/sort_bits_plan_check.cpp,
compiled here -- every range at the sizes of the GPU tests, both rankings, keys-only and key+value: one workgroup and one
launch up to 16384 elements, refused beyond, under every setting of VRDX_SMALL_SORT and VRDX_TILE_CONFIG (a range over part
of the key is planned by size alone), the full range equal to the whole-key plan under the same knobs -- and the size lists of
tests/test_sort_bits_gpu.py held to what the planner prints.  The same program also runs under ASan + UBSan."""
import os
import subprocess

import pytest

import sort_bits_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "sort_bits_plan_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SIZES = sorted(set(cases.ONE_WORKGROUP_SIZES + cases.REFUSED_SIZES + cases.BALLOT_SIZES + cases.INDIRECT_BOUNDS
                   + cases.BUILDER_SIZES + [8_400_000]))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__",
                    SOURCE, "-o", str(exe)] + extra, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("sort_bits_plan"), "sort_bits_plan_check", ["-O2"])
    return subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=300)


def test_every_range_at_the_sizes_of_the_gpu_tests(report):
    assert report.returncode == 0 and ", 0 failures" in report.stdout, report.stdout[-3000:] + report.stderr[-2000:]
    # 33 x 34 / 2 + 33 (b, e) pairs with b <= e <= 33 per size, ranking, value mode and setting of the knobs (smallSort on and
    # off times forcedConfig -1, 0 ... 3)
    assert f"sort bits plan: {len(SIZES) * 4 * 10 * (33 * 34 // 2 + 33)} cases" in report.stdout


def test_the_gpu_tests_sizes_take_the_plan_they_claim(report):
    got = {}
    for line in report.stdout.splitlines():
        if line.startswith("plan "):
            _, n, atomic, key_value, what = line.split()
            got[int(n), atomic == "1", key_value == "1"] = what
    sorted_sizes = cases.ONE_WORKGROUP_SIZES + cases.BALLOT_SIZES + cases.INDIRECT_BOUNDS + cases.BUILDER_SIZES
    for n in SIZES:
        for atomic in (True, False):
            for key_value in (False, True):
                assert got[n, atomic, key_value] == ("one-workgroup" if n in sorted_sizes else "refused"), (n, atomic, key_value)
    assert all(n > 16384 for n in cases.REFUSED_SIZES) and max(sorted_sizes) == 16384
    # both one-workgroup kernels: 256 threads up to 4096 elements, 1024 threads beyond
    assert any(n <= 4096 for n in sorted_sizes) and any(n > 4096 for n in sorted_sizes)


def test_the_plan_check_under_address_and_ub_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = _build(tmp_path, "sort_bits_plan_check_sanitized", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "1", "16384", "16385", "8400000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
