"""Without a GPU: the plan and the layout of the range sorts at every size (vrdx_plan.h, PlanRangeSort; vrdx_layout.h,
MakeRangeSortLayout and the chunk formula) through tests/native/range_sort_plan_check.cpp, compiled here, for devices of 8 and
of 256 CUs -- every n from 16380 to 16400, either side of cus * 8192, cus * 16384 and 2 * cus * 16384, and 2^30 - 4; per size
every range width, both modes, both rankings, every storage address modulo 128 -- and the chunk formula of
tests/range_sort_cases.py held to what the planner prints.  The same program also runs under ASan + UBSan."""
import os
import subprocess

import pytest

import range_sort_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "range_sort_plan_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
MAX_ELEMENTS = (1 << 30) - 4
CUS = (8, 256)


def sizes(cus):
    edges = [edge + d for edge in (cus * 8192, cus * 16384, 2 * cus * 16384) for d in (-1, 0, 1)]
    return sorted(set(list(range(16380, 16401)) + edges + cases.large_sizes(cus) + [0, 1, 65539, MAX_ELEMENTS]))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__",
                    SOURCE, "-o", str(exe)] + extra, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("range_sort_plan"), "range_sort_plan_check", ["-O2"])
    return {cus: subprocess.run([exe, str(cus)] + [str(n) for n in sizes(cus)], capture_output=True, text=True, timeout=600)
            for cus in CUS}


@pytest.mark.parametrize("cus", CUS)
def test_every_width_mode_and_address_at_every_size(reports, cus):
    report = reports[cus]
    assert report.returncode == 0 and ", 0 failures" in report.stdout, report.stdout[-3000:] + report.stderr[-2000:]
    # per size, ranking, mode and address: four other ranges, and 31 widths at the bottom and at the top of the key
    assert f"range sort plan: {len(sizes(cus)) * 2 * 2 * 128 * (4 + 62)} cases" in report.stdout


@pytest.mark.parametrize("cus", CUS)
def test_the_model_and_the_planner_cut_the_same_chunks(reports, cus):
    got = {}
    for line in reports[cus].stdout.splitlines():
        if line.startswith("plan "):
            _, units, n, grid, keys = line.split()
            assert int(units) == cus
            got[int(n)] = (int(grid), int(keys))
    assert sorted(got) == sizes(cus)
    for n, (grid, keys) in got.items():
        if n <= cases.ONE_WORKGROUP_MAX:
            assert (grid, keys) == (0, 0), n
            continue
        assert grid == cases.sort_grid(n, cus) and keys == cases.chunk_keys(n, cus), n
        used = -(-n // keys)   # the chunks cover [0, n) exactly once, with at most one per workgroup
        assert keys >= cases.CHUNK_MIN and keys % 256 == 0 and used <= grid and (used - 1) * keys < n <= used * keys, n
    # the sizes of the GPU tests take one, one, one, two and three tiles per chunk
    assert [-(-got[n][1] // cases.TILE) for n in cases.large_sizes(cus)] == [1, 1, 1, 2, 3]
    assert got[cases.indirect_bound(cus)][1] > cases.TILE


def test_the_plan_check_under_address_and_ub_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = _build(tmp_path, "range_sort_plan_check_sanitized", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "256", "1", "16384", "16385", "4194305", str(MAX_ELEMENTS)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
