"""Without a GPU: the plan and the layout of the balanced segmented sort (vrdx_plan.h, PlanBalancedSegmentedSort;
vrdx_layout.h, MakeBalancedSegmentedLayout and the two caps) through tests/native/balanced_segmented_plan_check.cpp, compiled
here, for devices of 8 and of 256 CUs -- every maxElementCount from 65500 to 65600, either side of every multiple of 65537 and
16384 that changes a cap up to five segments, samples up to 2^30 - 4; per bound both modes, both rankings, three segment
counts and every storage address modulo 128 -- and the caps and offsets of tests/balanced_segmented_cases.py held to what
the planner prints.  The same program also runs under ASan + UBSan."""
import os
import subprocess

import pytest

import balanced_segmented_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "balanced_segmented_plan_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CUS = (8, 256)


def sizes():
    edges = [k * unit + d for unit in (65537, 16384) for k in range(1, 6) for d in (-1, 0, 1)]
    samples = [0, 1, 4097, 16385, 1 << 20, (1 << 22) + 3, 85 * 65537, 86 * 65537, 256 * 16384 + 5, 1 << 24, (1 << 27) + 1,
               (1 << 29) + 77, cases.MAX_ELEMENTS - 1, cases.MAX_ELEMENTS]
    return sorted(set(list(range(65500, 65601)) + edges + samples))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__",
                    SOURCE, "-o", str(exe)] + extra, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("balanced_plan"), "balanced_segmented_plan_check", ["-O2"])
    return {cus: subprocess.run([exe, str(cus)] + [str(n) for n in sizes()], capture_output=True, text=True, timeout=600)
            for cus in CUS}


@pytest.mark.parametrize("cus", CUS)
def test_every_mode_and_address_at_every_bound(reports, cus):
    report = reports[cus]
    assert report.returncode == 0 and ", 0 failures" in report.stdout, report.stdout[-3000:] + report.stderr[-2000:]
    assert f"balanced segmented plan: {len(sizes()) * 2 * 2 * 3 * 128} cases" in report.stdout


@pytest.mark.parametrize("cus", CUS)
def test_the_model_and_the_planner_agree_on_the_form_and_the_caps(reports, cus):
    got = {}
    for line in reports[cus].stdout.splitlines():
        if line.startswith("plan "):
            _, units, n, form, spread, pieces, *offsets = line.split()
            assert int(units) == cus
            got[int(n)] = (int(form), int(spread), int(pieces))
            if int(form) == 2:   # the offsets the GPU tests look at, at address 127
                model = cases.layout(int(n), cus, address=127)
                assert [int(o) for o in offsets] == [model["split"], model["keysScratch"], model["valuesScratch"]], n
    assert sorted(got) == sizes()
    for n, (form, spread, pieces) in got.items():
        balanced = n > cases.SPREAD_FROM
        assert form == (2 if balanced else 1 if n else 0), n
        assert (spread, pieces) == ((cases.spread_cap(n, cus), cases.piece_cap(n, cus)) if balanced else (0, 0)), n
    assert got[65536][0] == 1 and got[65537] == (2, 1, 5)
    assert got[cases.MAX_ELEMENTS] == (2, (cus - 1) // 3, cus + (cus - 1) // 3)


def test_the_plan_check_under_address_and_ub_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = _build(tmp_path, "balanced_segmented_plan_check_sanitized", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "256", "0", "1", "65536", "65537", "4194305", str(cases.MAX_ELEMENTS)], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
