"""The composed sorts -- 64-bit, ordered, by a bit range (the range sorts at every size among them), with 8-byte values -- under
every planning knob, on the device: one
test per setting of tests/knob_cases.py, each ONE fresh child (tests/knob_battery_check.py) with the setting's environment,
because the library reads the knobs once per process.  The child checks the plans first, so a setting that did not arrive
fails there; then every case of the setting, guarded and bit for bit.  Children never run concurrently, and after one that
ended abnormally -- by a signal, by the timeout, or with an illegal-access error of the HIP runtime -- no other is started."""
import os
import re
import subprocess
import sys

import pytest

import knob_cases
from guarded_call import sorter, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "knob_battery_check.py")
ABNORMAL = []   # the latch: the name of the setting whose child ended abnormally


@pytest.fixture(scope="module")
def sizes_on_the_plans_the_knobs_take_away(sorter):
    """before the first child, on this process's own default sorter: the mid and large sizes do sit on the hybrid and the MSD
    plan"""
    assert sorter.describe_plan(knob_cases.H, True).name == "hybrid-8"
    for key_value in (False, True):
        assert sorter.describe_plan(knob_cases.M, key_value).name == "msd"


@pytest.mark.parametrize("name", list(knob_cases.SETTINGS))
def test_the_battery_under(name, sizes_on_the_plans_the_knobs_take_away):
    assert not ABNORMAL, f"not started: {ABNORMAL[0]} ended abnormally"
    env = dict(os.environ, **knob_cases.SETTINGS[name])
    try:
        r = subprocess.run([sys.executable, CHILD, name], env=env, timeout=600, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        ABNORMAL.append(name)
        pytest.fail(f"{name}: the child ran into the timeout; its last lines:\n{(e.stdout or b'')[-2000:]}")
    out = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in out:
        ABNORMAL.append(name)
    lines = r.stdout.strip().splitlines()
    report = "\n".join([line for line in lines if line.startswith("FAIL")][:20] + lines[-3:]) + r.stderr[-2000:]
    assert r.returncode == 0, f"{name}: exit status {r.returncode}\n{report}"
    verdict = re.fullmatch(r"(\d+) cases, (\d+) failures", lines[-1])
    assert verdict is not None and verdict.group(2) == "0", report
    assert int(verdict.group(1)) == len(knob_cases.cases(name)), report
