"""Replays tests/golden/front_end_cases.json against the five torch front ends of the working tree: for every recorded call --
every valid combination of the optional arguments, and every fault alone and paired with every other -- the same exception
type with the same message, character for character, or the same recording call with the same arguments.  The file was
recorded by tests/golden/make_front_end_cases.py from the package as it stood before the front ends shared their checks
(vulkan_radix_sort_amd/_checks.py) and their dispatcher (api.record_sort); the script has to reproduce it byte for byte."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_script():
    spec = importlib.util.spec_from_file_location("make_front_end_cases", os.path.join(GOLDEN, "make_front_end_cases.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


script = _load_script()


@pytest.fixture(scope="module")
def fixture():
    with open(script.FIXTURE) as f:
        return json.load(f)


def _replay(fixture, section, name):
    import torch
    import vulkan_radix_sort_amd as package
    assert fixture["cases"][name] == script.case_lists(name)
    recorded = script.unpack(name, fixture[section][name])
    assert len(recorded) > 200
    now = script.cases(torch, package, section, name)
    assert now == recorded
    assert script.pack(now) == fixture[section][name]


@pytest.mark.parametrize("name", list(script.FRONT_ENDS))
def test_front_end_on_cpu_tensors(fixture, name):
    _replay(fixture, "cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(script.FRONT_ENDS))
def test_front_end_on_gpu_tensors(fixture, name):
    _replay(fixture, "cuda", name)
    recorded = script.unpack(name, fixture["cuda"][name])
    assert all(" | returns " in outcome for case, outcome in recorded.items() if case.startswith("valid: ")), name


@pytest.mark.gpu
def test_the_script_reproduces_the_file_byte_for_byte():
    import torch
    import vulkan_radix_sort_amd as package
    with open(script.FIXTURE) as f:
        assert script.render(script.record(torch, package, script.SECTIONS)) == f.read()
