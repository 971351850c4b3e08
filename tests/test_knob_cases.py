"""tests/knob_cases.py and tests/knob_battery_check.py without a GPU.

expected_plan against the compiled planner (tests/native/plan_check `describe` with the setting's knobs as arguments) at every
(n, mode) the battery uses, for 256 CUs and both rankings; the case lists: deterministic, non-empty, together naming every flat
vrdxHipCmd* entry point; and the battery itself -- run_battery of the child script -- over the default setting's small cases
against HostSorter, a sorter on host memory in the manner of test_guarded_call.FakeSorter that covers the rows of all five
tables and can be told to misbehave: a clean one passes every case, and each planted fault makes the battery report failures
that name the cases it must hit."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import key_order32_cases
import key_order_cases
import knob_battery_check as battery
import knob_cases
import plan_check_tool
import segmented_bits_cases
import segmented_cases
import sort_bits_cases
import storage_reuse_cases
import wide_value_cases
import wide_value_segmented_cases
from vulkan_radix_sort_amd import api

ALL_CALLS = (api.RECORDING_CALLS + api.ORDERED_SORT_CALLS + api.WIDE_VALUE_CALLS + api.WIDE_VALUE_SEGMENTED_CALLS
             + api.RANGE_SORT_CALLS)
RANGE_SORT_NAMES = {call.c_name for call in api.RANGE_SORT_CALLS}
WIDE_VALUE_NAMES = {call.c_name for call in api.WIDE_VALUE_CALLS + api.WIDE_VALUE_SEGMENTED_CALLS}
ORDERED32_NAMES = {call.c_name for call in api.ORDERED_SORT_CALLS}
HEADER = 16   # HostSorter's storage: four words, the failure word the last of them


# ---- the plans ---------------------------------------------------------------------------------------------------------------

def test_the_sizes_are_those_of_the_storage_reuse_cases():
    assert (knob_cases.M, knob_cases.H) == (storage_reuse_cases.M, storage_reuse_cases.H)
    assert knob_cases.M % 32768 != 0 and -(-knob_cases.M // 32768) == 251 <= 256   # one round of tiles: block sums apply


def test_the_settings():
    assert list(knob_cases.SETTINGS) == [
        "default", "small-sort-off", "hybrid-off", "msd-off", "msd-off-classic-lookback", "tiles-1024x8", "tiles-1024x16",
        "tiles-1024x32", "tiles-1024x32x2", "ballot-small-sort-off", "ballot-tiles-1024x32x2"]
    assert knob_cases.SETTINGS["default"] == {}
    for name, env in knob_cases.SETTINGS.items():
        assert set(env) <= set(knob_cases.KNOBS) | {"VRDX_RANK"} and (env.get("VRDX_RANK") == "ballot") == name.startswith("ballot-")


@pytest.mark.parametrize("atomic", [True, False], ids=["atomic", "ballot"])
@pytest.mark.parametrize("setting", list(knob_cases.SETTINGS))
def test_expected_plan_is_what_the_compiled_planner_records(setting, atomic):
    """every (n, mode) of every battery -- not of this setting's alone -- and the sizes either side of where a rule changes"""
    points = {(n, kind, key_value) for s in knob_cases.SETTINGS for n, kind, key_value, _ in knob_cases.plan_points(knob_cases.cases(s))}
    edges = [0, knob_cases.WIDE_ONE_WORKGROUP_MAX, knob_cases.ONE_WORKGROUP_MAX, knob_cases.HYBRID_LAST[True],
             knob_cases.HYBRID_LAST[False], knob_cases.MSD_LAST, knob_cases.WIDE_TWO_SORTS_FROM - 1]
    sizes = sorted({n for n, _, _ in points} | {e + d for e in edges for d in (0, 1)})
    table = plan_check_tool.describe(256, atomic, sizes, knobs=knob_cases.SETTINGS[setting])
    for n in sizes:
        for key_value in (False, True):
            row = table[n, key_value]
            got = (row.name, row.bits_plan, row.wide_form, row.wide_one_workgroup_max)
            want = (knob_cases.expected_plan(setting, n, key_value, "sort", atomic),
                    knob_cases.expected_plan(setting, n, key_value, "bits", atomic),
                    knob_cases.expected_plan(setting, n, key_value, "wide", atomic),
                    knob_cases.expected_wide_one_workgroup_max(setting))
            assert got == want, (setting, atomic, n, key_value)
            # the range sorts: part of the key by size alone, the whole key with the launches of the whole-key plan
            got = (row.range_form, row.range_whole_form, row.range_whole_launches, row.launches)
            launches = knob_cases.expected_launches(setting, n, key_value, atomic)
            want = (knob_cases.expected_plan(setting, n, key_value, "range", atomic, bit_range=(8, 16)),
                    knob_cases.expected_plan(setting, n, key_value, "range", atomic, bit_range=(0, 32)), launches, launches)
            assert got == want, (setting, atomic, n, key_value)
    assert all(kind == "wide" or (n, key_value) in table for n, kind, key_value in points)
    assert any(kind == "range" and n > knob_cases.ONE_WORKGROUP_MAX for n, kind, _ in points)


def test_a_partial_range_sort_is_planned_by_size_alone():
    """one workgroup up to 16384 elements, chunked beyond, under every setting; never "none": no size is refused"""
    for setting in knob_cases.SETTINGS:
        for key_value in (False, True):
            for r in knob_cases.RANGES[1:]:
                assert knob_cases.expected_plan(setting, 1, key_value, "range", bit_range=r) == "one-workgroup"
                assert knob_cases.expected_plan(setting, 16384, key_value, "range", bit_range=r) == "one-workgroup"
                assert knob_cases.expected_plan(setting, 16385, key_value, "range", bit_range=r) == "chunked"
                assert knob_cases.expected_plan(setting, knob_cases.M, key_value, "range", bit_range=r) == "chunked"
            assert knob_cases.expected_plan(setting, 100, key_value, "range", bit_range=(0, 32)) == "whole-key"
    launches = knob_cases.expected_launches
    assert launches("default", 100, False) == 1 and launches("small-sort-off", 100, False) == 5
    assert launches("default", knob_cases.H, True) == 6 and launches("hybrid-off", knob_cases.H, True) == 5
    assert launches("default", knob_cases.M, True) == 7 and launches("msd-off", knob_cases.M, True) == 5


def test_describe_without_knobs_is_what_it_was():
    """no knob argument: the rows of before, and the same plans as with the default spelled out"""
    sizes = [1, 16384, 16385, knob_cases.H, knob_cases.M]
    plain, knobbed = plan_check_tool.describe(256, True, sizes), plan_check_tool.describe(256, True, sizes, knobs={})
    assert all(type(row) is plan_check_tool.Row for row in plain.values())
    assert {k: row[:6] for k, row in knobbed.items()} == {k: tuple(row) for k, row in plain.items()}
    assert plain[knob_cases.H, True].name == "hybrid-8" and plain[knob_cases.M, False].name == "msd"


def test_the_chosen_sizes_sit_on_plans_the_knobs_take_away():
    for key_value in (False, True):
        assert knob_cases.expected_plan("default", knob_cases.H, key_value) == "hybrid-8"
        assert knob_cases.expected_plan("hybrid-off", knob_cases.H, key_value) == "four-passes"
        assert knob_cases.expected_plan("default", knob_cases.M, key_value) == "msd"
        assert knob_cases.expected_plan("msd-off", knob_cases.M, key_value) == "four-passes"
        for n in knob_cases.SMALL:
            small = n <= knob_cases.ONE_WORKGROUP_MAX
            assert knob_cases.expected_plan("default", n, key_value) == ("one-workgroup" if small else "hybrid-8")
            assert knob_cases.expected_plan("small-sort-off", n, key_value) == ("four-passes" if small else "hybrid-8")
            assert knob_cases.expected_plan("tiles-1024x16", n, key_value) == "four-passes"
            assert knob_cases.expected_plan("tiles-1024x16", n, key_value, "bits") == ("one-workgroup" if small else "none")
    assert knob_cases.expected_plan("small-sort-off", 100, True, "wide") == "gather"
    assert knob_cases.expected_plan("tiles-1024x8", 100, True, "wide") == "one-workgroup"


# ---- the case lists ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", list(knob_cases.SETTINGS))
def test_the_cases_are_deterministic_and_not_empty(setting):
    rows = knob_cases.cases(setting)
    assert rows and rows == knob_cases.cases(setting) and len({knob_cases.name_of(c) for c in rows}) == len(rows)
    known = {call.c_name for call in ALL_CALLS}
    assert all(case.entry in known for case in rows)
    case = next(c for c in rows if "KeyValue" in c.entry or "Wide" in c.entry)
    first = [a.copy() for a in knob_cases.inputs_of(case)[:2]]
    knob_cases.inputs_of.cache_clear()
    again = knob_cases.inputs_of(case)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert not np.array_equal(again[1][:case.n], np.arange(case.n)), "values must not be the index"


def test_the_batteries_by_group():
    groups = {s: sorted({c.group for c in knob_cases.cases(s)}) for s in knob_cases.SETTINGS}
    assert groups["default"] == ["large", "mid", "segmented", "small"]
    assert groups["hybrid-off"] == ["mid"] and groups["msd-off"] == groups["msd-off-classic-lookback"] == ["large"]
    assert all(groups[s] == ["segmented", "small"] for s in knob_cases.SMALL_SETTINGS if s != "default")
    small = [c for c in knob_cases.cases("small-sort-off") if c.group == "small"]
    assert {c.n for c in small if c.count is None} == set(knob_cases.SMALL) | {100}
    assert [c.entry for c in small if c.n == 100] == ["vrdxHipCmdSortBits"] and not small[[c.n for c in small].index(100)].refused
    assert {(c.n, c.count) for c in small if c.count is not None} == {
        (b, k) for b in knob_cases.INDIRECT_BOUNDS for k in (0, 1, b - 1, b, b + 7)}
    refused = [c for c in small if c.refused]
    assert refused and all(c.n == 16385 and c.bit_range != (0, 32) and "SortBits" in c.entry for c in refused)
    # the range sorts: the four RANGES at every size and count of the sweep, keys-only and key+value, none of them refused
    ranged = [c for c in small if "RangeSort" in c.entry]
    assert {(c.n, c.count, c.bit_range, "KeyValue" in c.entry) for c in ranged} == {
        (c.n, c.count, c.bit_range, "KeyValue" in c.entry) for c in small if "SortBits" in c.entry and c.n != 100}
    assert {c.bit_range for c in ranged} == set(knob_cases.RANGES) and not any(c.refused for c in ranged)
    assert any(c.n == 16385 and c.bit_range == (8, 16) for c in ranged)   # ... the chunked form under every small setting
    assert any(c.entry == "vrdxHipCmdSortBits" and c.bit_range == (8, 16) and c.count is None for c in refused)
    segmented = [c for c in knob_cases.cases("small-sort-off") if c.group == "segmented"]
    assert [c.entry.replace("vrdxHipCmd", "") for c in segmented] == [
        "SortSegmented", "SortSegmentedKeyValue", "SortSegmented64", "SortSegmented64KeyValue", "SortSegmentedBits",
        "OrderedSortSegmented", "WideValueSortSegmented"]
    sizes = sorted(np.diff(knob_cases.inputs_of(segmented[0])[2].astype(np.int64)).tolist())
    assert sizes == [0, 300, 4097, 9000, 20000]
    assert [(c.entry, c.n, c.count) for c in knob_cases.cases("msd-off")] == [
        ("vrdxHipCmdSort64", knob_cases.M, None), ("vrdxHipCmdSort64KeyValueIndirect", knob_cases.M, knob_cases.M - 3),
        ("vrdxHipCmdOrderedSortKeyValue", knob_cases.M, None), ("vrdxHipCmdWideValueSort", knob_cases.M, None)]
    assert {c.n for c in knob_cases.cases("hybrid-off")} == {16385, 40_001, 300_001}
    mid = [(c.entry, c.n, c.bit_range) for c in knob_cases.cases("hybrid-off") if "RangeSort" in c.entry]
    assert mid == [("vrdxHipCmdRangeSort", 40_001, (5, 22)), ("vrdxHipCmdRangeSort", knob_cases.H, (0, 32))]


def test_together_the_settings_name_every_flat_hip_entry_point():
    flat = {call.c_name for call in api.RECORDING_CALLS + api.ORDERED_SORT_CALLS + api.WIDE_VALUE_CALLS + api.RANGE_SORT_CALLS
            if call.c_name.startswith("vrdxHipCmd") and not call.facts[1]}
    assert len(flat) == 22 and RANGE_SORT_NAMES <= flat
    named = {case.entry for setting in knob_cases.SETTINGS for case in knob_cases.cases(setting)}
    assert flat <= named, sorted(flat - named)
    for setting in knob_cases.SMALL_SETTINGS:   # ... and every setting that reaches small sizes names them all by itself
        assert flat <= {case.entry for case in knob_cases.cases(setting)}


# ---- the battery against a sorter on host memory -------------------------------------------------------------------------------

def _view(address, count, dtype):
    raw = np.ctypeslib.as_array((ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(address))
    return raw.view(dtype)


FAULTS = ("dropped-scalar-tail",        # a streaming step of the 64-bit and wide-value sorts leaves out the last n % 4 elements
          "value-words-swapped",        # the 8-byte values come back with their words swapped
          "small-range-sorts-refused",  # a sort by part of the key is refused at a size it must be sorted at
          "range-sorts-follow-small-sort")  # vrdxHipCmdRangeSort* over part of the key is planned through the knob-dependent
#                                             answer: refused where VRDX_SMALL_SORT=0 leaves it no one-workgroup plan


class HostSorter:
    """The cmd_* methods of every row of the five tables and what the helpers and check_plans ask of a sorter, on host
    memory, sorting with the families' own references.  setting: the knobs it plans under (describe_*); fault: one of FAULTS."""

    def __init__(self, setting="default", fault=None):
        self.setting, self.fault, self.sticky = setting, fault, 0

    def _requirement(self, n, per_element):
        req = api.VrdxSorterStorageRequirements()
        req.size, req.usage = HEADER + per_element * n, api.STORAGE_USAGE
        return req

    def storage_requirements(self, n):
        return self._requirement(n, 8)

    def key_value_storage_requirements(self, n):
        return self._requirement(n, 16)

    def storage_requirements64(self, n, key_value=False):
        return self._requirement(n, 24 if key_value else 16)

    def wide_value_storage_requirements(self, n):
        return self._requirement(n, 24)

    def read_status(self, stream, storage, storage_offset=0):
        return int(_view(storage + storage_offset, 4, np.uint32)[3])

    def read_plan_verdict(self, stream, storage, storage_offset=0):
        return int(_view(storage + storage_offset, 4, np.uint32)[1])

    def read_sorter_status(self, stream):
        status, self.sticky = self.sticky, 0
        return status

    def _plan(self, n, key_value, kind):
        return SimpleNamespace(name=knob_cases.expected_plan(self.setting, n, key_value, kind),
                               oneWorkgroupMax=knob_cases.expected_wide_one_workgroup_max(self.setting))

    def describe_plan(self, n, key_value):
        return self._plan(n, key_value, "sort")

    def describe_ordered_sort_plan(self, n, key_value, order):
        return self._plan(n, key_value, "sort")

    def describe_sort_bits_plan(self, n, key_value, begin, end):
        return self._plan(n, key_value, "sort" if (begin, end) == (0, 32) else "bits")

    def describe_wide_value_sort_plan(self, n):
        return self._plan(n, True, "wide")

    def describe_range_sort_plan(self, n, key_value, begin, end):
        return SimpleNamespace(name=knob_cases.expected_plan(self.setting, n, key_value, "range", bit_range=(begin, end)),
                               launches=knob_cases.expected_launches(self.setting, n, key_value))

    def record(self, call, command_buffer, storage, storage_offset, query_pool, query, keys, keys_offset, element_count=None,
               max_element_count=None, segment_count=None, offsets=None, offsets_offset=None, indirect=None,
               indirect_offset=None, values=None, values_offset=None, begin_bit=None, end_bit=None, order=None):
        key_bits, segmented, is_indirect, key_value, extra = call.facts
        assert command_buffer == 0 and query_pool is None and query == 0
        wide_value = call.c_name in WIDE_VALUE_NAMES
        bound = max_element_count if segmented or is_indirect else element_count
        partial = extra == "Bits" and (begin_bit, end_bit) != (0, 32)
        ranged = call.c_name in RANGE_SORT_NAMES   # (no size is refused)
        refuse = partial and not segmented and not ranged and bound > knob_cases.ONE_WORKGROUP_MAX
        if self.fault == "small-range-sorts-refused" and partial and not segmented and not ranged:
            refuse = True
        if (self.fault == "range-sorts-follow-small-sort" and partial and ranged and bound <= knob_cases.ONE_WORKGROUP_MAX
                and knob_cases.SETTINGS[self.setting].get("VRDX_SMALL_SORT") == "0"):
            refuse = True
        if refuse:
            self.sticky |= api.STATUS_ENQUEUE_REFUSED
            return
        k = _view(keys + keys_offset, bound, np.uint32 if key_bits == 32 else np.uint64)
        v = _view(values + values_offset, bound, np.uint64 if wide_value else np.uint32) if key_value else None
        n = min(bound, int(_view(indirect + indirect_offset, 1, np.uint32)[0])) if is_indirect else bound
        if self.fault == "dropped-scalar-tail" and not segmented and (key_bits == 64 or wide_value):
            n -= n % 4
        o = _view(offsets + offsets_offset, segment_count + 1, np.uint32).copy() if segmented else None
        if extra == "Ordered" or call.c_name in ORDERED32_NAMES:
            module = key_order_cases if key_bits == 64 else key_order32_cases
            word = (module.ORDERS[order & 0xFF], bool(order & api.ORDER_DESCENDING))
        elif key_bits == 64:
            module, word = key_order_cases, ("uint64", False)
        else:
            word = None
        if segmented:
            if wide_value:
                sorted_k, sorted_v = wide_value_segmented_cases.expected(k, v, o, bound)
            elif extra == "Bits":
                sorted_k, sorted_v = segmented_bits_cases.expected(k, v, o, bound, begin_bit, end_bit)
            elif word is not None and word[0] not in ("uint64",):
                sorted_k, sorted_v = module.expected_segments(k, v, o, bound, *word)
            else:
                sorted_k, sorted_v = segmented_cases.expected(k, v, o, bound)
        elif wide_value:
            sorted_k, sorted_v = wide_value_cases.expected(k, v, n)
        elif extra == "Bits":
            sorted_k, sorted_v = sort_bits_cases.reference(k, v, begin_bit, end_bit, n)
        else:
            sorted_k, sorted_v = module.expected(k, v, *word, count=n)
        k[:] = sorted_k
        if key_value:
            if self.fault == "value-words-swapped" and wide_value:
                sorted_v = sorted_v.copy()
                sorted_v[:n] = (sorted_v[:n] >> np.uint64(32)) | (sorted_v[:n] << np.uint64(32))
            v[:] = sorted_v
        required = {(32, False): self.storage_requirements, (32, True): self.key_value_storage_requirements,
                    (64, False): self.storage_requirements64,
                    (64, True): lambda m: self.storage_requirements64(m, True)}[key_bits, key_value and not wide_value](bound)
        if wide_value:
            required = self.wide_value_storage_requirements(bound)
        if bound > 0 and (not segmented or segment_count > 0):
            scratch = _view(storage + storage_offset, required.size, np.uint8)
            scratch[:] = 0x11                     # the requirement is the sorter's to write
            scratch[:HEADER].view(np.uint32)[:] = [n, 0, 0, 0]


def _method(call):
    names = [name for name, _ in call.parameters]

    def method(self, *args):
        assert len(args) == len(names), (call.method, len(args))
        self.record(call, **dict(zip(names, args)))
    return method


for _call in ALL_CALLS:
    setattr(HostSorter, _call.method, _method(_call))

SMALL_ROWS = [c for c in knob_cases.cases("default") if c.group in ("small", "segmented")]


def _run(sorter, setting, rows):
    lines = []
    failures = battery.run_battery(torch, sorter, setting, rows, device="cpu", out=lines.append)
    assert lines[-1] == f"{len(rows)} cases, {failures} failures"
    return failures, lines


def test_the_default_batterys_small_cases_pass_on_a_correct_sorter():
    failures, lines = _run(HostSorter(), "default", SMALL_ROWS)
    assert failures == 0, [line for line in lines if line.startswith("FAIL")][:5]
    # one line per plan point and per case, the refused rows among them
    assert len(lines) == len(knob_cases.plan_points(SMALL_ROWS)) + len(SMALL_ROWS) + 1
    assert sum("refused" in line for line in lines) == sum(c.refused for c in SMALL_ROWS) > 0


def _failed(lines):
    return {line[5:].split(":")[0] for line in lines if line.startswith("FAIL")}


def test_a_dropped_scalar_tail_is_reported_by_case():
    rows = [c for c in SMALL_ROWS if c.n in (1, 3, 5, 255, 4097, 8192) and c.group == "small"]
    failures, lines = _run(HostSorter(fault="dropped-scalar-tail"), "default", rows)
    hit = {knob_cases.name_of(c) for c in rows if ("Sort64" in c.entry or "WideValueSort" in c.entry)
           and knob_cases.sorted_count(c) % 4 != 0 and knob_cases.sorted_count(c) > 1}
    # (keys of seven values or fewer may leave a tail of two already in order: every failure is one of `hit`, and the sizes
    # with random 64-bit keys are all among them)
    assert _failed(lines) <= hit and failures == len(_failed(lines)) > 0
    assert {"vrdxHipCmdSort64 n=5", "vrdxHipCmdSort64KeyValue n=4097", "vrdxHipCmdWideValueSort n=255",
            "vrdxHipCmdSort64KeyValueIndirect n=8192 count=8191"} <= _failed(lines)


def test_swapped_value_words_are_reported_by_case():
    rows = [c for c in SMALL_ROWS if "Wide" in c.entry or c.entry == "vrdxHipCmdSort64KeyValue"]
    failures, lines = _run(HostSorter(fault="value-words-swapped"), "default", rows)
    hit = {knob_cases.name_of(c) for c in rows if "Wide" in c.entry and knob_cases.sorted_count(c) > 0}
    assert _failed(lines) == hit and failures == len(hit) > 0
    assert all("values:" in line for line in lines if line.startswith("FAIL"))
    assert "vrdxHipCmdWideValueSortSegmented n=%d" % rows[-1].n in hit


def test_a_refusal_that_should_not_be_is_reported_by_case():
    rows = [c for c in SMALL_ROWS if "Bits" in c.entry]
    failures, lines = _run(HostSorter(fault="small-range-sorts-refused"), "default", rows)
    hit = {knob_cases.name_of(c) for c in rows if "Segmented" not in c.entry and c.bit_range != (0, 32) and not c.refused}
    assert all("SortBits" in name for name in hit)
    assert _failed(lines) == hit and failures == len(hit) > 0
    assert all("the call was refused" in line for line in lines if line.startswith("FAIL"))
    assert "vrdxHipCmdSortBits n=255 bits=[8,16)" in hit
    # ... and a call that must be refused and is sorted instead
    control = [c for c in rows if c.refused and c.count is None and c.bit_range == (8, 16) and c.entry == "vrdxHipCmdSortBits"]

    class Sorts(HostSorter):
        def record(self, call, *args, **kw):
            if "begin_bit" in kw:
                kw["begin_bit"], kw["end_bit"] = 0, 32   # (the whole-key sort is not refused at any size)
            super().record(call, *args, **kw)

    failures, lines = _run(Sorts(), "default", control)
    assert failures == len(control) == 1 and "must be refused" in lines[-2]


@pytest.mark.parametrize("setting", list(knob_cases.SETTINGS))
def test_the_range_sorts_of_every_setting_pass_on_a_correct_sorter(setting):
    """every vrdxHipCmdRangeSort* case of the setting's battery, plans included, against a sorter that plans under that
    setting: part of the key by size alone, the whole key with the launches of the setting's whole-key plan"""
    rows = [c for c in knob_cases.cases(setting) if "RangeSort" in c.entry]
    small, mid = setting in knob_cases.SMALL_SETTINGS, setting in knob_cases.MID_SETTINGS
    assert len(rows) == 200 * small + 2 * mid and not any(c.refused for c in rows)
    if not rows:   # (the settings of the large group alone: the range sorts are not part of their battery)
        return
    failures, lines = _run(HostSorter(setting), setting, rows)
    assert failures == 0, [line for line in lines if line.startswith("FAIL")][:5]
    assert sum(line.startswith("ok   range-sort plan") for line in lines) == len(knob_cases.plan_points(rows))
    if small:   # the whole-key plan's launches follow the knobs; the partial ranges do not notice them
        sorter = HostSorter(setting)
        assert sorter.describe_range_sort_plan(16385, False, 8, 16).name == "chunked"
        assert sorter.describe_range_sort_plan(100, False, 0, 32).launches == knob_cases.expected_launches(setting, 100, False)


def test_a_range_sort_refused_without_the_small_sort_is_reported_by_case():
    """PlanSortBits' regression, on the entry points that took its place at every size: the one-workgroup range sorts refused
    under VRDX_SMALL_SORT=0.  The default setting does not show it; small-sort-off names every case."""
    rows = [c for c in knob_cases.cases("small-sort-off") if "RangeSort" in c.entry and c.n in (5, 255, 8192, 16384, 16385)]
    assert any(c.count is not None for c in rows) and any(c.n > knob_cases.ONE_WORKGROUP_MAX for c in rows)
    assert _run(HostSorter("small-sort-off"), "small-sort-off", rows)[0] == 0
    default_rows = [c for c in SMALL_ROWS if "RangeSort" in c.entry and c.n in (5, 255, 8192, 16384, 16385)]
    assert _run(HostSorter("default", fault="range-sorts-follow-small-sort"), "default", default_rows)[0] == 0
    failures, lines = _run(HostSorter("small-sort-off", fault="range-sorts-follow-small-sort"), "small-sort-off", rows)
    hit = {knob_cases.name_of(c) for c in rows if c.bit_range != (0, 32) and c.n <= knob_cases.ONE_WORKGROUP_MAX}
    assert _failed(lines) == hit and failures == len(hit) > 0
    assert all("the call was refused" in line for line in lines if line.startswith("FAIL"))
    assert {"vrdxHipCmdRangeSort n=255 bits=[8,16)", "vrdxHipCmdRangeSortKeyValueIndirect n=8192 count=0 bits=[5,22)"} <= hit
    assert "vrdxHipCmdRangeSort n=16385 bits=[8,16)" not in hit   # (the chunked form never went through that answer)


def test_a_setting_that_did_not_arrive_fails_on_the_plan_lines():
    """the battery of small-sort-off on a sorter that plans with the default knobs: the sorts are right, the plans are not"""
    rows = [c for c in knob_cases.cases("small-sort-off") if c.n in (5, 8193) and c.count is None]
    failures, lines = _run(HostSorter("default"), "small-sort-off", rows)
    wrong = [line for line in lines if line.startswith("FAIL")]
    assert failures == len(wrong) > 0 and all(" plan n=" in line and "expected" in line for line in wrong)
    assert any(line.startswith("FAIL wide-value plan n=5") for line in wrong)
    assert _run(HostSorter("small-sort-off"), "small-sort-off", rows)[0] == 0
