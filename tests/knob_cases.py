"""What tests/test_knobs_gpu.py (on the GPU, through tests/knob_battery_check.py) and tests/test_knob_cases.py (without one)
share: the planning knobs of the library as SETTINGS, the plan the host must report under each of them (expected_plan, written
out from the rules of vrdx_plan.h and held to the compiled planner by tests/test_knob_cases.py), and cases(setting), the
battery of composed sorts -- 64-bit, ordered, by a bit range (vrdxHipCmdSortBits* and vrdxHipCmdRangeSort*), with 8-byte
values: all twenty-two flat vrdxHipCmd* entry points -- that runs under that setting.  A plain
module next to storage_reuse_cases.py, imported the same way; it needs numpy only.

The knobs are read once per process (vrdx_api.cpp, EnvKnobs), so a setting is the environment of a fresh child.  They send the
32-bit sorts INSIDE the composed sorts down kernels the size-adaptive choice never takes at that size: the general path at
1 ... 16384 elements (VRDX_SMALL_SORT=0, any VRDX_TILE_CONFIG), four passes at the hybrid plan's sizes (VRDX_HYBRID=0) and at
the MSD plan's (VRDX_MSD=0: block sums; with VRDX_BLOCK_SUMS=0 the classic look-back).  The segmented sorts and the sorts
over part of the key take no notice of them -- vrdxHipCmdSortBits* and, at every size, the chunked form included,
vrdxHipCmdRangeSort* --; the battery holds them to that.  A range sort over (0, 32) is the whole-key sort, knobs and all.

Keys, values and references are those of the case modules of each family -- sort64_model / key_order_cases,
key_order32_cases, sort_bits_cases, wide_value_cases, segmented_cases, segmented64_cases, segmented_bits_cases,
wide_value_segmented_cases -- bit for bit against a stable numpy sort; values are never the index."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import key_order32_cases
import key_order_cases
import segmented64_cases
import segmented_bits_cases
import segmented_cases
import sort64_model
import sort_bits_cases
import wide_value_cases
import wide_value_segmented_cases

M = 8_200_003     # M and H of storage_reuse_cases.py (not imported: that module pulls in the GPU tests of the plain sorts):
H = 300_001       # the MSD plan by ten bits -- 251 tiles of 32768, one round: block sums apply -- and the hybrid plan
ONE_WORKGROUP_MAX = 16_384          # kSmallSortMaxElements (vrdx_kernels.h)
WIDE_ONE_WORKGROUP_MAX = wide_value_cases.ONE_WORKGROUP_MAX   # kWideSmallMaxElements
WIDE_TWO_SORTS_FROM = 1 << 24       # kWideValueTwoSortsFrom (vrdx_plan.h)
HYBRID_LAST = {True: 8_144_384, False: 4_072_192}   # HybridCapacity's last size: one-atomic ranking, ballot ranking
MSD_LAST = 67_108_864               # MsdBits' last size (one-atomic ranking only)
MSD_HALF_LAST = 18_149_376          # ... with the half-size bucket kernel, one launch more

SETTINGS = {
    "default": {},
    "small-sort-off": {"VRDX_SMALL_SORT": "0"},
    "hybrid-off": {"VRDX_HYBRID": "0"},
    "msd-off": {"VRDX_MSD": "0"},
    "msd-off-classic-lookback": {"VRDX_MSD": "0", "VRDX_BLOCK_SUMS": "0"},
    "tiles-1024x8": {"VRDX_TILE_CONFIG": "1024x8"},
    "tiles-1024x16": {"VRDX_TILE_CONFIG": "1024x16"},
    "tiles-1024x32": {"VRDX_TILE_CONFIG": "1024x32"},
    "tiles-1024x32x2": {"VRDX_TILE_CONFIG": "1024x32x2"},
    "ballot-small-sort-off": {"VRDX_RANK": "ballot", "VRDX_SMALL_SORT": "0"},
    # (key+value and the ballot ranking fall to 1024x32: ConfigIndex, vrdx_plan.h)
    "ballot-tiles-1024x32x2": {"VRDX_RANK": "ballot", "VRDX_TILE_CONFIG": "1024x32x2"},
}
KNOBS = ("VRDX_SMALL_SORT", "VRDX_HYBRID", "VRDX_MSD", "VRDX_BLOCK_SUMS", "VRDX_TILE_CONFIG")   # (VRDX_RANK picks the sorter)


def expected_plan(setting, n, key_value, kind="sort", atomic=None, bit_range=None):
    """The name the host must report for n elements under a setting.  kind "sort": vrdxHipDescribePlan,
    vrdxHipDescribeOrderedSortPlan and vrdxHipDescribeSortBitsPlan over (0, 32) (api.PLAN_NAMES; the same with and without
    values); "bits": vrdxHipDescribeSortBitsPlan over part of the key; "wide": the form of vrdxHipDescribeWideValueSortPlan
    (api.WIDE_VALUE_FORM_NAMES); "range": the form of vrdxHipDescribeRangeSortPlan over `bit_range`
    (api.RANGE_SORT_FORM_NAMES) -- over (0, 32) "whole-key", whose launches are those of kind "sort" under the same
    setting (expected_launches).  atomic: the ranking (default: the setting's sorter)."""
    env = SETTINGS[setting]
    atomic = env.get("VRDX_RANK") != "ballot" if atomic is None else atomic
    small_sort = env.get("VRDX_SMALL_SORT") != "0"
    tiles = "VRDX_TILE_CONFIG" in env
    hybrid = env.get("VRDX_HYBRID") != "0"
    msd = hybrid and env.get("VRDX_MSD") != "0"
    if n == 0:
        return "none"
    if kind == "bits":     # by size alone: no knob reaches a range sort (PlanSortBits)
        return "one-workgroup" if n <= ONE_WORKGROUP_MAX else "none"
    if kind == "range":    # PlanRangeSort: the whole key is PlanSort itself; part of it by size alone, and never refused
        if bit_range == (0, 32):
            return "whole-key"
        return "one-workgroup" if n <= ONE_WORKGROUP_MAX else "chunked"
    if kind == "wide":     # PlanWideValueSort looks at VRDX_SMALL_SORT only: a forced tile geometry keeps one workgroup
        if n <= WIDE_ONE_WORKGROUP_MAX and small_sort:
            return "one-workgroup"
        return "gather" if n < WIDE_TWO_SORTS_FROM else "two-sorts"
    assert kind == "sort", kind
    if tiles:              # a forced geometry is the general path at every size, with no plan in front
        return "four-passes"
    if n <= ONE_WORKGROUP_MAX:
        return "one-workgroup" if small_sort else "four-passes"
    if not hybrid:
        return "four-passes"
    if n <= HYBRID_LAST[atomic]:
        return "hybrid-8"
    return "msd" if msd and atomic and n <= MSD_LAST else "four-passes"


LAUNCHES = {"none": 0, "one-workgroup": 1, "four-passes": 5, "hybrid-8": 6}   # (plan_check_tool's tables; msd: 7 | 6)


def expected_launches(setting, n, key_value, atomic=None):
    """the launches of the whole-key plan (kind "sort") under a setting, which a range sort over (0, 32) must report as its own"""
    name = expected_plan(setting, n, key_value, "sort", atomic)
    return (7 if n <= MSD_HALF_LAST else 6) if name == "msd" else LAUNCHES[name]


def expected_wide_one_workgroup_max(setting):
    """oneWorkgroupMax of vrdxHipDescribeWideValueSortPlan"""
    return 0 if SETTINGS[setting].get("VRDX_SMALL_SORT") == "0" else WIDE_ONE_WORKGROUP_MAX


# ---- the battery -------------------------------------------------------------------------------------------------------------

SMALL = (1, 2, 3, 5, 255, 4097, 8192, 8193, 16384, 16385)
INDIRECT_BOUNDS = (5, 8192, 16385)
MID = (16385, 40_001, H)
RANGES = ((0, 32), (8, 16), (5, 22), (31, 32))
REFUSED_CONTROL = (16385, (8, 16))
REGRESSION_RANGE_SORT = (100, (8, 16))
SEGMENT_SIZES = (300, 4097, 9000, 20000, 0)   # every size class of every family, and an empty segment
TAIL = 3                                      # elements behind the count, which the call must leave alone
ORDERS64 = (("int64", False, "mixed-int"), ("float64", True, "float-specials"))
ORDERS32 = (("int32", False, "mixed-int"), ("float32", True, "float-specials"))
FLOAT32_DESCENDING = ("float32", True, "float-specials")

SMALL_SETTINGS = ("default", "small-sort-off", "tiles-1024x8", "tiles-1024x16", "tiles-1024x32", "tiles-1024x32x2",
                  "ballot-small-sort-off", "ballot-tiles-1024x32x2")
MID_SETTINGS = ("default", "hybrid-off")
LARGE_SETTINGS = ("default", "msd-off", "msd-off-classic-lookback")

# group: "small" | "segmented" | "mid" | "large".  entry: the C entry point.  n: elementCount / maxElementCount; the arrays are
# TAIL elements longer.  count: the device-side count of an indirect form, else None.  bit_range: (begin, end) or None.
# order: (key type, descending, key builder) or None.  refused: the call must be refused and leave everything as it was.
Case = namedtuple("Case", "group entry n count bit_range order refused")


def name_of(case):
    parts = [case.entry, f"n={case.n}"]
    if case.count is not None:
        parts.append(f"count={case.count}")
    if case.bit_range is not None:
        parts.append("bits=[%d,%d)" % case.bit_range)
    if case.order is not None:
        parts.append(case.order[0] + ("-descending" if case.order[1] else ""))
    if case.refused:
        parts.append("refused")
    return " ".join(parts)


def seed_of(case):
    return zlib.crc32(("knobs/" + name_of(case)).encode())


def _flat(group, family, n, count=None, key_value=False, bit_range=None, order=None):
    """One flat call of a family: "Sort64" | "Sort64Ordered" | "OrderedSort" | "SortBits" | "RangeSort" | "WideValueSort" """
    entry = "vrdxHipCmd" + family + ("KeyValue" if key_value else "") + ("Indirect" if count is not None else "")
    # (vrdxHipCmdSortBits* refuse part of the key beyond one workgroup; vrdxHipCmdRangeSort* refuse no size)
    refused = family == "SortBits" and bit_range != (0, 32) and n > ONE_WORKGROUP_MAX
    return Case(group, entry, n, count, bit_range, order, refused)


def _family_rows(group, n, count=None):
    """every flat entry point of the battery at one size (an indirect twin with a device-side count)"""
    rows = []
    for key_value in (False, True):
        rows.append(_flat(group, "Sort64", n, count, key_value))
        rows += [_flat(group, "Sort64Ordered", n, count, key_value, order=order) for order in ORDERS64]
        rows += [_flat(group, "OrderedSort", n, count, key_value, order=order) for order in ORDERS32]
        rows += [_flat(group, "SortBits", n, count, key_value, bit_range=r) for r in RANGES]
        rows += [_flat(group, "RangeSort", n, count, key_value, bit_range=r) for r in RANGES]
    rows.append(_flat(group, "WideValueSort", n, count))
    return rows


def _small_cases():
    rows = []
    for n in SMALL:
        rows += _family_rows("small", n)
    for bound in INDIRECT_BOUNDS:
        for count in (0, 1, bound - 1, bound, bound + 7):
            rows += _family_rows("small", bound, count)
    # the regression case of PlanSortBits: refused with VRDX_HIP_STATUS_ENQUEUE_REFUSED under VRDX_SMALL_SORT=0 and under every
    # VRDX_TILE_CONFIG while the range sorts were planned through PlanSort's knob-dependent answer
    rows.append(_flat("small", "SortBits", REGRESSION_RANGE_SORT[0], bit_range=REGRESSION_RANGE_SORT[1]))
    control = _flat("small", "SortBits", REFUSED_CONTROL[0], bit_range=REFUSED_CONTROL[1])
    assert control.refused and control in rows   # (the sweep above holds it: 16385 is one of SMALL)
    # the knobs must not reach these: one mixed-class call per family
    n = sum(SEGMENT_SIZES) + 100 + 77            # (segmented_cases.mixed_offsets: 100 elements in front, 77 behind)
    rows += [Case("segmented", "vrdxHipCmdSortSegmented", n, None, None, None, False),
             Case("segmented", "vrdxHipCmdSortSegmentedKeyValue", n, None, None, None, False),
             Case("segmented", "vrdxHipCmdSortSegmented64", n, None, None, None, False),
             Case("segmented", "vrdxHipCmdSortSegmented64KeyValue", n, None, None, None, False),
             Case("segmented", "vrdxHipCmdSortSegmentedBits", n, None, (5, 22), None, False),
             Case("segmented", "vrdxHipCmdOrderedSortSegmented", n, None, None, FLOAT32_DESCENDING, False),
             Case("segmented", "vrdxHipCmdWideValueSortSegmented", n, None, None, None, False)]
    return rows


def _mid_cases():
    rows = []
    for n in MID:
        rows += [_flat("mid", "Sort64", n, key_value=True), _flat("mid", "OrderedSort", n, key_value=True, order=FLOAT32_DESCENDING),
                 _flat("mid", "SortBits", n, bit_range=(0, 32)), _flat("mid", "WideValueSort", n)]
    # the range sorts beyond one workgroup: the chunked form, which no knob may reach, and the whole key at the hybrid plan's size
    rows += [_flat("mid", "RangeSort", 40_001, bit_range=(5, 22)), _flat("mid", "RangeSort", H, bit_range=(0, 32))]
    return rows


def _large_cases():
    return [_flat("large", "Sort64", M), _flat("large", "Sort64", M, M - 3, key_value=True),
            _flat("large", "OrderedSort", M, key_value=True, order=FLOAT32_DESCENDING), _flat("large", "WideValueSort", M)]


def cases(setting):
    """The battery of a setting, in the order it runs."""
    assert setting in SETTINGS, setting
    rows = []
    if setting in SMALL_SETTINGS:
        rows += _small_cases()
    if setting in MID_SETTINGS:   # (16385 is the last of SMALL as well: the same call is listed once)
        rows += [case for case in _mid_cases() if name_of(case) not in {name_of(c) for c in rows}]
    if setting in LARGE_SETTINGS:
        rows += _large_cases()
    assert len(set(rows)) == len(rows)
    return rows


def plan_points(rows):
    """every distinct (n, kind, key+value, order word | bit range | None) whose plan the battery's calls are recorded from:
    the inner 32-bit sorts of the 64-bit forms are key+value sorts (keys-only: of the low words with the high words)"""
    points = []
    for case in rows:
        if case.group == "segmented":
            continue
        key_value = "KeyValue" in case.entry
        if "Sort64" in case.entry:
            point = (case.n, "sort", True, None)
        elif "WideValueSort" in case.entry:
            point = (case.n, "wide", True, None)
        elif "SortBits" in case.entry:
            point = (case.n, "sort" if case.bit_range == (0, 32) else "bits", key_value, case.bit_range)
        elif "RangeSort" in case.entry:
            point = (case.n, "range", key_value, case.bit_range)
        else:
            point = (case.n, "sort", key_value, key_order32_cases.order_word(*case.order[:2]))
        if point not in points:
            points.append(point)
    return points


# ---- inputs and references -------------------------------------------------------------------------------------------------

def _segments(case, rng):
    return segmented_cases.mixed_offsets(rng, SEGMENT_SIZES)


@functools.lru_cache(maxsize=8)
def inputs_of(case):
    """(keys, values, offsets) of a case, read-only: keys of n + TAIL elements (a segmented call: n), values for the key+value
    forms, offsets for the segmented ones"""
    rng = np.random.default_rng(seed_of(case))
    entry, n = case.entry, case.n
    total = n if case.group == "segmented" else n + TAIL
    values = offsets = None
    key_value = "KeyValue" in entry
    if case.group == "segmented":
        offsets, length = _segments(case, rng)
        assert length == n
    if "WideValueSort" in entry:
        keys = wide_value_cases.make_keys("three" if n % 2 else "uniform", total, rng)
        values = (wide_value_segmented_cases if offsets is not None else wide_value_cases).make_values(total, rng)
    elif "Segmented64" in entry:
        keys = segmented64_cases.make_keys64("word-boundary", total, rng)
    elif "Sort64Ordered" in entry:
        keys = key_order_cases.make_keys(case.order[2], total, rng, *case.order[:2])
    elif "Sort64" in entry:       # ties that only the values tell apart, long runs of one high word
        keys = sort64_model.make_keys64("uniform" if not key_value and n > ONE_WORKGROUP_MAX else "dup-high", total, rng)
    elif "OrderedSort" in entry:  # (key+value: seven keys of both signs, every element with many equals)
        builder = "duplicates" if key_value and case.group == "small" else case.order[2]
        keys = key_order32_cases.make_keys(builder, total, rng, *case.order[:2])
    elif "Bits" in entry or "RangeSort" in entry:
        keys = sort_bits_cases.make_keys("few" if key_value else "uniform", total, *case.bit_range, rng)
    else:
        keys = segmented_cases.make_keys("uniform", total, rng)
    if key_value and values is None:
        values = sort64_model.payload64(total)
    for a in (keys, values, offsets):
        if a is not None:
            a.setflags(write=False)
    return keys, values, offsets


def sorted_count(case):
    return case.n if case.count is None else min(case.count, case.n)


def expected_of(case):
    """(keys, values) of the WHOLE arrays after the call"""
    keys, values, offsets = inputs_of(case)
    entry, n = case.entry, sorted_count(case)
    if case.refused:
        return keys, values
    if "WideValueSortSegmented" in entry:
        return wide_value_segmented_cases.expected(keys, values, offsets, case.n)
    if "WideValueSort" in entry:
        return wide_value_cases.expected(keys, values, n)
    if "OrderedSortSegmented" in entry:
        return key_order32_cases.expected_segments(keys, values, offsets, case.n, *case.order[:2])
    if "SegmentedBits" in entry:
        return segmented_bits_cases.expected(keys, values, offsets, case.n, *case.bit_range)
    if "Segmented" in entry:
        return segmented_cases.expected(keys, values, offsets, case.n)
    if "Sort64" in entry:
        order = case.order[:2] if case.order is not None else ("uint64", False)
        return key_order_cases.expected(keys, values, *order, count=n)
    if "OrderedSort" in entry:
        return key_order32_cases.expected(keys, values, *case.order[:2], count=n)
    assert "SortBits" in entry or "RangeSort" in entry, entry
    return sort_bits_cases.reference(keys, values, *case.bit_range, n)
