"""tests/native/plan_check, the host planner (vulkan_radix_sort_amd/csrc/vrdx_plan.h) as a CPU program: built on first use,
and its `describe` mode as a table.  A plain module next to plan_model.py, imported the same way; no GPU, no torch."""
import collections
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")

# The last size of every plan on an MI355X (vrdx_plan.h: HybridCapacity, MsdBits), as (last n, name, bits, hybridCap, msdCap,
# launches); beyond the last row: the four passes, five launches.  plan_check finds the same sizes from the functions.
ATOMIC_TABLE = [(16_384, "one-workgroup", 0, 0, 0, 1), (524_288, "hybrid-8", 8, 4096, 0, 6), (1_048_576, "hybrid-8", 8, 8192, 0, 6),
                (2_097_152, "hybrid-8", 8, 16384, 0, 6), (8_144_384, "hybrid-8", 8, 32768, 0, 6), (18_149_376, "msd", 10, 0, 18432, 7),
                (36_649_984, "msd", 10, 0, 36864, 6), (67_108_864, "msd", 11, 0, 36864, 6)]
BALLOT_TABLE = [(16_384, "one-workgroup", 0, 0, 0, 1), (524_288, "hybrid-8", 8, 4096, 0, 6), (1_048_576, "hybrid-8", 8, 8192, 0, 6),
                (4_072_192, "hybrid-8", 8, 16384, 0, 6)]
FOUR_PASSES = ("four-passes", 0, 0, 0, 5)

Row = collections.namedtuple("Row", "name bits hybrid_cap msd_cap launches config")
# ... and under knobs: the plan of a sort by the bits [8, 16), the form of the wide-value sort, its oneWorkgroupMax, the form
# of the range sort by the bits [8, 16), form and launches of the range sort over [0, 32)
KnobRow = collections.namedtuple("KnobRow", Row._fields + ("bits_plan", "wide_form", "wide_one_workgroup_max", "range_form",
                                                            "range_whole_form", "range_whole_launches"))


@functools.lru_cache(maxsize=1)
def executable():
    subprocess.run(["make", "-C", NATIVE, "plan_check"], check=True, capture_output=True)
    return os.path.join(NATIVE, "plan_check")


def describe(compute_units, atomic_rank, sizes, knobs=None):
    """{(n, key_value): Row} of the plan the host records for each size, keys-only and key+value.  knobs: the planning knobs
    as the environment spells them ({"VRDX_SMALL_SORT": "0"}, tests/knob_cases.py SETTINGS; VRDX_RANK is not one: the ranking
    is `atomic_rank`); with them -- an empty dict included -- every row is a KnobRow."""
    sizes = sorted(set(int(n) for n in sizes))
    spelled = []
    if knobs is not None:   # (the default spelled out: what turns on the three fields of a KnobRow)
        spelled = [f"{name}={value}" for name, value in sorted(knobs.items()) if name != "VRDX_RANK"] or ["VRDX_SMALL_SORT=1"]
    out = subprocess.run([executable(), "describe", str(compute_units), "1" if atomic_rank else "0"] + spelled
                         + [str(n) for n in sizes], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        n, key_value, name, bits, hybrid_cap, msd_cap, launches, config, *more = line.split()
        row = Row(name, int(bits), int(hybrid_cap), int(msd_cap), int(launches), config)
        if knobs is not None:
            row = KnobRow(*row, more[0], more[1], int(more[2]), more[3], more[4], int(more[5]))
        table[int(n), key_value == "1"] = row
    assert len(table) == 2 * len(sizes)
    return table


def table_row(table, n):
    """(name, bits, hybridCap, msdCap, launches) a table of edges states for n elements"""
    for last, *row in table:
        if n <= last:
            return tuple(row)
    return FOUR_PASSES


def edge_sizes(table):
    """either side of every edge: the last size of each plan and the first of the next"""
    return [last + d for last, *_ in table for d in (-1, 0, 1, 2)]
