"""Without a GPU: the host planner itself (vulkan_radix_sort_amd/csrc/vrdx_plan.h, through tests/native/plan_check) at every
size, and the numbers the tests keep by hand held to it -- MSD_FROM, MSD_HALF_UP_TO, TEN_BITS_UP_TO, msd_capacity(),
plan_model.hybrid_capacity(), the ballot sorter's capacity rule, and the plan every planted size is said to select."""
import subprocess

import pytest

import hybrid_bucket_cases
import msd_bucket_cases
import plan_check_tool as tool
import plan_model as model
import storage_reuse_cases
import test_bucket_output_policy_gpu as output_policy
import test_plan_choice_gpu as plan_choice
import test_sort_alignment_gpu as alignment
from test_sort_gpu import MSD_FROM, MSD_HALF_UP_TO, ROUND, msd_capacity

MI355X_CUS = 256
FIRST_MSD = 8_144_385   # one past the eight-bit plan's last size


def test_planner_invariants_and_edges_at_every_size():
    """plan_check's default mode: the step list, slots, launch counts, geometry and grid of every plan over the sweep of
    sizes, CU counts, value and ranking modes and forced geometries; the refused layout; the edges found from the rules."""
    r = subprocess.run([tool.executable()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _params(test, argnames):
    """the values one @pytest.mark.parametrize of a test function gives `argnames`"""
    for mark in test.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == argnames:
            return list(mark.args[1])
    raise KeyError(argnames)


# (n, name, bits, msdCap or None where the test does not state it) as each test's own comments and asserts claim
PLANTED_ATOMIC = (
    [(plan_choice.HALF, "msd", 10, 18432), (plan_choice.FULL10, "msd", 10, 36864), (plan_choice.ELEVEN, "msd", 11, 36864),
     (plan_choice.LAST, "msd", 11, 36864), (plan_choice.LAST + 1, "four-passes", 0, 0)]
    + [(n, plan, None, None) for n, plan, _ in plan_choice.PLAN_TABLE]
    + [(n, "msd", None, None) for n, _ in _params(plan_choice.test_sample_rule_at_cap_times_two_to_the_spread, "n,v")]
    + [(n, "msd", None, None) for n in _params(plan_choice.test_tiny_counts_under_a_large_bound, "bound")]
    + [(n, "hybrid-8", 8, 0) for n in _params(plan_choice.test_hybrid_plan_by_every_byte_at_the_bucket_capacity, "n")]
    + [(storage_reuse_cases.M, "msd", storage_reuse_cases.MSD_BITS, 18432), (storage_reuse_cases.H, "hybrid-8", 8, 0),
       (storage_reuse_cases.TAIL_SPLIT_N, "msd", storage_reuse_cases.MSD_BITS, 18432),
       (storage_reuse_cases.BLOCK_SUMS_N, "msd", storage_reuse_cases.MSD_BITS, 18432), (ROUND, "msd", 10, 18432)]
    + [(f.bound, "msd", f.bits, f.cap) for f in msd_bucket_cases.FORMS.values()]
    + [(n, "hybrid-8", 8, 0) for f in hybrid_bucket_cases.FORMS.values() for n in (f.bound, f.filled) if n is not None]
    + [(n, "one-workgroup", 0, 0) for n in alignment.ONE_WORKGROUP_SIZES]
    + [(n, "hybrid-8", 8, 0) for n, _ in alignment.HYBRID_ROWS]
    + [(n, "msd", 10, 18432) for n, _, _ in _params(alignment.test_msd_plan_with_half_size_buckets, "n,a_keys,a_values")]
    + [(n, "msd", 10, 36864) for n in _params(alignment.test_msd_plan_with_full_size_buckets, "n")]
    + [(n, "msd", 10, 36864) for n in _params(alignment.test_non_temporal_bucket_output, "n")]
    + [(36_649_987, "msd", 11, 36864), (alignment.LAST + 1, "four-passes", 0, 0)]   # test_eleven_bit_window, test_four_passes_past_...
    + [(n, "msd", 10, 18432) for n, _ in _params(alignment.test_window_and_verdict_under_misalignment, "n,a")]
    + [(bound, "one-workgroup" if bound <= 16384 else "msd", None, None)
       for bound, _ in _params(alignment.test_count_word_at_every_residue, "bound,count")]
    + [(n, "msd", 10 if n <= output_policy.TEN_BITS_UP_TO else 11, 18432 if n <= MSD_HALF_UP_TO else 36864)
       for n in output_policy.SIZES])


def test_planted_sizes_select_the_plan_their_tests_claim():
    got = tool.describe(MI355X_CUS, True, [n for n, *_ in PLANTED_ATOMIC])
    for n, name, bits, msd_cap in PLANTED_ATOMIC:
        for key_value in (False, True):
            row = got[n, key_value]
            assert row.name == name, (n, key_value, row)
            assert bits is None or row.bits == bits, (n, key_value, row)
            assert msd_cap is None or row.msd_cap == msd_cap, (n, key_value, row)
            # the hand-kept formulas, wherever they apply
            if row.name == "msd":
                assert msd_capacity(n, row.bits) == row.msd_cap, (n, key_value, row)
                assert row.launches == (7 if n <= MSD_HALF_UP_TO else 6) and n >= FIRST_MSD, (n, row)
            assert model.hybrid_capacity(n) == row.hybrid_cap or row.name == "one-workgroup", (n, key_value, row)
            assert (row.name == "hybrid-8") == (row.hybrid_cap != 0)


def test_the_calls_of_the_storage_reuse_table_record_their_plan():
    """storage_reuse_cases.CALLS: the plan column, for the sorter the call names; the ballot sorter's capacity rule"""
    calls = [c for c in storage_reuse_cases.CALLS if c.plan is not None]
    for atomic in (True, False):
        mine = [c for c in calls if (c.sorter == "atomic") == atomic]
        got = tool.describe(MI355X_CUS, atomic, [c.bound for c in mine] + [4_000_000, 4_200_000])
        for c in mine:
            for key_value in (False, True):   # (the same plan either way at these sizes, as the table assumes)
                row = got[c.bound, key_value]
                assert row.name == c.plan, (c.name, key_value, row)
                cap = model.hybrid_capacity(c.bound) if atomic else storage_reuse_cases.ballot_hybrid_capacity(c.bound)
                assert row.hybrid_cap == (cap if c.plan == "hybrid-8" else 0), (c.name, row)
        if not atomic:
            for n in (4_000_000, 4_200_000):
                assert got[n, False].hybrid_cap == got[n, True].hybrid_cap == storage_reuse_cases.ballot_hybrid_capacity(n)


def test_alignment_sizes_under_the_ballot_ranking():
    """test_ballot_ranking_one_workgroup_at_every_residue, test_ballot_ranking_hybrid_plan_at_every_residue"""
    got = tool.describe(MI355X_CUS, False, alignment.ONE_WORKGROUP_SIZES + [n for n, _ in alignment.HYBRID_ROWS])
    for key_value in (False, True):
        assert all(got[n, key_value].name == "one-workgroup" for n in alignment.ONE_WORKGROUP_SIZES)
        assert all(got[n, key_value][:2] == ("hybrid-8", 8) for n, _ in alignment.HYBRID_ROWS)


@pytest.mark.parametrize("atomic", [True, False])
def test_every_edge_of_the_plan_table(atomic):
    """either side of every size at which the plan changes: name, bits, capacities and launches are the table's, keys-only and
    key+value, and the tests' formulas give the planner's capacities"""
    table = tool.ATOMIC_TABLE if atomic else tool.BALLOT_TABLE
    sizes = tool.edge_sizes(table) + ([] if atomic else tool.edge_sizes(tool.ATOMIC_TABLE))
    got = tool.describe(MI355X_CUS, atomic, sizes)
    for n in sizes:
        for key_value in (False, True):
            row = got[n, key_value]
            assert tuple(row[:5]) == tool.table_row(table, n), (n, key_value, row)
            want_cap = model.hybrid_capacity(n) if atomic else storage_reuse_cases.ballot_hybrid_capacity(n)
            assert row.hybrid_cap == (want_cap if n > 16_384 else 0), (n, row)
            if row.name == "msd":
                assert msd_capacity(n, row.bits) == row.msd_cap, (n, row)
            assert (row.config == "-") == (row.name == "one-workgroup"), (n, row)
            if row.name == "msd":
                assert row.config == ("1024x32" if key_value else "1024x32x2"), (n, row)


def test_the_bounds_the_tests_keep_by_hand():
    """MSD_HALF_UP_TO and TEN_BITS_UP_TO are exactly the last sizes of their ranges; MSD_FROM lies inside the MSD plan's range
    with nothing but the MSD plan between the plan's first size and it."""
    ten = output_policy.TEN_BITS_UP_TO
    sizes = list(range(FIRST_MSD - 1, MSD_FROM + 1)) + [MSD_HALF_UP_TO, MSD_HALF_UP_TO + 1, ten, ten + 1]
    got = tool.describe(MI355X_CUS, True, sizes)
    for key_value in (False, True):
        assert got[MSD_HALF_UP_TO, key_value][:4] == ("msd", 10, 0, 18432)
        assert got[MSD_HALF_UP_TO + 1, key_value][:4] == ("msd", 10, 0, 36864)
        assert got[ten, key_value][:4] == ("msd", 10, 0, 36864)
        assert got[ten + 1, key_value][:4] == ("msd", 11, 0, 36864)
        assert got[FIRST_MSD - 1, key_value].name == "hybrid-8"
        assert all(got[n, key_value][:4] == ("msd", 10, 0, 18432) for n in range(FIRST_MSD, MSD_FROM + 1))
    assert (MSD_HALF_UP_TO, ten) == (tool.ATOMIC_TABLE[5][0], tool.ATOMIC_TABLE[6][0])
    assert FIRST_MSD == tool.ATOMIC_TABLE[4][0] + 1 <= MSD_FROM <= MSD_HALF_UP_TO
