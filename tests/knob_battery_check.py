"""The battery of tests/knob_cases.py under ONE setting of the planning knobs, in a process of its own: the knobs are read once
per process (vrdx_api.cpp, EnvKnobs), so tests/test_knobs_gpu.py starts this script once per setting with the setting's
environment.  argv[1] is the setting's name.

First the plans: for every (n, mode) of the setting's cases, what describe_plan, describe_ordered_sort_plan,
describe_sort_bits_plan, describe_range_sort_plan and describe_wide_value_sort_plan report against knob_cases.expected_plan -- a
mismatch is a failure, and a child whose environment did not arrive fails here.  Then every case through guarded_call /
range_call / ordered_call / wide_call / wide_segmented_call on poisoned storage: guard bytes, failure word, the sorter's sticky word, and the arrays bit for bit
against the case's reference.  No case is skipped; a refusal is a failure except where the case is marked refused.

One line per plan point and per case; the last line is "<cases> cases, <failures> failures".  Exit status 0 only with 0
failures.  Anything but a failed check -- an error of the HIP runtime above all -- ends the run at once with status 2: nothing
more is started on a device that has faulted.  tests/test_knob_cases.py runs run_case and check_plans against a sorter on
host memory."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

import knob_cases
from guarded_call import guarded_call
from ordered_guarded_call import ordered_call
from range_guarded_call import AsRangeSort
from vulkan_radix_sort_amd import api
from wide_guarded_call import wide_call
from wide_segmented_guarded_call import wide_segmented_call


def check_plans(sorter, setting, rows):
    """[(what, got, want)] of every plan point of `rows` under `setting`, on this sorter"""
    out = []
    for n, kind, key_value, extra in knob_cases.plan_points(rows):
        want = knob_cases.expected_plan(setting, n, key_value, kind)
        if kind == "wide":
            info = sorter.describe_wide_value_sort_plan(n)
            got, want = (info.name, int(info.oneWorkgroupMax)), (want, knob_cases.expected_wide_one_workgroup_max(setting))
            what = f"wide-value plan n={n}"
        elif kind == "range":   # part of the key: the form alone; the whole key: PlanSort's launches under this setting
            info = sorter.describe_range_sort_plan(n, key_value, *extra)
            want = knob_cases.expected_plan(setting, n, key_value, kind, bit_range=extra)
            got, what = info.name, "range-sort plan n=%d bits=[%d,%d)" % (n, *extra)
            if want == "whole-key":
                got, want = (got, int(info.launches)), (want, knob_cases.expected_launches(setting, n, key_value))
        elif isinstance(extra, tuple):
            got, what = sorter.describe_sort_bits_plan(n, key_value, *extra).name, "sort-bits plan n=%d bits=[%d,%d)" % (n, *extra)
        elif extra is not None:
            got, what = sorter.describe_ordered_sort_plan(n, key_value, extra).name, f"ordered plan n={n} order={extra:#x}"
        else:
            got, what = sorter.describe_plan(n, key_value).name, f"plan n={n}"
        out.append((f"{what} key+value={int(key_value)}", got, want))
    return out


def run_case(torch, sorter, case, device="cuda"):
    """One case through the guarded call of its table; raises AssertionError with what went wrong."""
    keys, values, offsets = knob_cases.inputs_of(case)
    want_keys, want_values = knob_cases.expected_of(case)
    stream = torch.cuda.current_stream().cuda_stream if torch.device(device).type == "cuda" else 0
    common = dict(count=case.n, device=device)
    try:
        if "WideValueSortSegmented" in case.entry:
            got = wide_segmented_call(torch, sorter, keys, values, offsets, **common)
        elif "WideValueSort" in case.entry:
            got = wide_call(torch, sorter, keys, values, device_count=case.count, **common)
        elif "OrderedSort" in case.entry:
            got = ordered_call(torch, sorter, keys, values, order=knob_cases.key_order32_cases.order_word(*case.order[:2]),
                               offsets=offsets, device_count=case.count, **common)
        else:
            order = knob_cases.key_order_cases.order_word(*case.order[:2]) if case.order is not None else None
            ranged = "RangeSort" in case.entry   # (the arguments of vrdxHipCmdSortBits*, name for name: range_guarded_call.py)
            got = guarded_call(torch, AsRangeSort(sorter) if ranged else sorter, keys, values, offsets=offsets,
                               device_count=case.count,
                               bit_range=case.bit_range, order=order, expect_refused=case.refused, **common)
    except AssertionError as e:
        # the sorter's word is read whatever happened, so that it is this case's alone; a refused call leaves the poisoned
        # storage as it is, which the helpers report as a failure word
        sticky = sorter.read_sorter_status(stream)
        if sticky & api.STATUS_ENQUEUE_REFUSED and not case.refused:
            raise AssertionError(f"the call was refused ({e})") from None
        raise
    sticky = sorter.read_sorter_status(stream)   # (a refusal that guarded_call expected was read, and cleared, by it)
    assert not sticky & api.STATUS_ENQUEUE_REFUSED, "the call was refused"
    assert sticky == 0, f"the sorter's sticky word is {sticky:#x}"
    for what, have, want in (("keys", got.keys, want_keys), ("values", got.values, want_values)):
        if want is None:
            assert have is None
            continue
        bad = np.flatnonzero(have != want)
        n = knob_cases.sorted_count(case)
        assert bad.size == 0, (f"{what}: {bad.size} elements differ, the first at {bad[:4].tolist()} of {n} sorted "
                               f"({have[bad[:2]].tolist()}, not {want[bad[:2]].tolist()})")


def run_battery(torch, sorter, setting, rows, device="cuda", out=print):
    """the plan lines, one line per case and the verdict line; returns the number of failures"""
    failures = 0
    for what, got, want in check_plans(sorter, setting, rows):
        ok = got == want
        failures += not ok
        out(f"{'ok  ' if ok else 'FAIL'} {what}: {got}" + ("" if ok else f", expected {want}"))
    for case in rows:
        try:
            run_case(torch, sorter, case, device)
            out(f"ok   {knob_cases.name_of(case)}")
        except AssertionError as e:
            failures += 1
            out(f"FAIL {knob_cases.name_of(case)}: {e}")
    out(f"{len(rows)} cases, {failures} failures")
    return failures


def main(setting):
    import torch
    import vulkan_radix_sort_amd as vrdx
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)   # (VRDX_RANK=ballot in the environment: the ballot ranking)
    try:
        failures = run_battery(torch, sorter, setting, knob_cases.cases(setting))
    except Exception as e:    # not a failed check: say so and start nothing more
        print(f"aborted: {type(e).__name__}: {e}", flush=True)
        return 2
    sorter.destroy()
    return 0 if failures == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
