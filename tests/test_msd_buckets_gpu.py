"""The MSD plan's bucket kernels bucket by bucket: bucket_sort2_half_kernel and the bucket role of
msd_buckets_or_pass1_kernel (ten and eleven bits, keys-only and key+value, plain and non-temporal output) on buckets whose
sizes and contents tests/msd_bucket_cases.py chooses -- every edge of the chunk dealing and of the capacity, keys that share
the pad's digit, slots that are uniform, nearly uniform or on either side of the probe's threshold, the two buckets of one
workgroup, every split of the two passes.

The plan, the grids and the kernel forms depend on the bound of an indirect sort only; the count, the window and the buckets
are read on the device.  So every call here is vrdxCmdSort[KeyValue]Indirect with the bound of a kernel form (8.6 M ... 37 M)
and a device count of at most 176 K keys, compared bit for bit with numpy's stable sort.  tests/test_msd_bucket_cases.py
checks without a GPU that the plan takes each case with the window it is built for and that the cases catch five faults
planted in a numpy model of the kernel.

Per form and mode the caller arrays (bound + 256 words of a guard word), the storage (poisoned once, then reused as the call
before left it) and the count word are allocated once.  After every call: keys and values of [0, count) equal the reference,
everything from `count` on still holds the guard (compared on the device), the storage's guard band is intact, the status is
0, word 1 of the storage is the verdict | shift << 8, and the sorter's plan counters moved by exactly this call.
"""
import numpy as np
import pytest

import msd_bucket_cases as cases
import plan_model as model
from test_sort_gpu import msd_capacity

pytestmark = pytest.mark.gpu

GUARD = cases.GUARD
MODES = [(name, key_value) for name in cases.FORMS for key_value in (False, True)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


class Rig:
    """The sorter, its plan counters as they must stand, and the buffers of ONE form and mode at a time."""

    def __init__(self, torch):
        import vulkan_radix_sort_amd as vrdx
        self.torch = torch
        self.sorter = vrdx.Sorter()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.recorded, self.declined = self.sorter.read_plan_counters(self.stream)
        self.key = None

    def arena(self, form, key_value):
        """buffers of (form, key_value): allocated when the tests move on to another form or mode, reused until then"""
        torch = self.torch
        if self.key == (form.name, key_value):
            return
        self.keys = self.values = self.storage = self.count = None   # (the form before: released first)
        for kv in (False, True):   # what the host records for the bound is the kernel form the cases are built for
            info = self.sorter.describe_plan(form.bound, kv)
            assert (info.name, int(info.bits), int(info.launches)) == ("msd", form.bits, form.launches), (form.name, kv)
        assert msd_capacity(form.bound, form.bits) == form.cap
        words = form.bound + 256
        self.keys = torch.full((words,), GUARD, dtype=torch.int32, device="cuda")
        self.values = torch.full((words,), GUARD, dtype=torch.int32, device="cuda") if key_value else None
        s = self.sorter
        self.required = int((s.key_value_storage_requirements(form.bound) if key_value
                             else s.storage_requirements(form.bound)).size)
        self.storage = torch.full((self.required + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.storage[self.required:] = 0x5A
        self.count = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
        self.dirty = 0
        self.key = (form.name, key_value)
        self.form, self.key_value = form, key_value

    def record(self, stream):
        s, f = self.sorter, self.form
        if self.key_value:
            s.cmd_sort_key_value_indirect(stream, f.bound, self.count.data_ptr(), 0, self.keys.data_ptr(), 0,
                                          self.values.data_ptr(), 0, self.storage.data_ptr(), 0, None, 0)
        else:
            s.cmd_sort_indirect(stream, f.bound, self.count.data_ptr(), 0, self.keys.data_ptr(), 0,
                                self.storage.data_ptr(), 0, None, 0)
        self.recorded += 1

    def upload(self, keys, values):
        """guards the front the call before used, then the first `count` keys (values) and the count word"""
        torch = self.torch
        n = len(keys)
        for dst, src in ((self.keys, keys), (self.values, values if self.key_value else None)):
            if dst is not None:
                dst[:self.dirty].fill_(GUARD)
                dst[:n].copy_(torch.from_numpy(src.view(np.int32)))
        self.count[0] = n
        self.dirty = n
        torch.cuda.synchronize()

    def check(self, case, keys, values):
        """everything a finished call must have left behind"""
        torch, n, what = self.torch, len(keys), (case.name, self.key_value)
        want_keys, want_values = cases.reference(keys, values)
        got = self.keys[:n].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want_keys), (what, "keys", int((got != want_keys).sum()))
        assert bool((self.keys[n:] == GUARD).all()), (what, "keys behind the count")
        if self.key_value:
            got = self.values[:n].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want_values), (what, "values", int((got != want_values).sum()))
            assert bool((self.values[n:] == GUARD).all()), (what, "values behind the count")
        assert self.count.cpu().numpy().view(np.uint32).tolist() == [n, GUARD, GUARD, GUARD], what
        assert bool((self.storage[self.required:] == 0x5A).all()), (what, "wrote past the storage requirement")
        assert self.sorter.read_status(self.stream, self.storage.data_ptr(), 0) == 0, what
        word = int(self.storage[4:8].cpu().numpy().view(np.uint32)[0])
        expected = case.verdict | ((case.shift << 8) if case.verdict == model.VERDICT_MSD_RUNS else 0)
        assert word == expected, (what, hex(word), hex(expected))
        if case.verdict == model.VERDICT_NONE:
            self.declined += 1
        assert self.sorter.read_plan_counters(self.stream) == (self.recorded, self.declined), what

    def inputs(self, case):
        keys = cases.case_keys(case)
        return keys, cases.payload(len(keys))

    def run(self, case):
        """one recorded call, one synchronise, every check"""
        keys, values = self.inputs(case)
        self.upload(keys, values)
        self.record(self.stream)
        self.torch.cuda.synchronize()
        self.check(case, keys, values)


@pytest.fixture(scope="module")
def rig(torch_mod):
    b = Rig(torch_mod)
    yield b
    b.keys = b.values = b.storage = b.count = None
    b.sorter.destroy()


def _setup(rig, form_name, key_value):
    form = cases.FORMS[form_name]
    rig.arena(form, key_value)
    return form


LADDER = [(name, key_value, shift) for name, key_value in MODES for shift in cases.shifts_of(cases.FORMS[name])]


@pytest.mark.parametrize("form_name,key_value,shift", LADDER)
def test_ladder_at_every_below(rig, form_name, key_value, shift):
    """every bucket size of the ladder in one call, the contents rotating with the shift, under every split of the passes"""
    form = _setup(rig, form_name, key_value)
    rig.run(cases.ladder_case(form, key_value, shift))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_ladder_with_whole_scatter_tiles_of_one_bucket(rig, form_name, key_value):
    form = _setup(rig, form_name, key_value)
    for shift in cases.grouped_shifts(form):
        rig.run(cases.ladder_case(form, key_value, shift, order="grouped"))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_top_window_with_real_sentinels_in_the_top_bucket(rig, form_name, key_value):
    """real 0xFFFFFFFF keys -- the pad itself -- in a ragged, a nearly full and a full top bucket; zeros in bucket 0"""
    form = _setup(rig, form_name, key_value)
    for size in cases.top_sizes(form):
        rig.run(cases.top_case(form, size))


@pytest.mark.parametrize("form_name,key_value", [m for m in MODES if cases.FORMS[m[0]].waves == 16])
def test_the_two_buckets_of_one_workgroup(rig, form_name, key_value):
    """full then one key, one key then full, empty then ragged, ragged then empty, full then full"""
    form = _setup(rig, form_name, key_value)
    for shift in cases.pair_shifts(form):
        rig.run(cases.pair_case(form, shift))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_one_key_beyond_the_capacity_is_turned_down(rig, form_name, key_value):
    form = _setup(rig, form_name, key_value)
    case = cases.overflow_case(form)
    assert case.verdict == model.VERDICT_NONE
    rig.run(case)
