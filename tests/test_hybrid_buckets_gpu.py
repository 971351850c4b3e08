"""The hybrid plan's kernels bucket by bucket: launch 0 in its scatter role (ReadPassPlan with plan.digit = t) under every
tile geometry the planner picks at a hybrid size, and bucket_sort_kernel<1024, 4 | 8 | 16 | 32> (SortInWorkgroup with
bytes = t, at a base that is an arbitrary word offset), keys-only and key+value, one-atomic and ballot ranking, on buckets
whose sizes and contents tests/hybrid_bucket_cases.py chooses -- every edge of the chunk dealing and of the capacity, keys
that share the pad's digit in one pass or in all, slots that are uniform, 63 + 1, two-valued or on either side of the two
thresholds of 48 lanes, in pass 0 and in the passes behind it, t = 3, 2, 1 and 0.

The plan, the grids and the kernel forms depend on the bound of an indirect sort only; the count, the byte t, the verdict and
the buckets are read on the device.  So nearly every call here is vrdxCmdSort[KeyValue]Indirect with the bound of a kernel
form (0.5 M ... 8.1 M) and a device count of at most 262 K keys, compared bit for bit with numpy's stable sort; one direct
sort per form fills every bucket.  tests/test_hybrid_bucket_cases.py checks without a GPU that the plan takes each case by the
byte it is built for and that the cases catch seven faults planted in a numpy model of the kernel.

Per form and mode the caller arrays (bound + 256 words of a guard word), the storage (poisoned once, then reused as the call
before left it) and the count words are allocated once.  After every call: keys and values of [0, count) equal the reference,
everything from `count` on still holds the guard (compared on the device), the count words are untouched, the storage's guard
band is intact, the status is 0, word 1 of the storage and vrdxHipReadPlanVerdict are the case's verdict, and the sorter's
plan counters (MSD sorts only) have not moved.
"""
import numpy as np
import pytest

import hybrid_bucket_cases as cases
import plan_model as model
from guarded_call import ballot_sorter, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

GUARD = cases.GUARD
MODES = [(name, key_value) for name in cases.FORMS for key_value in (False, True)]
BALLOT_MODES = [(name, key_value) for name, key_value in MODES if cases.FORMS[name].ballot]
FILLED_MODES = [(name, key_value) for name, key_value in MODES if cases.FORMS[name].filled is not None]


class Rig:
    """A sorter, its plan counters as they must stand, and the buffers of ONE form and mode at a time."""

    def __init__(self, torch, sorter, owned):
        self.torch = torch
        self.sorter = sorter
        self.owned = owned
        self.stream = torch.cuda.current_stream().cuda_stream
        self.counters = self.sorter.read_plan_counters(self.stream)
        self.key = None
        self.keys = self.values = self.storage = self.count = None

    def release(self):
        self.keys = self.values = self.storage = self.count = None
        self.key = None

    def arena(self, form, key_value):
        """buffers of (form, key_value): allocated when the tests move on to another form or mode, reused until then"""
        torch = self.torch
        if self.key == (form.name, key_value):
            return
        self.release()   # (the form before: released first)
        sizes = [form.bound] + ([form.filled] if form.filled is not None else [])
        s = self.sorter
        for n in sizes:   # what the host records is the plan the cases are built for
            for kv in (False, True):
                info = s.describe_plan(n, kv)
                assert (info.name, int(info.bits), int(info.launches)) == ("hybrid-8", 8, 6), (form.name, n, kv)
            assert model.hybrid_capacity(n) == form.cap
        words = max(sizes) + 256
        self.keys = torch.full((words,), GUARD, dtype=torch.int32, device="cuda")
        self.values = torch.full((words,), GUARD, dtype=torch.int32, device="cuda") if key_value else None
        self.required = max(int((s.key_value_storage_requirements(n) if key_value else s.storage_requirements(n)).size)
                            for n in sizes)
        self.storage = torch.full((self.required + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.storage[self.required:] = 0x5A
        self.count = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
        self.count_word = GUARD
        self.dirty = 0
        self.key = (form.name, key_value)
        self.form, self.key_value = form, key_value

    def record(self, stream, direct=None):
        s, f = self.sorter, self.form
        keys, values, storage = self.keys.data_ptr(), self.values.data_ptr() if self.key_value else None, self.storage.data_ptr()
        if direct is not None:
            if self.key_value:
                s.cmd_sort_key_value(stream, direct, keys, 0, values, 0, storage, 0)
            else:
                s.cmd_sort(stream, direct, keys, 0, storage, 0)
        elif self.key_value:
            s.cmd_sort_key_value_indirect(stream, f.bound, self.count.data_ptr(), 0, keys, 0, values, 0, storage, 0, None, 0)
        else:
            s.cmd_sort_indirect(stream, f.bound, self.count.data_ptr(), 0, keys, 0, storage, 0, None, 0)

    def upload(self, keys, values, direct=None):
        """guards the front the call before used, then the first `count` keys (values) and, for an indirect call, the count"""
        torch = self.torch
        n = len(keys)
        for dst, src in ((self.keys, keys), (self.values, values if self.key_value else None)):
            if dst is not None:
                dst[:self.dirty].fill_(GUARD)
                dst[:n].copy_(torch.from_numpy(np.array(src, dtype=np.uint32).view(np.int32)))
        if direct is None:
            self.count[0] = n
            self.count_word = n
        self.dirty = n
        torch.cuda.synchronize()

    def check(self, case, keys, values):
        """everything a finished call must have left behind"""
        n, what = len(keys), (case.name, self.key_value)
        want_keys, want_values = cases.reference(keys, values)
        got = self.keys[:n].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want_keys), (what, "keys", int((got != want_keys).sum()))
        assert bool((self.keys[n:] == GUARD).all()), (what, "keys behind the count")
        if self.key_value:
            got = self.values[:n].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want_values), (what, "values", int((got != want_values).sum()))
            assert bool((self.values[n:] == GUARD).all()), (what, "values behind the count")
        assert self.count.cpu().numpy().view(np.uint32).tolist() == [self.count_word, GUARD, GUARD, GUARD], what
        assert bool((self.storage[self.required:] == 0x5A).all()), (what, "wrote past the storage requirement")
        assert self.sorter.read_status(self.stream, self.storage.data_ptr(), 0) == 0, what
        word = int(self.storage[4:8].cpu().numpy().view(np.uint32)[0])
        assert word == case.verdict, (what, hex(word), case.verdict)
        assert self.sorter.read_plan_verdict(self.stream, self.storage.data_ptr(), 0) == case.verdict, what
        assert self.sorter.read_plan_counters(self.stream) == self.counters, what

    def inputs(self, case):
        keys = cases.case_keys(case)
        return keys, cases.payload(len(keys))

    def run(self, case):
        """one recorded call, one synchronise, every check"""
        assert case.form is self.form
        keys, values = self.inputs(case)
        self.upload(keys, values, case.direct)
        self.record(self.stream, case.direct)
        self.torch.cuda.synchronize()
        self.check(case, keys, values)


@pytest.fixture(scope="module")
def rig(torch_mod):
    import vulkan_radix_sort_amd as vrdx
    b = Rig(torch_mod, vrdx.Sorter(), True)
    yield b
    b.release()
    b.sorter.destroy()


@pytest.fixture(scope="module")
def ballot_rig(torch_mod, ballot_sorter):
    b = Rig(torch_mod, ballot_sorter, False)
    yield b
    b.release()


def _setup(rig, form_name, key_value):
    form = cases.FORMS[form_name]
    rig.arena(form, key_value)
    return form


@pytest.mark.parametrize("t", cases.LADDER_TS)
@pytest.mark.parametrize("form_name,key_value", MODES)
def test_ladder_at_every_byte_and_turn(rig, form_name, key_value, t):
    """every bucket size of the ladder in one call, scattered by byte t and sorted by the t bytes below; the contents rotate
    with the turn: over the turns every bucket holds every content"""
    form = _setup(rig, form_name, key_value)
    for turn in range(len(cases.ROTATION)):
        rig.run(cases.ladder_case(form, key_value, t, turn))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_ladder_grouped(rig, form_name, key_value):
    """bucket after bucket: whole scatter tiles of one digit, every slot of launch 0 uniform"""
    form = _setup(rig, form_name, key_value)
    for t, turn in cases.GROUPED:
        rig.run(cases.ladder_case(form, key_value, t, turn, order="grouped"))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_top_bucket_with_real_sentinels(rig, form_name, key_value):
    """t = 3, real 0xFFFFFFFF keys -- the pad itself, with values that are not the pad's -- in a ragged, a nearly full and a
    full bucket 255; zeros in bucket 0"""
    form = _setup(rig, form_name, key_value)
    for size in cases.top_sizes(form):
        rig.run(cases.top_case(form, size))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_two_buckets_only(rig, form_name, key_value):
    """only two of the 256 digits occur: a full bucket and one key, then two full buckets; launch 0 ranks a two-valued byte"""
    form = _setup(rig, form_name, key_value)
    for t in cases.LADDER_TS:
        for second in (1, form.cap):
            rig.run(cases.two_bucket_case(form, t, second))


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_one_key_beyond_the_capacity_runs_the_four_passes(rig, form_name, key_value):
    """a designed decline: verdict 2, the bucket launch returns, the four passes sort, the status stays 0"""
    form = _setup(rig, form_name, key_value)
    for t in cases.OVERFLOW_TS:
        case = cases.overflow_case(form, t)
        assert case.verdict == model.VERDICT_HYBRID_DECLINED
        rig.run(case)


@pytest.mark.parametrize("t", cases.FILLED_TS)
@pytest.mark.parametrize("form_name,key_value", FILLED_MODES)
def test_filled_direct_sort(rig, form_name, key_value, t):
    """vrdxCmdSort[KeyValue] at a size of the form's bucket kernel: the ladder's buckets, every other digit filled evenly"""
    form = _setup(rig, form_name, key_value)
    rig.run(cases.filled_case(form, key_value, t))


@pytest.mark.parametrize("form_name,key_value", BALLOT_MODES)
def test_ballot_ranking_ladder(ballot_rig, form_name, key_value):
    """the RankBallot forms of the same kernels (capacities up to 16384)"""
    form = _setup(ballot_rig, form_name, key_value)
    for case in cases.ballot_cases(form, key_value):
        ballot_rig.run(case)
