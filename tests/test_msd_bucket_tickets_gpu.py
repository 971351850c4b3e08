"""The bucket launches of the MSD plan hand their buckets out by a ticket (BucketSort2Body in vrdx_kernels.hip): the workgroups
that are resident draw bucket after bucket until 2^bits are taken, every other workgroup returns on its first draw.  What that
can get wrong, on every kernel form (half-size, ten bits, ten bits with streamed output, eleven bits), keys-only and key+value
with values that are no indices:

  * a bucket nobody draws (an unsorted range) or one drawn twice (a race): EVERY bucket holds one to three keys;
  * a long bucket first or last in the drawing order, among buckets that are empty or hold a single key: the other
    workgroups run out of tickets while one still sorts;
  * a ticket word that does not start at 0: two sorts through one storage, and a sort behind one that the device turned
    down -- its four passes have drawn their tiles from the same word;
  * counts of 0 and 1.

Like tests/test_msd_buckets_gpu.py, whose rig this uses: every call is an indirect sort with the bound of a kernel form and a
small device count, compared bit for bit with numpy's stable sort; behind the count the guard words are intact, the status is
0, word 1 of the storage is the verdict | shift << 8 and the plan counters move by one recorded call (and one declined plan
where the model says so).  The expectations do not depend on how the buckets are handed out: they hold for a strided loop as
well.  tests/test_bucket_ticket_draw.py pins the draw itself without a GPU.
"""
import numpy as np
import pytest

import msd_bucket_cases as cases
import plan_model as model
import test_msd_buckets_gpu as base

pytestmark = pytest.mark.gpu

MODES = base.MODES


@pytest.fixture(scope="module")
def rig():
    import torch
    b = base.Rig(torch)
    yield b
    b.keys = b.values = b.storage = b.count = None
    b.sorter.destroy()


def tiny_keys(form, shift, seed):
    """one to three keys in every one of the 2^bits buckets, in random order; a key of bucket 0 first and one of the top bucket
    last, so that the sample sees the window's top bit vary"""
    rng = np.random.default_rng(seed)
    nb = 1 << form.bits
    sizes = 1 + (np.arange(nb) + seed) % 3
    digit = np.repeat(np.arange(nb, dtype=np.uint32), sizes)
    digit = digit[rng.permutation(len(digit))]
    first = int(np.flatnonzero(digit == 0)[0])
    digit[[0, first]] = digit[[first, 0]]
    last = int(np.flatnonzero(digit == nb - 1)[-1])
    digit[[-1, last]] = digit[[last, -1]]
    low = rng.integers(0, 1 << shift, size=len(digit), dtype=np.uint64).astype(np.uint32)
    high = np.uint32(model.prefix_of(shift + form.bits) if shift + form.bits < 32 else 0)
    return high | (digit << np.uint32(shift)) | low


def run_keys(rig, name, form, shift, keys):
    """one call on `keys`: the verdict is the model's, and every check of the rig"""
    n = len(keys)
    verdict, found = model.msd_verdict(keys, n, form.bits, form.cap)
    if verdict == model.VERDICT_MSD_RUNS:
        assert found == shift, (name, found, shift)
    case = cases.Case(f"{name}-{form.name}", form, shift, "merged", (), verdict)
    values = cases.payload(n)
    rig.upload(keys, values)
    rig.record(rig.stream)
    rig.torch.cuda.synchronize()
    rig.check(case, keys, values)
    return verdict


def shifts(form):
    return (32 - form.bits, 7)   # the top window of uniform keys: 11 | 11 (10 | 11) bits in the two passes; 4 | 3 under a prefix


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_every_bucket_holds_one_to_three_keys(rig, form_name, key_value):
    form = base._setup(rig, form_name, key_value)
    for shift in shifts(form):
        keys = tiny_keys(form, shift, seed=shift)
        assert int(cases.window_histogram(keys, form.bits, shift).min()) >= 1
        assert run_keys(rig, "tiny", form, shift, keys) == model.VERDICT_MSD_RUNS


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("form_name,key_value", MODES)
def test_one_full_bucket_first_or_last_in_drawing_order(rig, form_name, key_value, where):
    """bucket 0 or bucket 2^bits - 1 at the capacity; 62 other buckets hold the one key the sample needs, the rest none"""
    form = base._setup(rig, form_name, key_value)
    digit = 0 if where == "first" else (1 << form.bits) - 1
    for shift in shifts(form):
        low = {digit: cases.content("random", form.cap, shift, np.random.default_rng(shift + digit))}
        keys = cases.build(form.bits, shift, model.PREFIX, low, "merged", seed=shift)
        hist = cases.window_histogram(keys, form.bits, shift)
        assert int(hist[digit]) == form.cap and int((hist == 0).sum()) == (1 << form.bits) - model.SAMPLE_KEYS
        assert run_keys(rig, "full-" + where, form, shift, keys) == model.VERDICT_MSD_RUNS


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_the_ticket_starts_at_zero_for_every_sort_through_one_storage(rig, form_name, key_value):
    """two plan sorts one behind the other, then a sort the device turns down (four passes, which draw their tiles from the
    same words), then a plan sort again: the storage is as the call before left it every time"""
    form = base._setup(rig, form_name, key_value)
    shift = 32 - form.bits
    assert run_keys(rig, "again-1", form, shift, tiny_keys(form, shift, seed=1)) == model.VERDICT_MSD_RUNS
    assert run_keys(rig, "again-2", form, shift, tiny_keys(form, shift, seed=2)) == model.VERDICT_MSD_RUNS
    declined = cases.overflow_case(form)
    assert run_keys(rig, "declined", form, declined.shift, cases.case_keys(declined)) == model.VERDICT_NONE
    assert run_keys(rig, "behind-four-passes", form, shift, tiny_keys(form, shift, seed=3)) == model.VERDICT_MSD_RUNS
    assert run_keys(rig, "behind-four-passes-7", form, 7, tiny_keys(form, 7, seed=4)) == model.VERDICT_MSD_RUNS


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_counts_of_zero_and_one(rig, form_name, key_value):
    """no key: the plan runs with every bucket empty (the window at its lowest place); one key: nothing to sort"""
    form = base._setup(rig, form_name, key_value)
    assert run_keys(rig, "count-0", form, 2, np.zeros(0, np.uint32)) == model.VERDICT_MSD_RUNS
    assert run_keys(rig, "count-1", form, 2, np.array([0x89ABCDEF], np.uint32)) == model.VERDICT_MSD_SORTED
    assert run_keys(rig, "count-0-again", form, 2, np.zeros(0, np.uint32)) == model.VERDICT_MSD_RUNS
