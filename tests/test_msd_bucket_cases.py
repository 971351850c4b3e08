"""Without a GPU: the inputs of tests/msd_bucket_cases.py do what tests/test_msd_buckets_gpu.py needs them to do.

  * Every case that file runs is taken by the MSD plan with the window where the case wants it (tests/plan_model.py with the
    bits and the capacity of the form's bound), its window histogram is the designed one, and the case with a bucket of
    cap + 1 keys is turned down.
  * The named contents produce the slots their names promise, by a numpy restatement of the bucket kernel's slot layout.
  * The inputs bite: a numpy model of BucketSort2Bucket equals the stable sort, and with each of five planted faults at least
    one of the GPU file's calls comes out different -- three of them in the values alone.
"""
import numpy as np
import pytest

import msd_bucket_cases as cases
import plan_model as model
from test_sort_gpu import MSD_FROM, MSD_HALF_UP_TO, msd_capacity

FORM_NAMES = list(cases.FORMS)
MODES = [(name, key_value) for name in FORM_NAMES for key_value in (False, True)]


def test_the_forms_are_the_kernel_forms_of_their_bounds():
    for f in cases.FORMS.values():
        assert MSD_FROM <= f.bound <= (1 << 26) and msd_capacity(f.bound, f.bits) == f.cap
        assert (f.cap == 18432) == (f.bound <= MSD_HALF_UP_TO) == (f.waves == 8)
        assert f.cap % (64 * f.waves) == 0 and f.cap // (64 * f.waves) == 36   # 36 slots per lane
        sizes = cases.ladder_sizes(f)
        assert len(sizes) == len(set(sizes)) == len(cases.LADDER_DIGITS[f.bits]) == 17 and max(sizes) == f.cap
        digits = cases.LADDER_DIGITS[f.bits]
        assert sorted(digits.values()) == list(range(17)) and {1, (1 << f.bits) - 2} <= set(digits)
        half = (1 << f.bits) // 2
        assert sum(1 for b in digits if b + half in digits) >= 4      # workgroups that sort two designed buckets
    assert {767, 768} <= set(cases.LADDER_DIGITS[10])                # the last streamed bucket and the first plain one
    assert cases.FORMS["full10-streamed"].bound >= 1 << 25 and cases.FORMS["full10"].bound > 1 << 24


@pytest.mark.parametrize("form_name,key_value", MODES)
def test_the_plan_takes_every_case_with_the_designed_window_and_buckets(form_name, key_value):
    form = cases.FORMS[form_name]
    listed = cases.gpu_cases(form, key_value)
    assert len({c.name for c in listed}) == len(listed)
    declined = 0
    for case in listed:
        keys = cases.case_keys(case)
        n = len(keys)
        designed = {digit: size for digit, _, size in case.buckets}
        assert n == sum(designed.values()) + 64 - sum(1 for b in (0, (1 << form.bits) - 1) if designed.get(b)), case.name
        assert n <= 180_000 and n < form.bound   # (the 1024-thread ladder: 176 132 keys)
        window = model.msd_window(keys, n, form.bits, form.cap)
        assert (window["varying"], window["lowest"], window["spread"], window["mode"]) == (
            case.shift + form.bits, case.shift, form.bits, model.MODE_PLAN), case.name
        hist = cases.window_histogram(keys, form.bits, case.shift)
        for digit, size in designed.items():
            assert hist[digit] == size, (case.name, digit)
        others = np.delete(hist, list(designed))
        assert int(others.sum()) == n - sum(designed.values()) and int(others.max()) == 1, case.name
        verdict = model.msd_verdict(keys, n, form.bits, form.cap)
        if case.verdict == model.VERDICT_NONE:
            declined += 1
            assert int(hist.max()) == form.cap + 1 and verdict == (model.VERDICT_NONE, None), case.name
        else:
            assert int(hist.max()) <= form.cap and verdict == (model.VERDICT_MSD_RUNS, case.shift), case.name
        # arrival order: the keys of a bucket, in input order, are its designed low bits
        lows = cases.bucket_lows(case)
        digit_of = (keys >> np.uint32(case.shift)) & np.uint32((1 << form.bits) - 1)
        for digit, low in lows.items():
            assert np.array_equal(keys[digit_of == digit] & np.uint32((1 << case.shift) - 1), low), (case.name, digit)
        if case.order == "grouped" and len(case.buckets) > 3:   # whole scatter tiles of one bucket
            big = max(designed, key=designed.get)
            where = np.flatnonzero(digit_of == big)
            assert where[-1] - where[0] < designed[big] + 64
    assert declined == 1


@pytest.mark.parametrize("form_name", FORM_NAMES)
def test_every_content_sits_in_every_ladder_bucket_under_an_odd_and_an_even_below(form_name):
    form = cases.FORMS[form_name]
    sizes = cases.ladder_sizes(form)
    seen = set()
    for key_value in (False, True):
        for shift in cases.shifts_of(form):
            for _, name, size in cases.ladder_case(form, key_value, shift).buckets:
                seen.add((name, size, shift % 2))
    assert seen == {(name, size, parity) for name in cases.ROTATION for size in sizes for parity in (0, 1)}
    assert any(size % 256 and 256 < size < form.cap - 256 for size in sizes)   # ragged mid-size buckets exist


BELOWS = (2, 3, 4, 11, 12, 21, 22)


@pytest.mark.parametrize("below", BELOWS)
@pytest.mark.parametrize("size", [257, 4097, 18432, 36863])
def test_the_contents_do_what_their_names_say(size, below):
    w0, w1 = cases.widths(below)
    ones, ones0, ones1 = (1 << below) - 1, (1 << w0) - 1, (1 << w1) - 1
    chunks, whole_slots, whole_chunks = -(-size // 256), size // 64, size // 256
    first_slots = -(-size // 256) if size % 256 == 0 or size % 256 >= 64 else size // 256   # chunks whose first slot is whole
    census = {}
    lows = {}
    for name in cases.ROTATION + ("zeros", "top-sentinels"):
        low = cases.content(name, size, below, np.random.default_rng(7 * size + below))
        assert low.dtype == np.uint32 and len(low) == size and int(low.max()) <= ones, name
        lows[name] = low
        census[name] = [cases.slot_census(cases.pass_digits(low, below, which)) for which in (0, 1)]
        assert len(census[name][0]["probe"]) == chunks
    d0 = {name: low & np.uint32(ones0) for name, low in lows.items()}
    d1 = {name: low >> np.uint32(w0) for name, low in lows.items()}

    assert len(np.unique(lows["all-equal"])) == 1 and not lows["zeros"].any()
    assert census["all-equal"][0]["uniform"] >= whole_slots and census["all-equal"][1]["uniform"] >= whole_slots
    two = lows["two-values"]
    assert len(np.unique(two)) == 2 and (two[:-1] != two[1:]).all() and d0["two-values"][0] != d0["two-values"][1] \
        and d1["two-values"][0] != d1["two-values"][1]
    assert census["two-values"][0]["uniform"] <= 4 and (census["two-values"][0]["probe"][:first_slots] == 32).all()
    up = lows["ascending"]
    assert (up[:-1] <= up[1:]).all() and up[0] == 0 and up[-1] >= ones - (1 << below) // size - 1
    assert np.array_equal(lows["descending"], up[::-1])
    for name in ("pad-twins", "top-sentinels"):
        twins = lows[name] == ones
        assert size % 256 != 0 or name == "top-sentinels" or size == 18432   # (pads exist where the ladder is ragged)
        assert twins[0] and twins[-1] and twins[::3].all() and twins.sum() >= size // 3
    assert (lows["all-pad-twins"] == ones).all()
    assert (d0["pass0-ones"] == ones0).all() and (d1["pass0-ones"] != ones1).all()
    assert (d1["pass1-ones"] == ones1).all() and (d0["pass1-ones"] != ones0).all()
    # whole slots and chunks of one pass-0 digit; the same runs one arrival early: 63 + 1 in every slot, lane 0 in the 63
    assert census["runs64"][0]["uniform"] >= whole_slots and (census["runs64"][0]["probe"][:first_slots] == 0).all()
    assert census["runs256"][0]["uniform"] >= 4 * whole_chunks
    if size >= 512:
        assert len(np.unique(d0["runs256"][:256])) == 1 and d0["runs256"][255] != d0["runs256"][256]
    assert census["runs64+1"][0]["lone"] >= whole_slots - 1 and census["runs64+1"][0]["uniform"] <= 4
    assert (census["runs64+1"][0]["probe"][:first_slots] == 1).all()      # ... in chunks that watch
    # the probe's slot against the other three
    c = census["first-slot-only-uniform"][0]
    assert (c["probe"][:first_slots] == 0).all() and first_slots <= c["uniform"] <= first_slots + 4
    c = census["first-slot-only-mixed"][0]
    assert (c["probe"][:first_slots] > 0).all() and c["uniform"] >= 3 * whole_chunks
    if w0 >= 8:   # (a random first slot of 64 keys with 256 or more digits: the chunk is not watched)
        assert (c["probe"][:first_slots] > 48).all()
    assert (census["probe-48"][0]["probe"][:first_slots] == 48).all() and first_slots >= 1
    assert (census["probe-49"][0]["probe"][:first_slots] == 49).all()
    assert census["probe-48"][0]["uniform"] <= 4 and census["probe-49"][0]["uniform"] <= 4
    # one pass all uniform, the other not
    assert census["pass1-uniform"][1]["uniform"] >= whole_slots and census["pass1-uniform"][0]["uniform"] <= 4
    assert census["pass0-uniform"][0]["uniform"] >= whole_slots and census["pass0-uniform"][1]["uniform"] <= 4
    assert census["random"][0]["uniform"] <= 4 and census["random"][1]["uniform"] <= 4


def test_a_bucket_with_pads_holds_pad_twins_in_every_ladder():
    """the ragged buckets of the ladder get pad twins: real keys with the pad's digit in both passes, in front of real pads"""
    for form in cases.FORMS.values():
        found = 0
        for shift in cases.shifts_of(form):
            for _, name, size in cases.ladder_case(form, False, shift).buckets:
                if name == "pad-twins" and size % 256 and size > 256:
                    digits = cases.pass_digits(cases.content(name, size, shift, np.random.default_rng(1)), shift, 1)
                    w1 = cases.widths(shift)[1]
                    pads = 256 - size % 256
                    assert int((digits == (1 << w1) - 1).sum()) >= size // 3 + pads and pads > 0
                    found += 1
        assert found >= 5, form.name


def test_top_sentinels_are_real_keys_of_all_ones():
    for form in cases.FORMS.values():
        for size in cases.top_sizes(form):
            keys = cases.case_keys(cases.top_case(form, size))
            assert int((keys == 0xFFFFFFFF).sum()) >= size // 3 and keys[-1] == 0xFFFFFFFF
            assert int((keys == 0).sum()) == 4097 and keys[0] == 0


# ---- the inputs bite -------------------------------------------------------------------------------------------------

def _taken(form_name, key_value):
    return [c for c in cases.gpu_cases(cases.FORMS[form_name], key_value) if c.verdict == model.VERDICT_MSD_RUNS]


@pytest.mark.parametrize("form_name,key_value", [("half", False), ("full10-streamed", True), ("eleven", False)])
def test_the_model_without_a_fault_is_the_stable_sort(form_name, key_value):
    for case in _taken(form_name, key_value)[::3] + _taken(form_name, key_value)[-8:]:
        keys = cases.case_keys(case)
        values = cases.payload(len(keys))
        want = cases.reference(keys, values)
        got = cases.call_model(keys, values, case.form, case.shift)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case.name


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_every_planted_fault_changes_the_result_of_a_gpu_case(fault):
    """With the fault planted in the model, calls of the GPU file's list come out different from the stable sort in every
    form: pads-first, pass1-unstable and stale-value-ranks in the values alone (stale-value-ranks in nothing else)."""
    by_values = fault in ("pads-first", "pass1-unstable", "stale-value-ranks")
    for form_name in FORM_NAMES:
        caught = None
        for case in _taken(form_name, True):
            keys = cases.case_keys(case)
            values = cases.payload(len(keys))
            want = cases.reference(keys, values)
            got = cases.call_model(keys, values, case.form, case.shift, fault)
            if fault == "stale-value-ranks":
                assert np.array_equal(got[0], want[0])
            if not np.array_equal(got[1], want[1]) or (not by_values and not np.array_equal(got[0], want[0])):
                caught = case.name
                break
        assert caught is not None, (fault, form_name)


def test_the_faults_need_the_designed_contents():
    """What uniform keys in evenly filled buckets -- the inputs the suite had -- let through: a bucket of whole chunks has
    no pads to rank first, and random slots are never 63 + 1."""
    form = cases.FORMS["half"]
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 22, size=4096, dtype=np.uint64).astype(np.uint32)
    values = cases.payload(len(keys))
    want = cases.reference(keys, values)
    for fault in ("pads-first", "lone-lane-uniform", "dropped-chunk"):
        got = cases.bucket_model(keys, values, 22, form.waves, fault)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), fault
