"""Without a GPU: the inputs of tests/hybrid_bucket_cases.py do what tests/test_hybrid_buckets_gpu.py needs them to do.

  * The forms are the kernel forms of their bounds: the host planner itself (tests/native/plan_check) records the hybrid
    plan with the form's capacity and launch 0's tile geometry, keys-only and key+value, under both rankings where the form
    exists, and every geometry the planner picks either side of an edge of the hybrid rows is some form's.
  * Every case the GPU file runs is taken by the plan as designed (tests/plan_model.py: verdict 1 by byte t, 2 for the cases
    with a bucket of cap + 1 keys), its byte-t histogram is the designed one, and a numpy restatement of bucket_sort_kernel
    + SortInWorkgroup sorts it like numpy's stable sort.
  * The named contents produce the slots their names promise, in the pass they name.
  * The inputs bite: with each of seven planted faults at least one of the GPU file's calls comes out different in every
    form the fault can touch.
"""
import numpy as np
import pytest

import hybrid_bucket_cases as cases
import plan_check_tool as tool
import plan_model as model

MI355X_CUS = 256
ONE_FORM_PER_CAPACITY = ["b4", "b8", "b16", "b32-a"]   # (b32-b and b32-c run b32-a's keys: checked below)


# ---- the forms -------------------------------------------------------------------------------------------------------

def test_the_forms_are_the_kernel_forms_of_their_bounds():
    sizes = [f.bound for f in cases.FORMS.values()] + [f.filled for f in cases.FORMS.values() if f.filled]
    for atomic in (True, False):
        got = tool.describe(MI355X_CUS, atomic, sizes)
        for f in cases.FORMS.values():
            if not (atomic or f.ballot):
                continue
            for n, keys, kv in ((f.bound, f.config_keys, f.config_kv), (f.filled, f.filled_keys, f.filled_kv)):
                if n is None:
                    continue
                for key_value, config in ((False, keys), (True, kv)):
                    row = got[n, key_value]
                    assert (row.name, row.bits, row.hybrid_cap, row.launches, row.config) == (
                        "hybrid-8", 8, f.cap, 6, config), (f.name, n, atomic, key_value, row)
            assert model.hybrid_capacity(f.bound) == f.cap and f.kpt * 1024 == f.cap
            assert f.bound % 2 == 1 and (f.filled is None or f.filled % 2 == 1)
    assert [f.name for f in cases.FORMS.values() if f.ballot] == ["b4", "b8", "b16"]
    assert [f.name for f in cases.FORMS.values() if f.kpt < 8] == ["b4"]          # the one form that is not DYN


def test_every_geometry_either_side_of_an_edge_of_the_hybrid_rows_is_a_form():
    have = {(f.config_keys, f.config_kv, f.cap) for f in cases.FORMS.values()}
    have |= {(f.filled_keys, f.filled_kv, f.cap) for f in cases.FORMS.values() if f.filled}
    sizes = tool.edge_sizes(tool.ATOMIC_TABLE[:5])
    got = tool.describe(MI355X_CUS, True, sizes)
    seen = set()
    for n in sizes:
        if got[n, False].name == "hybrid-8":
            assert got[n, True].name == "hybrid-8" and got[n, True].hybrid_cap == got[n, False].hybrid_cap
            seen.add((got[n, False].config, got[n, True].config, got[n, False].hybrid_cap))
    assert len(seen) >= 5 and seen <= have, seen - have


def test_the_ladders():
    """12 ... 24 buckets either side of every edge of the dealing and of the capacity; the key counts of one call"""
    totals = {}
    for f in cases.FORMS.values():
        sizes, lad = cases.ladder_sizes(f), cases.ladder(f)
        w = cases.WAVES
        assert sorted(lad.values()) == list(sizes) and 12 <= len(sizes) <= 24 and max(sizes) == f.cap
        assert {0, 1, 254, 255} <= set(lad) and cases.OVERFLOW_DIGIT not in lad and not set(cases.TWO_DIGITS) & set(lad)
        want = {1, 2, 63, 64, 65, 255, 256, 257, 256 * (w - 1) + 1, 256 * w - 1, 256 * w, f.cap - 256, f.cap - 255, f.cap - 1,
                f.cap}
        if f.cap > 4096:   # chunks = 1, 15, 16, 17, 31, 32, cap / 256 - 1, cap / 256; n = 1, 255, 0 mod 256
            want |= {256 * w + 1, 256 * (w + 1), 256 * (w + 1) + 1, 256 * (2 * w - 1), 256 * (2 * w - 1) + 1, 512 * w}
        if f.cap > 8192:
            want |= {512 * w + 1}
        if f.cap == 32768:
            want |= {256 * 5 * w, 256 * 5 * w + 1}
        assert want == set(sizes), f.name
        totals[f.cap] = sum(sizes)
    assert totals == {4096: 16_835, 8192: 58_053, 16384: 123_079, 32768: 188_615 + 256 * 160 + 1}


def test_forms_of_one_capacity_run_the_same_keys():
    a = cases.FORMS["b32-a"]
    for name in ("b32-b", "b32-c"):
        f = cases.FORMS[name]
        for key_value in (False, True):
            def plain(c, of):
                return c.name.replace(of, "b32-a"), c.t, c.order, c.buckets, c.verdict, cases.case_seed(c)
            mine = {plain(c, name) for c in cases.gpu_cases(f, key_value)}
            theirs = {plain(c, "b32-a") for c in cases.gpu_cases(a, key_value) if c.direct is None}
            assert mine == theirs


def test_over_the_turns_every_ladder_bucket_holds_every_content():
    for f in cases.FORMS.values():
        for key_value in (False, True):
            seen = {(size, name) for turn in range(len(cases.ROTATION))
                    for _, name, size in cases.ladder_case(f, key_value, 3, turn).buckets}
            assert seen == {(size, name) for size in cases.ladder_sizes(f) for name in cases.ROTATION}
    assert len(set(cases.ROTATION)) == len(cases.ROTATION)
    # every content whose name carries a pass is laid out for a pass the kernel runs; under a smaller t for one that it runs
    assert {cases.split_name(name, 3)[1] for name in cases.ROTATION} == {0, 1, 2}
    assert all(cases.split_name(name, 1)[1] == 0 for name in cases.ROTATION)
    assert cases.split_name("lone-lane@2", 3) == ("lone-lane", 2) and cases.split_name("pass1-ones", 3) == ("ones", 1)


# ---- every case: verdict, histogram, arrival order, and the model ----------------------------------------------------

def _all_cases(form):
    listed = {}
    for key_value in (False, True):
        for c in cases.gpu_cases(form, key_value) + (cases.ballot_cases(form, key_value) if form.ballot else []):
            listed.setdefault(c.name, c)
    return list(listed.values())


@pytest.mark.parametrize("form_name", ONE_FORM_PER_CAPACITY)
def test_every_case_is_taken_as_designed_and_the_model_sorts_it(form_name):
    form = cases.FORMS[form_name]
    listed = _all_cases(form)
    declined = 0
    for checked, case in enumerate(listed):
        keys = cases.case_keys(case)
        n = len(keys)
        designed = {digit: size for digit, _, size in case.buckets}
        assert n == sum(designed.values()) and len(designed) == len(case.buckets), case.name
        if case.direct is None:
            assert n <= 265_000 and n < form.bound, case.name
        else:
            assert n == case.direct == form.filled and model.hybrid_capacity(n) == form.cap, case.name
        hist = cases.byte_histogram(keys, case.t)
        assert all(hist[d] == size for d, size in designed.items()) and int(hist.sum()) == n, case.name   # (the rest: empty)
        verdict = model.hybrid_verdict(keys, n, form.cap)
        assert verdict == (case.verdict, case.t), (case.name, verdict)
        if case.verdict == model.VERDICT_HYBRID_DECLINED:
            declined += 1
            assert int(hist.max()) == form.cap + 1
        else:
            assert int(hist.max()) <= form.cap
        if case.t < 3:   # the bytes above t are the prefix's
            assert not ((keys ^ np.uint32(model.PREFIX)) >> np.uint32(8 * (case.t + 1))).any(), case.name
        if case.direct is None and (not case.name.startswith("ladder") or checked % 4 == 0):
            # arrival order: the keys of a bucket, in input order, are its designed low bits (every fourth ladder)
            lows = cases.bucket_lows(case)
            digit_of = (keys >> np.uint32(8 * case.t)) & np.uint32(0xFF)
            for digit, low in lows.items():
                assert np.array_equal(keys[digit_of == digit] & np.uint32((1 << (8 * case.t)) - 1), low), (case.name, digit)
            if case.order == "grouped":   # whole scatter tiles of one bucket
                big = max(designed, key=designed.get)
                where = np.flatnonzero(digit_of == big)
                assert where[-1] - where[0] == designed[big] - 1
        values = cases.payload(n)
        want = cases.reference(keys, values)
        got = cases.call_model(keys, values, form, case.t)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case.name
    assert declined == len(cases.OVERFLOW_TS)
    print(f"{form.name}: {len(listed)} cases, {declined} of them declined")


def test_top_sentinels_are_real_keys_of_all_ones():
    for form in cases.FORMS.values():
        for size in cases.top_sizes(form):
            keys = cases.case_keys(cases.top_case(form, size))
            assert int((keys == 0xFFFFFFFF).sum()) >= size // 3 and int((keys == 0).sum()) == 1025
            values = cases.payload(len(keys))
            assert (values[keys == 0xFFFFFFFF] != 0).sum() >= size // 3 - 1   # the pad's key with another value than the pad's


# ---- the contents ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 2, 3])
@pytest.mark.parametrize("size", [257, 4097, 8192, 32767])
def test_the_contents_do_what_their_names_say(size, t):
    ones = (1 << (8 * t)) - 1
    chunks, whole_slots, whole_chunks = -(-size // 256), size // 64, size // 256
    first_slots = chunks if size % 256 == 0 or size % 256 >= 64 else size // 256   # chunks whose first slot is whole
    low, census = {}, {}
    for name in cases.ROTATION:
        low[name] = cases.content(name, size, t, np.random.default_rng(7 * size + t))
        assert low[name].dtype == np.uint32 and len(low[name]) == size and int(low[name].max()) <= ones, name
        census[name] = [cases.slot_census(cases.pass_digits(low[name], t, p)) for p in range(t)]
        assert all(len(c["probe"]) == chunks for c in census[name])

    def byte(name, p):
        return (low[name] >> np.uint32(8 * p)) & np.uint32(0xFF)

    def at(name):
        """the census of the pass the name is laid out for, and that pass"""
        p = cases.split_name(name, t)[1]
        return census[name][p], p

    assert len(np.unique(low["all-equal"])) == 1 and not low["zeros"].any() and (low["all-pad-twins"] == ones).all()
    assert all(c["uniform"] >= whole_slots for name in ("all-equal", "zeros", "all-pad-twins") for c in census[name])
    two = low["two-values"]
    assert len(np.unique(two)) == 2 and (two[:-1] != two[1:]).all() and all(byte("two-values", p)[0] != byte("two-values", p)[1]
                                                                               for p in range(t))
    assert (census["two-values"][0]["pair"][:whole_slots] == 32).all()            # ballots, 32 and 32, in pass 0 ...
    assert all(c["uniform"] >= whole_slots - 1 for c in census["two-values"][1:])  # ... and one digit per slot behind it
    up = low["ascending"]
    assert (up[:-1] <= up[1:]).all() and up[0] == 0 and up[-1] >= ones - (1 << (8 * t)) // size - 1
    assert np.array_equal(low["descending"], up[::-1])
    twins = low["pad-twins"] == ones
    assert twins[0] and twins[-1] and twins[::3].all()
    for p in range(3):
        name = f"pass{p}-ones"
        q = p % t
        assert (byte(name, q) == 0xFF).all() and all((byte(name, o) != 0xFF).all() for o in range(t) if o != q), name
        name = f"pass{p}-uniform"
        assert len(np.unique(byte(name, q))) == 1 and census[name][q]["uniform"] >= whole_slots, name
        assert all(census[name][o]["uniform"] <= 4 for o in range(t) if o != q), name
    assert all(c["uniform"] <= 4 for c in census["random"])
    # whole slots and chunks of one digit; the same runs one position early: 63 + 1 in every slot, lane 0 among the 63
    for name in ("runs64", "runs256", "runs64+1", "runs64+1@1"):
        c, p = at(name)
        if name in ("runs64", "runs256"):
            assert c["uniform"] >= whole_slots and (c["probe"][:first_slots] == 0).all(), name
        else:
            assert c["lone0"] >= whole_slots - 1 and c["uniform"] <= 4 and (c["probe"][:first_slots] == 1).all(), (name, p)
    if size >= 512:
        assert len(np.unique(byte("runs256", 0)[:256])) == 1 and byte("runs256", 0)[255] != byte("runs256", 0)[256]
    # the probe's slot against the other three
    for name in ("first-slot-only-uniform", "first-slot-only-uniform@2"):
        c, _ = at(name)
        assert (c["probe"][:first_slots] == 0).all() and first_slots <= c["uniform"] <= first_slots + 4, name
    c, _ = at("first-slot-only-mixed")
    assert (c["probe"][:first_slots] > 48).all() and c["uniform"] >= 3 * whole_chunks   # (not watched, yet uniform slots)
    for name in ("probe-48", "probe-49", "probe-48@1", "probe-49@2", "probe-48@2", "probe-49@1"):
        c, _ = at(name)
        differ = int(name[6:8])
        assert (c["probe"][:first_slots] == differ).all() and first_slots >= 1 and c["uniform"] <= 4, name
        assert (c["pair"][::4][:first_slots] == -1).all(), name    # 48 lanes that differ, but not ONE other digit
    for name in ("pair-48", "pair-49", "pair-48@2", "pair-49@1", "pair-48@1", "pair-49@2"):
        c, _ = at(name)
        second = int(name[5:7])
        inner = np.arange(whole_slots) % 4 != 0
        assert c["watched"][:4 * first_slots].all() and (c["pair"][:whole_slots][inner] == second).all(), name
        assert (c["pair"][:whole_slots][~inner] == (48 if second == 48 else -1)).all(), name
    for name in ("lone-lane", "lone-lane@1", "lone-lane@2"):
        c, _ = at(name)
        assert c["lone"] >= whole_slots and c["watched"][:4 * first_slots].all(), name
        assert 0 < c["lone0"] and (size < 4096 or c["lone0"] < c["lone"]), name   # lane 0 among the 63, and lane 0 alone


def test_later_passes_see_the_order_the_pass_before_left():
    """a content laid out for pass 1 does not show in arrival order: its slots are made by pass 0's stable order"""
    rng = np.random.default_rng(11)
    low = cases.content("lone-lane@1", 4096, 3, rng)
    arrival = ((low >> np.uint32(8)) & np.uint32(0xFF)).reshape(-1, 64)
    assert cases.slot_census(arrival)["lone"] == 0 and cases.slot_census(cases.pass_digits(low, 3, 1))["lone"] == 64


def test_a_bucket_with_pads_holds_pad_twins_in_every_ladder():
    """ragged buckets get pad twins over the turns: real keys with the pad's digit in every pass, in front of real pads"""
    for form in cases.FORMS.values():
        ragged = [size for size in cases.ladder_sizes(form) if size % 256 and size > 256]
        assert len(ragged) >= 3
        for size in ragged[:2] + ragged[-2:]:
            low = cases.content("pad-twins", size, 3, np.random.default_rng(size))
            for p in range(3):
                digits = cases.pass_digits(low, 3, p)
                assert int((digits == 0xFF).sum()) >= size // 3 + (256 - size % 256)


# ---- the inputs bite -------------------------------------------------------------------------------------------------

def _candidates(form, fault):
    """the GPU file's key+value calls the plan takes, without the filled direct sorts"""
    listed = [c for c in cases.gpu_cases(form, True) if c.verdict == model.VERDICT_HYBRID_RUNS and c.direct is None]
    if fault == "one-pass-short":
        listed = [c for c in listed if c.t >= 1]
    return listed


def _differs(case, fault, values=None, key_value=True):
    keys = cases.case_keys(case)
    values = cases.payload(len(keys)) if values is None else values
    want = cases.reference(keys, values)
    got = cases.call_model(keys, values, case.form, case.t, fault)
    keys_differ = not np.array_equal(got[0], want[0])
    return keys_differ, keys_differ or (key_value and not np.array_equal(got[1], want[1]))


@pytest.mark.parametrize("fault", cases.FAULTS)
def test_every_planted_fault_changes_the_result_of_a_gpu_case(fault):
    """With the fault planted in the model, a call of the GPU file's list comes out different from the stable sort in every
    form the fault can touch.  dropped-chunk (5) touches only the forms whose dealing is computed (KPT >= 8): in b4 wave w
    takes chunk w, there is no `extra`, and the model leaves b4's calls as they are -- asserted, not skipped.
    stale-value-ranks (6) shows in the values alone; one-pass-short (7) needs t >= 1."""
    for form_name in ONE_FORM_PER_CAPACITY:
        form = cases.FORMS[form_name]
        listed = _candidates(form, fault)
        if fault == "dropped-chunk" and form.kpt < 8:
            assert not any(_differs(case, fault)[1] for case in listed[:3] + listed[-3:])
            continue
        caught = None
        for case in listed:
            keys_differ, differs = _differs(case, fault)
            assert not (fault == "stale-value-ranks" and keys_differ)
            if differs:
                caught = case.name
                break
        assert caught is not None, (fault, form_name)
        print(f"{fault}: {form_name} caught by {caught}")


def test_one_pass_short_and_stale_value_ranks_need_their_cases():
    """one-pass-short changes nothing at t = 0 (there is no pass), stale-value-ranks nothing at t <= 1 (there is no pass
    before) and nothing in a keys-only call"""
    form = cases.FORMS["b8"]
    assert not _differs(cases.ladder_case(form, True, 0, 4), "one-pass-short")[1]
    assert not _differs(cases.ladder_case(form, True, 1, 4), "stale-value-ranks")[1]
    assert not _differs(cases.ladder_case(form, False, 3, 4), "stale-value-ranks", key_value=False)[1]
    assert _differs(cases.ladder_case(form, True, 3, 4), "stale-value-ranks") == (False, True)


def test_iota_values_hide_a_pad_in_the_place_of_a_real_sentinel():
    """Values that are all different show every wrong permutation, iota as well as payload: stale-value-ranks (6) never moves
    a pad's value in front of position n, so what it leaves is a permutation of the values, and no injective labelling lets
    it through.  What iota does let through is a PAD stored in the place of a real key: the pad is (0xFFFFFFFF, 0), and with
    iota the call's first element is the one real key that may look like it.  pads-first (1) on a bucket 255 whose only
    sentinel is the call's first key passes with iota and is caught with payload, whose 0 sits elsewhere."""
    rng = np.random.default_rng(5)
    top = np.concatenate([[0xFFFFFF], cases._rand(rng, 24, 256, exclude_ones=True)]).astype(np.uint32)
    keys = cases.build(3, {255: top, 0: np.zeros(300, np.uint32)}, "grouped", 1)
    assert keys[0] == 0xFFFFFFFF and int((keys == 0xFFFFFFFF).sum()) == 1
    form = cases.FORMS["b8"]
    for values, hidden in ((np.arange(len(keys), dtype=np.uint32), True), (cases.payload(len(keys)), False)):
        want = cases.reference(keys, values)
        got = cases.call_model(keys, values, form, 3, "pads-first")
        assert (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])) == hidden
    # and fault 6, on a case that shows it: with either labelling
    case = cases.ladder_case(form, True, 3, 4)
    n = len(cases.case_keys(case))
    assert _differs(case, "stale-value-ranks", values=np.arange(n, dtype=np.uint32))[1]
    assert _differs(case, "stale-value-ranks", values=cases.payload(n))[1]


def test_the_faults_need_the_designed_contents():
    """What uniform keys in evenly filled buckets -- the inputs the suite had -- let through: a bucket of whole chunks, as many
    as the waves, has no pads to rank first and no extra chunk to drop, and random slots are never 63 + 1 or two-valued."""
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 24, size=4096, dtype=np.uint64).astype(np.uint32) | np.uint32(0x5A000000)
    values = cases.payload(len(keys))
    want = cases.reference(keys, values)
    for fault in ("pads-first", "lone-lane-uniform", "pair-second-from-first", "dropped-chunk"):
        got = cases.bucket_model(keys, values, 3, cases.WAVES, fault)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), fault
