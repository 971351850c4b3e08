"""Without a GPU: the inputs of tests/storage_reuse_cases.py are what their names say.  Every call of CALLS is put through
tests/plan_model.py with the constants the host uses at its bound -- ten bits and msd_capacity() where the MSD plan is
recorded, hybrid_capacity() for the hybrid plan, the ballot sorter's capacity rule (HybridCapacity in vrdx_plan.h: no
bucket beyond 16384, and never the MSD plan) -- and the verdict must be the one the table of CALLS states.  A generator that
changes cannot turn a "declined" call into an "accepted" one, or the other way round, without this file noticing.

The rows of the newer families are held to their own case modules the same way: every range row goes through
range_sort_cases.sort_range_model at three CU counts and must show the mask, the copy back, the chunks and the scratch writes
that RANGE_FACTS states; the wide-value rows have the form their name says at their bound; the segmented rows hold every size
class of their family; the ordered rows hold the special values of their key type.  And the matrix is sensitive to the clears
it newly covers: the same model, told what the storage held before -- totals that are not zero, a mask that is not rewritten,
count rows of a longer sort -- gives another result for the inputs of every range row."""
import numpy as np
import pytest

import key_order32_cases
import key_order_cases
import plan_model as model
import range_sort_cases
import storage_reuse_cases as cases
import wide_value_cases
import wide_value_segmented_cases
from test_sort_gpu import MSD_FROM, MSD_HALF_UP_TO, msd_capacity

MI355X_CUS = 256
CU_COUNTS = (MI355X_CUS, 1, 304)
RANGE_ROWS = [c.name for c in cases.CALLS if cases.is_range_sort(c)]


def test_the_names_are_the_issue_list_and_unique():
    assert len(set(cases.NAMES)) == len(cases.CALLS) == 38
    assert {c.sorter for c in cases.CALLS} == {"atomic", "ballot"}
    assert {c.requirement for c in cases.CALLS} == {"keys", "key-value", "keys64", "key-value64", "wide-value"}
    # the first 21 rows are the table as it stood: name for name, with nothing of the newer families in them
    assert cases.NAMES[:cases.FIRST_CALLS] == [
        "msd-runs-keys", "msd-runs-pairs", "msd-declined-keys", "msd-declined-pairs-skips", "msd-all-equal", "msd-indirect-small",
        "msd-indirect-declined", "tail-split", "block-sums", "hybrid-runs", "hybrid-declined", "one-workgroup",
        "ballot-four-passes", "ballot-hybrid", "segmented", "segmented-invalid", "segmented64", "sort64-pairs", "sort64-indirect",
        "sort64-small", "empty"]
    assert all((c.bits, c.order, c.form) == (None, None, None) for c in cases.CALLS[:cases.FIRST_CALLS])
    assert sorted(RANGE_ROWS) == sorted(cases.RANGE_FACTS)
    assert {c.requirement == "wide-value" for c in cases.CALLS if cases.has_wide_values(c)} == {True}
    assert [c.name for c in cases.CALLS if c.failure not in (0, cases.INHERITED)] == ["segmented-invalid"]
    assert [c.name for c in cases.CALLS if c.verdict == cases.INHERITED] == ["empty"]


def test_the_constants_of_the_bounds():
    """The sizes select what the table says: the MSD plan with the half-size bucket kernel at M, at one round and at two
    rounds + 1; the hybrid plan with buckets of 4096 at H for both rankings; nothing but the four passes for the ballot
    sorter at M; one workgroup up to 16384."""
    assert cases.M % 4 == 3
    for n in (cases.M, cases.BLOCK_SUMS_N, cases.TAIL_SPLIT_N):
        assert MSD_FROM <= n <= MSD_HALF_UP_TO and model.hybrid_capacity(n) == 0 and msd_capacity(n, cases.MSD_BITS) == 18432
    assert model.hybrid_capacity(cases.H) == cases.ballot_hybrid_capacity(cases.H) == 4096
    assert cases.ballot_hybrid_capacity(cases.M) == 0
    assert cases.ballot_hybrid_capacity(4_000_000) == 16384 and cases.ballot_hybrid_capacity(4_200_000) == 0
    assert cases.BY_NAME["one-workgroup"].bound == 16384 and cases.BY_NAME["sort64-small"].bound <= 16384
    assert cases.BY_NAME["bits-one-workgroup"].bound == 16384 and cases.BY_NAME["ordered-small"].bound <= 16384
    # a row that records the MSD plan at another bound than M takes bits and capacity from the table of plan edges
    assert cases.msd_constants(cases.BY_NAME["ordered-msd"]) == (cases.MSD_BITS, 18432)
    two_sorts = cases.BY_NAME["wide-two-sorts-indirect"]
    assert MSD_FROM <= two_sorts.bound <= MSD_HALF_UP_TO and cases.msd_constants(two_sorts) == (10, 18432)
    for c in cases.CALLS:
        if c.count is not None:
            assert 0 < c.count < c.bound, c.name


@pytest.mark.parametrize("name", [c.name for c in cases.CALLS if not cases.is_segmented(c) and c.name != "empty"])
def test_the_model_gives_the_verdict_of_the_table(name):
    call = cases.BY_NAME[name]
    verdict, where = cases.verdict_of(call)
    assert verdict == call.verdict, (name, verdict, where)
    keys, values, _ = cases.inputs_of(call)
    assert len(keys) == call.bound and (values is None or len(values) == call.bound)
    assert keys.dtype == (np.uint64 if cases.is_wide(call) else np.uint32)
    if values is not None:   # random words, never the index
        assert values.dtype == (np.uint64 if cases.has_wide_values(call) else np.uint32)
        assert int((values == np.arange(len(values), dtype=np.uint32)).sum()) < 4
    if values is not None and cases.has_wide_values(call):   # ... with random high words
        high = (values >> np.uint64(32)).astype(np.uint32)
        assert len(np.unique(high[:4096])) > 4000 and int((high == (values & np.uint64(0xFFFFFFFF))).sum()) == 0


def test_the_uniform_msd_calls_scatter_by_the_top_bits():
    """uniform keys: the window lies at the top, also under the small device-side count"""
    for name in ("msd-runs-keys", "msd-runs-pairs", "msd-indirect-small"):
        assert cases.verdict_of(cases.BY_NAME[name]) == (model.VERDICT_MSD_RUNS, 32 - cases.MSD_BITS), name


def test_the_declined_calls_are_declined_for_the_reason_in_their_name():
    """decline_msd's keys: one bucket beyond the capacity (whether the sample or the spine finds it).  The keys with two
    constant bytes: the top byte varies, so the window is at the top, where 256 of its 1024 buckets hold all the keys."""
    for name in ("msd-declined-keys", "msd-indirect-declined", "tail-split", "block-sums"):
        call = cases.BY_NAME[name]
        keys = cases.inputs_of(call)[0][:cases.sorted_count(call)]
        top = np.bincount(keys >> np.uint32(32 - cases.MSD_BITS), minlength=1 << cases.MSD_BITS)
        assert int(top.max()) >= 40000 > msd_capacity(call.bound, cases.MSD_BITS), name
    skips = cases.inputs_of(cases.BY_NAME["msd-declined-pairs-skips"])[0]
    assert bool(((skips >> np.uint32(8)) & np.uint32(0xFFFF) == 0xA5C3).all())     # bytes 1 and 2 are constant ...
    assert len(np.unique(skips & np.uint32(0xFF))) == 256 and len(np.unique(skips >> np.uint32(24))) == 256   # ... 0 and 3 are not
    window = model.msd_window(skips, cases.M, cases.MSD_BITS, 18432)
    assert window["lowest"] == 22 and window["mode"] == model.MODE_PLAN   # the sample lets it through: the spine declines
    top = np.bincount(skips >> np.uint32(22), minlength=1024)
    assert int((top != 0).sum()) == 256 and int(top.max()) > 18432


def test_the_hybrid_calls_sit_at_the_capacity():
    heavy = cases.inputs_of(cases.BY_NAME["hybrid-declined"])[0]
    assert int(np.bincount(heavy >> np.uint32(24), minlength=256).max()) == 4096 + 1
    for name in ("hybrid-runs", "ballot-hybrid"):
        keys = cases.inputs_of(cases.BY_NAME[name])[0]
        assert cases.verdict_of(cases.BY_NAME[name]) == (model.VERDICT_HYBRID_RUNS, 3)
        assert int(np.bincount(keys >> np.uint32(24), minlength=256).max()) <= 4096
    # the 64-bit calls: the second inner sort scatters the high words by their top byte (63-bit keys) and by byte 1 (a
    # sixteen-bit tile id)
    assert cases.verdict_of(cases.BY_NAME["sort64-pairs"]) == (model.VERDICT_HYBRID_RUNS, 3)
    assert cases.verdict_of(cases.BY_NAME["sort64-indirect"]) == (model.VERDICT_HYBRID_RUNS, 1)


def test_the_one_workgroup_call_has_eight_bit_keys():
    keys = cases.inputs_of(cases.BY_NAME["one-workgroup"])[0]
    assert int(keys.max()) < 256 and len(np.unique(keys)) == 256


@pytest.mark.parametrize("name,mid_max", [
    ("segmented", 16384), ("segmented64", 16384), ("segmented-bits", 16384), ("ordered-segmented", 16384),
    ("segmented64-ordered", 16384), ("wide-segmented", wide_value_segmented_cases.MID_MAX)])
def test_the_segmented_calls_hold_every_size_class(name, mid_max):
    """empty, in-LDS with 256 threads (<= 4096), in-LDS with 1024 threads, through memory -- at least one segment each, inside
    the bound, the offsets increasing.  The large class starts at 8193 for 8-byte values and for 64-bit keys with values, at
    16385 everywhere else."""
    call = cases.BY_NAME[name]
    assert cases.is_segmented(call)
    assert mid_max == (8192 if cases.has_wide_values(call) or (cases.is_wide(call) and cases.is_key_value(call)) else 16384)
    assert (wide_value_segmented_cases.MID_MAX, key_order_cases.MID_MAX_KEY_VALUE) == (8192, 8192)
    _, _, offsets = cases.inputs_of(call)
    sizes = np.diff(offsets.astype(np.int64))
    assert len(sizes) == len(cases.SEGMENT_SIZES) and (sizes >= 0).all() and int(offsets[-1]) <= call.bound
    assert (sizes == 0).any() and ((sizes > 1) & (sizes <= 4096)).any()
    assert ((sizes > 4096) & (sizes <= mid_max)).any() and (sizes > mid_max).any()


def test_the_invalid_offsets_are_invalid_twice():
    call = cases.BY_NAME["segmented-invalid"]
    offsets = cases.inputs_of(call)[2].astype(np.int64)
    assert (np.diff(offsets) < 0).sum() == 1 and int(offsets[-1]) > call.bound
    assert call.failure == cases.STATUS_SEGMENTS_INVALID


def test_the_references_leave_the_tail_alone():
    """expected_of(): sorted up to the count, the input behind it (small calls only: the large ones are sorted on the GPU
    machine, once)"""
    for name in ("one-workgroup", "sort64-small", "sort64-indirect", "segmented-invalid", "range-chunked-keys",
                 "range-chunked-pairs-copy-back", "range-gap-in-mask", "range-equal-field", "range-ballot", "bits-one-workgroup",
                 "ordered-small", "sort64-ordered-pairs", "wide-one-workgroup", "wide-gather"):
        call = cases.BY_NAME[name]
        keys, values, _ = cases.inputs_of(call)
        want_keys, want_values = cases.expected_of(call)
        n = cases.sorted_count(call)
        assert np.array_equal(want_keys[n:], keys[n:]) and np.array_equal(np.sort(want_keys), np.sort(keys))
        if not cases.is_segmented(call):   # in the order the call sorts by: the field, T(key), the key
            by = want_keys[:n]
            if call.bits is not None:
                by = range_sort_cases.field(by, *call.bits)
            elif call.order is not None:
                by = (key_order_cases if cases.is_wide(call) else key_order32_cases).T(by, *call.order)
            assert bool((by[1:] >= by[:-1]).all()), name
        if values is not None:
            pairs = set(zip(keys.tolist(), values.tolist()))
            assert set(zip(want_keys.tolist(), want_values.tolist())) == pairs
    assert len(cases.padded(keys)) == len(keys) + cases.GUARD_ELEMENTS


# ---- the rows of the newer families ------------------------------------------------------------------------------------------

def _small_count_inputs(call):
    """the arrays of a range row as the model needs them: an indirect row under a large bound keeps only what lies in front of
    the count and a few elements behind it (nothing behind the count is read)"""
    keys, values, _ = cases.inputs_of(call)
    if call.count is None:
        return keys, values, {}
    cut = call.count + 16
    return keys[:cut], (values[:cut] if values is not None else None), {"count": call.count, "bound": call.bound}


@pytest.mark.parametrize("name", RANGE_ROWS)
def test_the_range_rows_take_the_path_in_their_name(name):
    """mask of active passes, copy back, chunks that hold keys and whether the scratch arrays are written: what RANGE_FACTS
    states, on an MI355X and on a device of one CU and of 304; the model's result is the reference's"""
    call, facts = cases.BY_NAME[name], cases.RANGE_FACTS[name]
    assert call.form == "chunked" and call.bound > range_sort_cases.ONE_WORKGROUP_MAX and 0 < call.bits[1] - call.bits[0] < 32
    keys, values, counts = _small_count_inputs(call)
    want = range_sort_cases.reference(keys, values, *call.bits, cases.sorted_count(call))
    for cus in CU_COUNTS:
        got_keys, got_values, info = range_sort_cases.sort_range_model(keys, values, *call.bits, cus, **counts)
        assert info["form"] == "chunked", (name, cus)
        assert (info["active"], info["copy_back"], info["scratch_written"]) == facts[:3], (name, cus, info["active"])
        assert info["chunks"] == min(cus, facts.most_chunks), (name, cus, info["chunks"])
        assert np.array_equal(got_keys, want[0]) and (values is None or np.array_equal(got_values, want[1])), (name, cus)
    # the full arrays give the reference the GPU test uses the same first elements
    full = cases.expected_of(call)
    assert np.array_equal(full[0][:len(keys)], want[0]) and (values is None or np.array_equal(full[1][:len(keys)], want[1]))
    if name == "range-equal-field":
        assert np.array_equal(want[0], keys)   # nothing moves


def test_the_range_rows_keep_random_bits_outside_their_field():
    for name in RANGE_ROWS + ["bits-one-workgroup", "segmented-bits"]:
        call = cases.BY_NAME[name]
        keys = cases.inputs_of(call)[0][:65536]
        begin, end = call.bits
        outside = keys & np.uint32(~(((1 << (end - begin)) - 1) << begin) & 0xFFFFFFFF)
        # (65536 draws from 2^b values leave more than half of them, or of the draws, distinct)
        assert len(np.unique(outside)) > min(1 << (32 - (end - begin)), len(keys)) // 2, name


def _clean_and_leavers():
    """every range row's model run on an MI355X: (inputs, clean result, info)"""
    out = {}
    for name in RANGE_ROWS:
        call = cases.BY_NAME[name]
        keys, values, counts = _small_count_inputs(call)
        out[name] = (keys, values, counts, range_sort_cases.sort_range_model(keys, values, *call.bits, MI355X_CUS, **counts))
    return out


def _differs(a, b, scratch=False):
    """keys or values differ; scratch: or one run writes the scratch arrays and the other does not (what the GPU test sees of
    range-equal-field, whose scratch must stay byte for byte what the leaver left)"""
    return (not np.array_equal(a[0], b[0]) or (a[1] is not None and not np.array_equal(a[1], b[1]))
            or (scratch and a[2]["scratch_written"] != b[2]["scratch_written"]))


def test_stale_storage_changes_what_every_range_row_gives():
    """The three clears the matrix newly covers, shown on the model: totals that are not zero (the word 1 in every bin, and the
    totals range-chunked-pairs-copy-back leaves), a mask that is not rewritten (every other mask a row of the table or an MSD
    sort's word 2 leaves), count rows of a longer sort (those range-chunked-pairs-copy-back leaves; for that row itself and
    for the rows of two chunks, rows of ones).  Each changes the result of every range row -- keys in other places, or keys
    that never arrive."""
    runs = _clean_and_leavers()
    leaver = runs["range-chunked-pairs-copy-back"][3][2]
    assert int(leaver["totals"][:3].sum()) == 3 * cases.RANGE_N and int(leaver["totals"][3].sum()) == 0
    assert leaver["counts"].shape == (8, 256)
    # (the masks of the table's rows; a fill of ones; an MSD plan's word: a window at bit 22, "turned down")
    masks = sorted({f.active for f in cases.RANGE_FACTS.values()} | {0xFFFFFFFF, 0x00001601})
    for name in RANGE_ROWS:
        call = cases.BY_NAME[name]
        keys, values, counts, clean = runs[name]

        def run(**stale):
            return range_sort_cases.sort_range_model(keys, values, *call.bits, MI355X_CUS, **counts, **stale)

        for what, totals in (("one per bin", 1), ("a leaver's", leaver["totals"])):
            # (equal fields: every key goes back to where it was, through the scratch arrays the row must not write)
            assert _differs(run(stale_totals=totals), clean, scratch=name == "range-equal-field"), (name, "stale totals", what)
        own = cases.RANGE_FACTS[name].active
        digits = range_sort_cases.digits_of(*call.bits)
        exposing = []
        for mask in masks:
            seen, mine = mask & 0xF, mask & ((1 << digits) - 1)
            if seen == own:
                continue
            changed = _differs(run(stale_mask=mask), clean, scratch=name == "range-equal-field")
            # A stale mask is harmless only when it adds passes to the row's own: a pass over a digit that is the same in
            # every key moves every key to where it was, in the other array -- unless that pass is pass 0, whose scan launch
            # has returned -- and bits above the row's digits must not change the parity the copy back goes by.
            harmless = (mine & own) == own and (mine & 1) == (own & 1) and bin(seen & ~mine).count("1") % 2 == 0
            assert changed != harmless, (name, "stale mask", hex(mask))
            exposing += [mask] if changed else []
        # ... and every row is exposed by the mask another row of the table leaves
        assert {f.active for f in cases.RANGE_FACTS.values()} & set(exposing), (name, exposing)
        rows = leaver["counts"] if name != "range-chunked-pairs-copy-back" else np.ones((8, 256), np.int64)
        if own != 0:   # (a field that is equal in every key launches nothing that reads the table)
            assert _differs(run(stale_counts=rows), clean), (name, "stale count rows")
    # the row whose field is equal reads no row of counts -- but stale totals or a stale mask make it move keys
    keys, values, counts, clean = runs["range-equal-field"]
    moved = range_sort_cases.sort_range_model(keys, values, 5, 14, MI355X_CUS, stale_mask=0b11)
    assert _differs(moved, clean) and moved[2]["scratch_written"]


@pytest.mark.parametrize("name,form", [("wide-one-workgroup", "one-workgroup"), ("wide-gather", "gather"),
                                       ("wide-two-sorts-indirect", "two-sorts")])
def test_the_wide_value_rows_have_the_form_in_their_name(name, form):
    call = cases.BY_NAME[name]
    assert call.form == form == wide_value_cases.form_of(call.bound, cases.WIDE_TWO_SORTS_N)
    # ... at the edge of it: the last bound of one workgroup, the first of the two-sorts form
    assert wide_value_cases.form_of(cases.WIDE_ONE_WORKGROUP_N + 1, cases.WIDE_TWO_SORTS_N) == "gather"
    assert wide_value_cases.form_of(cases.WIDE_TWO_SORTS_N - 1, cases.WIDE_TWO_SORTS_N) == "gather"
    assert call.bound in (cases.WIDE_ONE_WORKGROUP_N, cases.H, cases.WIDE_TWO_SORTS_N)
    if name == "wide-two-sorts-indirect":   # the model of the form on what the device sorts: the reference
        keys, values, _ = cases.inputs_of(call)
        cut = call.count + 16
        got = wide_value_cases.wide_value_model(keys[:cut], values[:cut], bound=cut, count=call.count, two_sorts_from=0)
        want = cases.expected_of(call)
        assert np.array_equal(got[0], want[0][:cut]) and np.array_equal(got[1], want[1][:cut])
        assert np.array_equal(want[0][cut:], keys[cut:]) and np.array_equal(want[1][cut:], values[cut:])


def test_the_ordered_rows_hold_the_special_values_of_their_key_type():
    for name, specials in (("ordered-msd", key_order32_cases.FLOAT_EDGES), ("ordered-segmented", key_order32_cases.FLOAT_EDGES),
                           ("ordered-small", key_order32_cases.INT_EDGES), ("sort64-ordered-pairs", key_order_cases.FLOAT_EDGES),
                           ("segmented64-ordered", key_order_cases.INT_EDGES)):
        call = cases.BY_NAME[name]
        keys = cases.inputs_of(call)[0]
        assert call.order is not None and cases.order_word(call) != 0
        assert np.isin(specials, keys).all(), name
    # ordered-msd: the specials are few enough for the plan to run on T(key), with the window at the top
    assert cases.verdict_of(cases.BY_NAME["ordered-msd"]) == (model.VERDICT_MSD_RUNS, 32 - cases.MSD_BITS)
    assert cases.verdict_of(cases.BY_NAME["wide-two-sorts-indirect"]) == (model.VERDICT_MSD_RUNS, 22)
    assert cases.verdict_of(cases.BY_NAME["wide-gather"]) == (model.VERDICT_HYBRID_RUNS, 3)
    assert cases.verdict_of(cases.BY_NAME["sort64-ordered-pairs"]) == (model.VERDICT_HYBRID_DECLINED, 3)
