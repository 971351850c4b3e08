"""What tests/test_storage_reuse_gpu.py (on the GPU) and tests/test_storage_reuse_cases.py (without one) share: CALLS, one
recorded call of every kind the library has, each with the inputs that send it down the path its name says and with what it
must leave in the storage header.  A plain module next to plan_model.py and segmented_cases.py, imported the same way; it
needs numpy only.

Every call is described by the C entry point it goes through, the sorter (one-atomic or ballot ranking), the bound the
host plans with, the device-side count of the indirect forms, the plan the host records for that bound
(vrdxHipDescribePlan) and the verdict and failure word the device must leave (vrdxHipReadPlanVerdict, vrdxHipReadStatus).
The verdicts are written down here as constants; verdict_of() restates them from tests/plan_model.py with the constants the
host uses at that bound, and tests/test_storage_reuse_cases.py asserts that the two agree, so a changed generator cannot
turn a "declined" call into an "accepted" one unnoticed.

References, bit for bit: np.argsort(kind="stable") of the first `count` keys (32- and 64-bit alike: the 64-bit keys are
compared as uint64), np.lexsort((keys, segment id)) through segmented_cases.expected() for the segmented forms.  Values are
random words, never the index.  The families with a case module of their own -- by a bit range, in a key order, with 8-byte
values, range sorts at every size -- take that module's reference (expected_of() says which); none is written again here.
Their keys come from that module's builders: bits outside a sorted range are random, the ordered rows hold the special
values of their key type, 8-byte values have random high words.
"""
import functools
from collections import namedtuple

import numpy as np

import key_order32_cases
import key_order_cases
import plan_model as model
import range_sort_cases
import segmented_bits_cases
import sort64_model
import sort_bits_cases
import wide_value_cases
import wide_value_segmented_cases
from plan_check_tool import ATOMIC_TABLE, table_row
from segmented_cases import expected as segmented_expected
from test_sort_gpu import ROUND, decline_msd, msd_capacity

M = 8_200_003     # the MSD plan: ten bits, half-size buckets (18432); M % 4 == 3
H = 300_001       # the hybrid plan, buckets of 4096
MSD_BITS = 10     # what MsdBits (vrdx_plan.h) records at M, at ROUND and at 2 ROUND + 1
TAIL_SPLIT_N = 2 * ROUND + 1   # the smallest size of test_tail_split_tiles_at_their_boundaries (keys-only)
BLOCK_SUMS_N = ROUND           # the smallest size of test_block_sums_in_sorts_of_one_round
SEGMENTED_N = 400_000
SEGMENT_SIZES = [300] * 60 + [5000] * 20 + [40000] * 4 + [0] * 16
INVALID_N = 50_000
INVALID_OFFSETS = [100, 1100, 21100, 9000, 9000, INVALID_N + 5000]   # of test_bad_offsets_leave_their_segments_alone_and_say_so
RANGE_N = 65_539                  # the chunked range sort: eight chunks of 8448 keys on a device of eight CUs and more
SMALL_COUNT = 20_001              # the device-side count of the indirect rows under a large bound: two short chunks
WIDE_ONE_WORKGROUP_N = wide_value_cases.ONE_WORKGROUP_MAX   # kWideSmallMaxElements
WIDE_TWO_SORTS_N = 1 << 24        # kWideValueTwoSortsFrom (vrdx_plan.h): the first bound of the two-sorts form

STATUS_SEGMENTS_INVALID = 0x00000004   # VRDX_HIP_STATUS_SEGMENTS_INVALID (include/vk_radix_sort.h)
NONE, HYBRID8_RUNS, HYBRID8_DECLINED, MSD_RUNS, MSD_SORTED = (
    model.VERDICT_NONE, model.VERDICT_HYBRID_RUNS, model.VERDICT_HYBRID_DECLINED, model.VERDICT_MSD_RUNS,
    model.VERDICT_MSD_SORTED)
INHERITED = "inherited"   # the `empty` call: the header words are those of the call before

GUARD_ELEMENTS = 8192     # behind every caller array, in the pristine and in the expected copy alike (more than the 5000
                          # elements by which the invalid offsets end behind their bound)
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

# name: what failure messages call it.  sorter: "atomic" | "ballot".  entry: the C entry point.  requirement: the calculator
# the storage of this call is sized with ("keys" | "key-value" | "keys64" | "key-value64"), for `bound` elements.
# count: the device-side count of an indirect form, else None.  plan: vrdxHipDescribePlan(bound, key_value).name for the
# 32-bit sorts, the inner sorts' plan for the 64-bit ones, None for the segmented forms and the empty call.
# inputs: the input set (input_set()).  verdict, failure: what the call must leave.
# The families behind the first 21 rows add: bits, (beginBit, endBit) of the calls by a bit range; order, (key type,
# descending) of the ordered calls; form, the name the family's own describe call gives for the bound
# (vrdxHipDescribeRangeSortPlan, vrdxHipDescribeSortBitsPlan, vrdxHipDescribeWideValueSortPlan; the ordered calls: `plan`
# through vrdxHipDescribeOrderedSortPlan); the requirement "wide-value" (wide_value_storage_requirements), whose calls take
# values of 8 bytes.  plan: for the wide-value calls the inner sorts' plan, like the 64-bit ones.
Call = namedtuple("Call", "name sorter entry requirement bound count plan inputs verdict failure bits order form",
                  defaults=(None, None, None))
FLOAT32_DESCENDING, INT32_ASCENDING = ("float32", True), ("int32", False)
FLOAT64_DESCENDING, INT64_ASCENDING = ("float64", True), ("int64", False)

CALLS = [
    Call("msd-runs-keys", "atomic", "vrdxCmdSort", "keys", M, None, "msd", "uniform-M", MSD_RUNS, 0),
    Call("msd-runs-pairs", "atomic", "vrdxCmdSortKeyValue", "key-value", M, None, "msd", "uniform-M", MSD_RUNS, 0),
    Call("msd-declined-keys", "atomic", "vrdxCmdSort", "keys", M, None, "msd", "declined-M", NONE, 0),
    Call("msd-declined-pairs-skips", "atomic", "vrdxCmdSortKeyValue", "key-value", M, None, "msd", "skips-M", NONE, 0),
    Call("msd-all-equal", "atomic", "vrdxCmdSort", "keys", M, None, "msd", "all-equal-M", MSD_SORTED, 0),
    Call("msd-indirect-small", "atomic", "vrdxCmdSortKeyValueIndirect", "key-value", M, 20_001, "msd", "uniform-M", MSD_RUNS, 0),
    Call("msd-indirect-declined", "atomic", "vrdxCmdSortIndirect", "keys", M, M - 3, "msd", "declined-M", NONE, 0),
    Call("tail-split", "atomic", "vrdxCmdSort", "keys", TAIL_SPLIT_N, None, "msd", "tail-split", NONE, 0),
    Call("block-sums", "atomic", "vrdxCmdSort", "keys", BLOCK_SUMS_N, None, "msd", "block-sums", NONE, 0),
    Call("hybrid-runs", "atomic", "vrdxCmdSortKeyValue", "key-value", H, None, "hybrid-8", "uniform-H", HYBRID8_RUNS, 0),
    Call("hybrid-declined", "atomic", "vrdxCmdSort", "keys", H, None, "hybrid-8", "heavy-H", HYBRID8_DECLINED, 0),
    Call("one-workgroup", "atomic", "vrdxCmdSortKeyValue", "key-value", 16_384, None, "one-workgroup", "8-bit", NONE, 0),
    Call("ballot-four-passes", "ballot", "vrdxCmdSortKeyValue", "key-value", M, None, "four-passes", "uniform-M", NONE, 0),
    Call("ballot-hybrid", "ballot", "vrdxCmdSort", "keys", H, None, "hybrid-8", "uniform-H", HYBRID8_RUNS, 0),
    Call("segmented", "atomic", "vrdxHipCmdSortSegmentedKeyValue", "key-value", SEGMENTED_N, None, None, "segments", NONE, 0),
    Call("segmented-invalid", "atomic", "vrdxHipCmdSortSegmented", "keys", INVALID_N, None, None, "bad-segments", NONE,
         STATUS_SEGMENTS_INVALID),
    Call("segmented64", "atomic", "vrdxHipCmdSortSegmented64", "keys64", SEGMENTED_N, None, None, "segments64", NONE, 0),
    Call("sort64-pairs", "atomic", "vrdxHipCmdSort64KeyValue", "key-value64", H, None, "hybrid-8", "uniform63-H", HYBRID8_RUNS, 0),
    Call("sort64-indirect", "atomic", "vrdxHipCmdSort64Indirect", "keys64", H, H // 2, "hybrid-8", "tile-depth-H", HYBRID8_RUNS, 0),
    Call("sort64-small", "atomic", "vrdxHipCmdSort64KeyValue", "key-value64", 5_000, None, "one-workgroup", "uniform64-small",
         NONE, 0),
    Call("empty", "atomic", "vrdxCmdSort", "keys", 0, None, None, "nothing", INHERITED, INHERITED),
    # the chunked range sort (RANGE_FACTS: its mask, copy back, scratch and chunks)
    Call("range-chunked-keys", "atomic", "vrdxHipCmdRangeSort", "keys", RANGE_N, None, None, "range-uniform-5-14", NONE, 0,
         bits=(5, 14), form="chunked"),
    Call("range-chunked-pairs-copy-back", "atomic", "vrdxHipCmdRangeSortKeyValue", "key-value", RANGE_N, None, None,
         "range-uniform-4-28", NONE, 0, bits=(4, 28), form="chunked"),
    Call("range-gap-in-mask", "atomic", "vrdxHipCmdRangeSortKeyValue", "key-value", RANGE_N, None, None, "range-const-mid-4-28",
         NONE, 0, bits=(4, 28), form="chunked"),
    Call("range-equal-field", "atomic", "vrdxHipCmdRangeSort", "keys", RANGE_N, None, None, "range-equal-5-14", NONE, 0,
         bits=(5, 14), form="chunked"),
    Call("range-indirect-small", "atomic", "vrdxHipCmdRangeSortKeyValueIndirect", "key-value", M, SMALL_COUNT, None, "uniform-M",
         NONE, 0, bits=(4, 28), form="chunked"),
    Call("range-ballot", "ballot", "vrdxHipCmdRangeSort", "keys", RANGE_N, None, None, "range-uniform-8-24", NONE, 0,
         bits=(8, 24), form="chunked"),
    # by a bit range in one workgroup, and segment by segment
    Call("bits-one-workgroup", "atomic", "vrdxHipCmdSortBitsKeyValue", "key-value", 16_384, None, None, "bits-uniform-8-16",
         NONE, 0, bits=(8, 16), form="one-workgroup"),
    Call("segmented-bits", "atomic", "vrdxHipCmdSortSegmentedBitsKeyValue", "key-value", SEGMENTED_N, None, None, "segments",
         NONE, 0, bits=(5, 22)),
    # in a key order: the transform steps around the MSD plan, one workgroup, the segmented kernels, the 64-bit compositions
    Call("ordered-msd", "atomic", "vrdxHipCmdOrderedSortKeyValue", "key-value", M, None, "msd", "float-specials-M", MSD_RUNS, 0,
         order=FLOAT32_DESCENDING),
    Call("ordered-small", "atomic", "vrdxHipCmdOrderedSort", "keys", 5_000, None, "one-workgroup", "mixed-int-small", NONE, 0,
         order=INT32_ASCENDING),
    Call("ordered-segmented", "atomic", "vrdxHipCmdOrderedSortSegmentedKeyValue", "key-value", SEGMENTED_N, None, None,
         "float-segments", NONE, 0, order=FLOAT32_DESCENDING),
    Call("sort64-ordered-pairs", "atomic", "vrdxHipCmdSort64OrderedKeyValue", "key-value64", H, None, "hybrid-8",
         "float64-specials-H", HYBRID8_DECLINED, 0, order=FLOAT64_DESCENDING),
    Call("segmented64-ordered", "atomic", "vrdxHipCmdSortSegmented64Ordered", "keys64", SEGMENTED_N, None, None,
         "int64-segments", NONE, 0, order=INT64_ASCENDING),
    # 32-bit keys with 8-byte values: the three flat forms and the segmented one
    Call("wide-one-workgroup", "atomic", "vrdxHipCmdWideValueSort", "wide-value", WIDE_ONE_WORKGROUP_N, None, "one-workgroup",
         "wide-small", NONE, 0, form="one-workgroup"),
    Call("wide-gather", "atomic", "vrdxHipCmdWideValueSort", "wide-value", H, None, "hybrid-8", "wide-H", HYBRID8_RUNS, 0,
         form="gather"),
    Call("wide-two-sorts-indirect", "atomic", "vrdxHipCmdWideValueSortIndirect", "wide-value", WIDE_TWO_SORTS_N, SMALL_COUNT,
         "msd", "wide-two-sorts", MSD_RUNS, 0, form="two-sorts"),
    Call("wide-segmented", "atomic", "vrdxHipCmdWideValueSortSegmented", "wide-value", SEGMENTED_N, None, None, "wide-segments",
         NONE, 0),
]
FIRST_CALLS = 21   # the rows above the range sorts: the table as it stood before the families behind them existed
NAMES = [c.name for c in CALLS]
BY_NAME = {c.name: c for c in CALLS}

# what the chunked range sorts must decide on the device, as range_sort_cases.sort_range_model restates it: the mask of active
# passes (header word 2), whether the copy back copies, whether a pass writes the scratch arrays, and the chunks that hold keys
# on a device of `cus` CUs -- min(cus, most)
RangeFacts = namedtuple("RangeFacts", "active copy_back scratch_written most_chunks")
RANGE_FACTS = {
    "range-chunked-keys": RangeFacts(0b11, False, True, 8),
    "range-chunked-pairs-copy-back": RangeFacts(0b111, True, True, 8),
    "range-gap-in-mask": RangeFacts(0b101, False, True, 8),
    "range-equal-field": RangeFacts(0, False, False, 8),
    "range-indirect-small": RangeFacts(0b111, True, True, 2),
    "range-ballot": RangeFacts(0b11, False, True, 8),
}


def is_segmented(call):
    return "Segmented" in call.entry


def has_wide_values(call):
    """values of 8 bytes"""
    return call.entry.startswith("vrdxHipCmdWideValueSort")


def is_key_value(call):
    return "KeyValue" in call.entry or has_wide_values(call)


def is_wide(call):
    """uint64 keys"""
    return "64" in call.entry


def is_range_sort(call):
    return call.entry.startswith("vrdxHipCmdRangeSort")


def is_ordered32(call):
    return call.entry.startswith("vrdxHipCmdOrderedSort")


def order_word(call):
    """the order word of an ordered call (include/vk_radix_sort.h), else None"""
    if call.order is None:
        return None
    return (key_order_cases if is_wide(call) else key_order32_cases).order_word(*call.order)


def sorted_count(call):
    """how many elements the call sorts: the device-side count of an indirect form, else the bound"""
    return call.bound if call.count is None else call.count


def records_msd_plan(call):
    """a 32-bit sort in front of whose passes the host records the MSD plan (the inner sorts of a wide-value call are such
    sorts): word 1 of the storage is checked as a whole"""
    return call.plan == "msd" and not is_wide(call)


def msd_constants(call):
    """(bits, bucket capacity) of the MSD plan at the call's bound, from the table of plan edges tests/test_plan_check.py
    holds to the planner (the GPU test compares the bits with describe_plan's)"""
    name, bits, _, cap, _ = table_row(ATOMIC_TABLE, call.bound)
    assert name == "msd" and cap == msd_capacity(call.bound, bits), (call.name, name, bits, cap)
    return bits, cap


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def _words(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def segment_offsets(sizes, head, seed):
    sizes = list(sizes)
    np.random.default_rng(seed).shuffle(sizes)
    return (head + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def input_set(name):
    """(keys, values, offsets) of one input set, read-only: calls that share a set share its arrays.  values: random words
    for every set a key+value call uses; offsets: the segmented sets only."""
    values = offsets = None
    if name == "uniform-M":
        keys, values = _words(M, 11), _words(M, 12)
    elif name == "declined-M":
        keys = decline_msd(_words(M, 21))
    elif name == "skips-M":   # bytes 1 and 2 constant: two of the four passes move nothing
        keys, values = (_words(M, 31) & np.uint32(0xFF0000FF)) | np.uint32(0x00A5C300), _words(M, 32)
    elif name == "all-equal-M":
        keys = np.full(M, 0x9E3779B9, np.uint32)
    elif name == "tail-split":
        keys = decline_msd(_words(TAIL_SPLIT_N, 41))
    elif name == "block-sums":
        # one value of the top eleven bits 40000 times, as test_block_sums_in_sorts_of_one_round plants it
        keys = _words(BLOCK_SUMS_N, 51)
        step = max(1, BLOCK_SUMS_N // 40000)
        keys[::step][:40000] = (keys[::step][:40000] & np.uint32(0x001FFFFF)) | np.uint32(0x0AB << 23)
    elif name == "uniform-H":
        keys, values = _words(H, 61), _words(H, 62)
    elif name == "heavy-H":
        # one top byte at capacity + 1, as test_hybrid_plan_and_its_fallback_at_the_bucket_capacity builds it
        rng = np.random.default_rng(71)
        heavy = model.hybrid_capacity(H) + 1
        keys = rng.integers(0, 1 << 32, size=H, dtype=np.uint64).astype(np.uint32)
        keys[(keys >> 24) == 0x5A] ^= np.uint32(0x01000000)
        where = rng.choice(H, size=heavy, replace=False)
        keys[where] = (keys[where] & np.uint32(0x00FFFFFF)) | np.uint32(0x5A000000)
    elif name == "8-bit":
        keys, values = _words(16_384, 81) >> np.uint32(24), _words(16_384, 82)
    elif name == "segments":
        keys, values = _words(SEGMENTED_N, 91), _words(SEGMENTED_N, 92)
        offsets = segment_offsets(SEGMENT_SIZES, 100, 93)
    elif name == "bad-segments":
        keys, offsets = _words(INVALID_N, 101), np.array(INVALID_OFFSETS, np.uint32)
    elif name == "segments64":
        keys = np.random.default_rng(111).integers(0, 1 << 64, size=SEGMENTED_N, dtype=np.uint64)
        offsets = segment_offsets(SEGMENT_SIZES, 100, 113)
    elif name == "uniform63-H":
        keys, values = np.random.default_rng(121).integers(0, 1 << 63, size=H, dtype=np.uint64), _words(H, 122)
    elif name == "tile-depth-H":   # tile id << 32 | the bits of a positive float depth
        keys = sort64_model.make_keys64("tile-depth", H, np.random.default_rng(131))
    elif name == "uniform64-small":
        keys, values = np.random.default_rng(141).integers(0, 1 << 64, size=5_000, dtype=np.uint64), _words(5_000, 142)
    elif name == "nothing":
        keys = np.zeros(0, np.uint32)
    elif name.startswith("range-"):   # range-<builder>-<begin>-<end>: range_sort_cases' builders, random bits outside the field
        *builder, begin, end = name[len("range-"):].split("-")
        keys = range_sort_cases.make_keys("-".join(builder), RANGE_N, int(begin), int(end), np.random.default_rng(201))
        values = _words(RANGE_N, 202)
    elif name == "bits-uniform-8-16":
        keys, values = sort_bits_cases.make_keys("uniform", 16_384, 8, 16, np.random.default_rng(211)), _words(16_384, 212)
    elif name == "float-specials-M":
        # the keys and values of uniform-M with every float32 special value planted a few hundred times: few enough that no
        # bucket of T(key) outgrows the MSD plan's capacity
        keys, values = input_set("uniform-M")[0].copy(), input_set("uniform-M")[1]
        keys[::1021] = np.resize(key_order32_cases.FLOAT_EDGES, len(keys[::1021]))
    elif name == "mixed-int-small":
        keys = key_order32_cases.make_keys("mixed-int", 5_000, np.random.default_rng(221), *INT32_ASCENDING)
    elif name == "float-segments":
        keys = key_order32_cases.make_keys("float-specials", SEGMENTED_N, np.random.default_rng(231), *FLOAT32_DESCENDING)
        values, offsets = _words(SEGMENTED_N, 232), segment_offsets(SEGMENT_SIZES, 100, 233)
    elif name == "float64-specials-H":
        keys = key_order_cases.make_keys("float-specials", H, np.random.default_rng(241), *FLOAT64_DESCENDING)
        values = _words(H, 242)
    elif name == "int64-segments":
        keys = key_order_cases.make_keys("mixed-int", SEGMENTED_N, np.random.default_rng(251), *INT64_ASCENDING)
        offsets = segment_offsets(SEGMENT_SIZES, 100, 253)
    elif name == "wide-small":
        rng = np.random.default_rng(261)
        keys = wide_value_cases.make_keys("uniform", WIDE_ONE_WORKGROUP_N, rng)
        values = wide_value_cases.make_values(WIDE_ONE_WORKGROUP_N, rng)
    elif name == "wide-H":
        rng = np.random.default_rng(271)
        keys, values = wide_value_cases.make_keys("uniform", H, rng), wide_value_cases.make_values(H, rng)
    elif name == "wide-two-sorts":
        rng = np.random.default_rng(281)
        keys = wide_value_cases.make_keys("uniform", WIDE_TWO_SORTS_N, rng)
        values = wide_value_cases.make_values(WIDE_TWO_SORTS_N, rng)
    elif name == "wide-segments":
        rng = np.random.default_rng(291)
        keys = wide_value_segmented_cases.make_keys("random", SEGMENTED_N, rng)
        values, offsets = wide_value_segmented_cases.make_values(SEGMENTED_N, rng), segment_offsets(SEGMENT_SIZES, 100, 293)
    else:
        raise ValueError(name)
    for a in (keys, values, offsets):
        if a is not None:
            a.setflags(write=False)
    return keys, values, offsets


def inputs_of(call):
    """(keys, values, offsets) as the call gets them: values only for the key+value forms"""
    keys, values, offsets = input_set(call.inputs)
    if is_key_value(call):
        assert values is not None, call.name
    else:
        values = None
    return keys, values, offsets


@functools.lru_cache(maxsize=None)
def _stable_order(inputs, n):
    """np.argsort(kind="stable") of the first n keys of an input set, once for every call that sorts them"""
    return np.argsort(input_set(inputs)[0][:n], kind="stable")


def expected_of(call):
    """(keys, values) of the WHOLE arrays after the call: the first sorted_count() elements stably sorted (the segmented
    forms: every valid segment on its own), everything behind them as it was."""
    keys, values, offsets = inputs_of(call)
    n = sorted_count(call)
    if call.entry == "vrdxHipCmdWideValueSortSegmented":
        return wide_value_segmented_cases.expected(keys, values, offsets, call.bound)
    if has_wide_values(call):
        return wide_value_cases.expected(keys, values, n)
    if call.order is not None:
        cases = key_order_cases if is_wide(call) else key_order32_cases
        if is_segmented(call):
            return cases.expected_segments(keys, values, offsets, call.bound, *call.order)
        return cases.expected(keys, values, *call.order, count=n)
    if call.bits is not None:
        if is_segmented(call):
            return segmented_bits_cases.expected(keys, values, offsets, call.bound, *call.bits)
        return sort_bits_cases.reference(keys, values, *call.bits, n)   # (range_sort_cases.reference is this function)
    if is_segmented(call):
        return segmented_expected(keys, values, offsets, call.bound)
    want_keys, want_values = keys.copy(), (values.copy() if values is not None else None)
    if values is None:
        want_keys[:n] = np.sort(keys[:n])
    else:
        order = _stable_order(call.inputs, n)
        want_keys[:n], want_values[:n] = keys[:n][order], values[:n][order]
    return want_keys, want_values


def padded(a):
    """the array with GUARD_ELEMENTS guard elements behind it (what lies on the device, pristine and expected alike)"""
    guard = np.full(GUARD_ELEMENTS, GUARD64 if a.dtype == np.uint64 else GUARD32, a.dtype)
    return np.concatenate([a, guard])


# ---- what the device must decide ---------------------------------------------------------------------------------------------

def ballot_hybrid_capacity(n):
    """HybridCapacity (vrdx_plan.h; pinned by tests/test_plan_check.py) for the ballot ranking: as plan_model.hybrid_capacity, but the largest bucket is 16384
    (the ballot forms of the 32768-element bucket kernel would spill); 0 = no hybrid plan.  That sorter never records the
    MSD plan (MsdBits), so beyond the hybrid plan its sorts are the four passes alone."""
    mean = -(-n // 256)
    for cap in (4096, 8192, 16384):
        if mean * 200 // 100 <= cap:
            return cap
    return 16384 if mean * 103 // 100 <= 16384 else 0


def verdict_of(call):
    """(verdict, shift | byte | None) by plan_model's rules with the constants the host uses at the call's bound, on the keys
    the device meets; the 64-bit sorts report their second inner sort, a key+value sort of the high words in the order the
    first one left them.  The ordered calls sort T(key): the model sees those words.  A wide-value call reports the last
    inner sort it records -- of the caller's keys, with the index or with the values' high words -- and no inner sort in
    one workgroup.  The range sorts over part of the key, the sorts by a bit range and the segmented forms record no plan."""
    keys, _, _ = inputs_of(call)
    n = sorted_count(call)
    if call.plan is None or call.plan in ("one-workgroup", "four-passes"):
        return NONE, None
    if call.order is not None:
        keys = (key_order_cases if is_wide(call) else key_order32_cases).T(keys, *call.order)
    if is_wide(call):
        keys = sort64_model.second_sort_keys(keys[:n])
    if call.plan == "msd":
        assert call.sorter == "atomic"
        bits, cap = msd_constants(call)
        assert call.bound != M or bits == MSD_BITS
        return model.msd_verdict(keys, n, bits, cap)
    assert call.plan == "hybrid-8"
    cap = model.hybrid_capacity(call.bound) if call.sorter == "atomic" else ballot_hybrid_capacity(call.bound)
    assert cap != 0
    return model.hybrid_verdict(keys, n, cap)
