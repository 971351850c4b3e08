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
random words, never the index.
"""
import functools
from collections import namedtuple

import numpy as np

import plan_model as model
import sort64_model
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
Call = namedtuple("Call", "name sorter entry requirement bound count plan inputs verdict failure")

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
]
NAMES = [c.name for c in CALLS]
BY_NAME = {c.name: c for c in CALLS}

SEGMENTED_ENTRIES = ("vrdxHipCmdSortSegmented", "vrdxHipCmdSortSegmentedKeyValue", "vrdxHipCmdSortSegmented64")
KEY_VALUE_ENTRIES = ("vrdxCmdSortKeyValue", "vrdxCmdSortKeyValueIndirect", "vrdxHipCmdSortSegmentedKeyValue",
                     "vrdxHipCmdSort64KeyValue")
WIDE_ENTRIES = ("vrdxHipCmdSortSegmented64", "vrdxHipCmdSort64KeyValue", "vrdxHipCmdSort64Indirect")


def is_segmented(call):
    return call.entry in SEGMENTED_ENTRIES


def is_key_value(call):
    return call.entry in KEY_VALUE_ENTRIES


def is_wide(call):
    """uint64 keys"""
    return call.entry in WIDE_ENTRIES


def sorted_count(call):
    """how many elements the call sorts: the device-side count of an indirect form, else the bound"""
    return call.bound if call.count is None else call.count


def records_msd_plan(call):
    """a 32-bit sort in front of whose passes the host records the MSD plan: word 1 of the storage is checked as a whole"""
    return call.plan == "msd" and not is_wide(call)


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
    if is_segmented(call):
        return segmented_expected(keys, values, offsets, call.bound)
    n = sorted_count(call)
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
    first one left them."""
    keys, _, _ = inputs_of(call)
    n = sorted_count(call)
    if call.plan is None or call.plan in ("one-workgroup", "four-passes"):
        return NONE, None
    if is_wide(call):
        keys = sort64_model.second_sort_keys(keys[:n])
    if call.plan == "msd":
        assert call.sorter == "atomic"
        return model.msd_verdict(keys, n, MSD_BITS, msd_capacity(call.bound, MSD_BITS))
    assert call.plan == "hybrid-8"
    cap = model.hybrid_capacity(call.bound) if call.sorter == "atomic" else ballot_hybrid_capacity(call.bound)
    assert cap != 0
    return model.hybrid_verdict(keys, n, cap)
