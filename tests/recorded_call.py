"""One call of tests/storage_reuse_cases.py (or of a module with the same Call rows, as tests/in_flight_cases.py) on buffers
that outlive it: what the host records for it, its buffers and expected outputs on the device, the recording itself and the
checks of what it left -- shared by tests/test_storage_reuse_gpu.py (one call at a time, on the storage the call before left)
and tests/in_flight_battery.py (two calls at a time, each on a storage of its own).  A plain module next to guarded_call.py,
imported the same way; torch comes in as an argument, so the checks also run on host tensors.

The checks are handed out as data -- array_checks() lists (message, what the call left, what it must have left) -- so that one
caller compares with torch.equal after a synchronise and the other adds torch.ne(...).any() to a device counter in stream
order, under the same messages."""
from types import SimpleNamespace

import numpy as np

import storage_reuse_cases as cases
from guarded_call import to_device
from storage_reuse_cases import INHERITED
from test_plan_choice_gpu import expected_word
from test_range_sort_gpu import scratch_from
from vulkan_radix_sort_amd import api

OFFSETS = (0, 48)     # storageOffset: the layout moves with the low seven bits of the storage's address
FRONT = max(OFFSETS)
BAND = 256            # 0x5A behind the largest requirement
BEHIND = 4096         # bytes right behind a call's own requirement that it must leave alone
POISON, FRONT_BYTE, BAND_BYTE = 0xA5, 0x3C, 0x5A

ROWS = {row.c_name: row for row in api.RECORDING_CALLS + api.ORDERED_SORT_CALLS + api.WIDE_VALUE_CALLS
        + api.WIDE_VALUE_SEGMENTED_CALLS + api.RANGE_SORT_CALLS}


def family_plan(s, call, key_value):
    """The plan of a call of the newer families against the family's own describe call, before anything runs; returns the
    chunks of a chunked range sort (else None)."""
    if cases.is_segmented(call):
        return None
    if cases.is_range_sort(call):
        info = s.describe_range_sort_plan(call.bound, key_value, *call.bits)
        cus = int(s.describe_range_sort_plan(0x3FFFFFFC, False, 0, 8).chunks)   # (the device's CU count)
        assert (info.name, int(info.digits)) == (call.form, -(-(call.bits[1] - call.bits[0]) // 8)), (call.name, info.name)
        assert int(info.chunks) == min(cus, call.bound // 8192), (call.name, int(info.chunks))
        assert cus >= cases.RANGE_FACTS[call.name].most_chunks, cus   # (every chunk RANGE_FACTS counts on holds keys here)
        return int(info.chunks)
    if call.bits is not None:
        info = s.describe_sort_bits_plan(call.bound, key_value, *call.bits)
        assert info.name == call.form and int(info.launches) == 1, (call.name, info.name)
    elif cases.is_ordered32(call):
        info = s.describe_ordered_sort_plan(call.bound, key_value, cases.order_word(call))
        assert info.name == call.plan, (call.name, info.name)
        assert call.plan != "msd" or int(info.bits) == cases.msd_constants(call)[0], (call.name, int(info.bits))
    elif cases.has_wide_values(call):
        info = s.describe_wide_value_sort_plan(call.bound)
        assert info.name == call.form, (call.name, info.name)
        assert (int(info.oneWorkgroupMax), int(info.twoSortsFrom)) == (cases.WIDE_ONE_WORKGROUP_N, cases.WIDE_TWO_SORTS_N)
        assert call.form == "one-workgroup" or api.PLAN_NAMES[int(info.innerPlan)] == call.plan, (call.name, int(info.innerPlan))
    return None


def planned(s, call, msd_bits=None):
    """What the host records for the call is what its row assumes (msd_bits: the window's bits where the row's plan is the
    MSD plan, default those of storage_reuse_cases.M); returns (the call's storage requirement, the chunks of a chunked range
    sort or None)."""
    key_value, wide = cases.is_key_value(call), cases.is_wide(call)
    if call.plan is not None:
        info = s.describe_plan(call.bound, True if wide else key_value)
        assert info.name == call.plan, (call.name, info.name)
        assert call.plan != "msd" or int(info.bits) == (cases.MSD_BITS if msd_bits is None else msd_bits), (call.name, int(info.bits))
        assert call.plan != "msd" or int(info.bits) == cases.msd_constants(call)[0], (call.name, int(info.bits))
    chunks = family_plan(s, call, key_value)
    required = {"keys": lambda: s.storage_requirements(call.bound),
                "key-value": lambda: s.key_value_storage_requirements(call.bound),
                "keys64": lambda: s.storage_requirements64(call.bound, False),
                "key-value64": lambda: s.storage_requirements64(call.bound, True),
                "wide-value": lambda: s.wide_value_storage_requirements(call.bound)}[call.requirement]().size
    # (the wide-value requirement is the inner one plus 12 bytes per element plus 112 + 2 x 124: a multiple of 4 only)
    assert required % (4 if call.requirement == "wide-value" else 16) == 0
    return required, chunks


def device_call(torch, call, shared, required, chunks=None, source=cases, device="cuda"):
    """The call's inputs and expected outputs on the device (calls that share an input set share its pristine copy and its
    working buffers: `shared`, by the set's name), its count word and the words it must leave.  source: the module that holds
    the call's row -- its input_set, expected_of and verdict_of."""
    key_value = cases.is_key_value(call)
    if call.inputs not in shared:
        keys, values, offsets = source.input_set(call.inputs)
        pristine = SimpleNamespace(keys=to_device(torch, cases.padded(keys), device=device),
                                   values=to_device(torch, cases.padded(values), device=device) if values is not None else None,
                                   offsets=to_device(torch, offsets, device=device) if offsets is not None else None)
        shared[call.inputs] = SimpleNamespace(
            pristine=pristine, keys=pristine.keys.clone(),
            values=pristine.values.clone() if values is not None else None,
            offsets=pristine.offsets.clone() if offsets is not None else None, expected={})
    d = shared[call.inputs]
    which = (key_value, cases.sorted_count(call), call.bits, call.order, cases.is_segmented(call))
    if which not in d.expected:
        want_keys, want_values = source.expected_of(call)
        d.expected[which] = (to_device(torch, cases.padded(want_keys), device=device),
                             to_device(torch, cases.padded(want_values), device=device) if key_value else None)
    verdict, shift = source.verdict_of(call) if call.verdict != INHERITED else (INHERITED, None)
    assert verdict == call.verdict, (call.name, verdict)
    count = None
    if call.count is not None:
        count = to_device(torch, np.array([call.count, 0, 0, 0], np.uint32), device=device)
    return SimpleNamespace(
        buffers=d, key_value=key_value, expected_keys=d.expected[which][0], expected_values=d.expected[which][1],
        required=required, count=count, count_pristine=count.clone() if count is not None else None,
        bits=call.bits if call.bits is not None else (None, None), order=cases.order_word(call),
        scratch_from=scratch_from(chunks) if call.name == "range-equal-field" else None,
        plan_word=expected_word(verdict, shift) if cases.records_msd_plan(call) else None)


def record(s, stream, call, d, storage, off):
    """the row of RECORDING_CALLS, ORDERED_SORT_CALLS, WIDE_VALUE_CALLS, WIDE_VALUE_SEGMENTED_CALLS or RANGE_SORT_CALLS that
    `call.entry` names, on the world's buffers at byte offset 0"""
    b = d.buffers
    row = ROWS[call.entry]
    given = {"command_buffer": stream, "element_count": call.bound, "max_element_count": call.bound,
             "segment_count": len(b.offsets) - 1 if b.offsets is not None else None, "offsets": b.offsets, "indirect": d.count,
             "keys": b.keys, "values": b.values if d.key_value else None, "begin_bit": d.bits[0], "end_bit": d.bits[1],
             "order": d.order}
    given = {name: t.data_ptr() if hasattr(t, "data_ptr") else t for name, t in given.items()}
    given.update(storage=storage, storage_offset=off, offsets_offset=0, indirect_offset=0, keys_offset=0, values_offset=0)
    getattr(s, row.method)(*(given[name] for name, _ in row.parameters[:-2]))   # (no query pool)


def restore_inputs(d):
    """fresh copies of the keys and the values (the count word and the offsets must never change: they are not restored)"""
    b = d.buffers
    b.keys.copy_(b.pristine.keys)
    if b.values is not None:
        b.values.copy_(b.pristine.values)


def array_checks(d):
    """[(message, what the call left, what it must have left)]: keys and values bit for bit, the elements from the count on
    and the guard behind the arrays included; the values of a keys-only call, the count word and the offsets as they were"""
    b = d.buffers
    checks = [("keys differ", b.keys, d.expected_keys)]
    if d.key_value:
        checks.append(("values differ", b.values, d.expected_values))
    if b.values is not None and not d.key_value:
        checks.append(("a keys-only call wrote the values", b.values, b.pristine.values))
    if d.count is not None:
        checks.append(("the count word changed", d.count, d.count_pristine))
    if b.offsets is not None:
        checks.append(("the offsets changed", b.offsets, b.pristine.offsets))
    return checks


def header_problems(call, d, status, verdict, word, before=None, after=None):
    """The failure word, the verdict, and word 1 as a whole where the MSD plan is recorded.  before, after: the four header
    words in front of and behind an empty sort, which records nothing -- the header is the call before's.  word: a callable,
    asked only where the whole word is checked."""
    problems = []
    want_status, want_verdict = call.failure, call.verdict
    if call.verdict == INHERITED:
        want_status, want_verdict = int(before[3]), int(before[1]) & 0xFF
        if not np.array_equal(before, after):
            problems.append("an empty sort wrote the header")
    if status != want_status:
        problems.append(f"failure word {status:#x}, not {want_status:#x}")
    if verdict != want_verdict:
        problems.append(f"verdict {verdict}, not {want_verdict}")
    if d.plan_word is not None:
        word = word()
        if word != d.plan_word:
            problems.append(f"plan word {word:#x}, not {d.plan_word:#x}")
    return problems


def failure_left(call):
    """what the call adds to its sorter's sticky word"""
    return 0 if call.failure == INHERITED else call.failure
