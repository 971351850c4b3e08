"""tests/guarded_call.py on the CPU, against a sorter that works on host memory and can be told to misbehave.

Every row of RECORDING_CALLS: a correct fake passes `guarded_call` and the arrays come back as the reference has them, which
shows that the harness reaches all rows with their arguments in the right order.  Every fault of FAULTS: the same call on a
fake that commits it must fail with a message that names the region.  The fake sorts with numpy -- the first count elements,
every segment, by the bit range, in the order word's order -- through the addresses it is handed."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import key_order_cases
import segmented_bits_cases
import segmented_cases
import sort_bits_cases
from guarded_call import BAND, TAIL, guarded_call
from vulkan_radix_sort_amd import api

N_BUF, COUNT, DEVICE_COUNT = 40, 37, 29            # the buffer is longer than the count, the bound larger than the device's count
OFFSETS = [2, 9, 20, 31]                           # three segments, elements in front of and behind them
BIT_RANGE, ORDER = (3, 12), key_order_cases.order_word("float64", descending=True)
WHERE = dict(keys_off=8, values_off=4, storage_off=48)
HEADER = 16                                        # the fake's storage: four words, the failure word the last of them


def _bytes(address, count):
    return np.ctypeslib.as_array((ctypes.c_uint8 * count).from_address(address))


# (name, what the message must say, the rows it applies to by their facts, where the fake writes one byte)
FAULTS = (
    ("front of keys", "in front of the keys", lambda f: True, lambda a: a.keys - 1),
    ("behind keys", "behind the keys", lambda f: True, lambda a: a.keys + a.key_bytes),
    ("end of keys' guard", "behind the keys", lambda f: True, lambda a: a.keys + a.key_bytes + TAIL - 1),
    ("front of values", "in front of the values", lambda f: f[3], lambda a: a.values - 1),
    ("behind values", "behind the values", lambda f: f[3], lambda a: a.values + 4 * N_BUF),
    ("end of values' guard", "behind the values", lambda f: f[3], lambda a: a.values + 4 * N_BUF + TAIL - 1),
    ("count word", "the count word changed", lambda f: f[2], lambda a: a.indirect),
    ("next to count word", "behind the count word", lambda f: f[2], lambda a: a.indirect + 4),
    ("one offset", "the offsets changed", lambda f: f[1], lambda a: a.offsets + 4),
    ("front of storage", "in front of the storage offset", lambda f: True, lambda a: a.storage - 1),
    ("behind requirement", "behind the storage requirement", lambda f: True, lambda a: a.storage + a.required),
    ("end of band", "behind the storage requirement", lambda f: True, lambda a: a.storage + a.required + BAND - 1),
)
# ... and two that are no stray byte: a failure word under expect_status=0, a storage byte written under expect_refused


class FakeSorter:
    """The cmd_* methods of every row, on host memory.  fault: a row of FAULTS, whose byte is written after the sort;
    status: the failure word it leaves; refuse: records nothing and raises STATUS_ENQUEUE_REFUSED (touch: ... and writes one
    byte of the storage all the same)."""

    def __init__(self, fault=None, status=0, refuse=False, touch=False):
        self.fault, self.status, self.refuse, self.touch, self.sticky = fault, status, refuse, touch, 0

    def _requirement(self, n, key_bytes, key_value):
        req = api.VrdxSorterStorageRequirements()
        req.size, req.usage = HEADER + (2 * key_bytes + (8 if key_value else 0)) * n, api.STORAGE_USAGE
        return req

    def storage_requirements(self, n):
        return self._requirement(n, 4, False)

    def key_value_storage_requirements(self, n):
        return self._requirement(n, 4, True)

    def storage_requirements64(self, n, key_value=False):
        return self._requirement(n, 8, key_value)

    def read_status(self, stream, storage, storage_offset=0):
        return int(_bytes(storage + storage_offset, HEADER).view(np.uint32)[3])

    def read_sorter_status(self, stream):
        status, self.sticky = self.sticky, 0
        return status

    def record(self, call, command_buffer, storage, storage_offset, query_pool, query, keys, keys_offset, element_count=None,
               max_element_count=None, segment_count=None, offsets=None, offsets_offset=None, indirect=None,
               indirect_offset=None, values=None, values_offset=None, begin_bit=None, end_bit=None, order=None):
        key_bits, segmented, is_indirect, key_value, extra = call.facts
        assert command_buffer == 0 and query_pool is None and query == 0
        assert (values is not None) == key_value and (offsets is not None) == segmented and (indirect is not None) == is_indirect
        bound = max_element_count if segmented or is_indirect else element_count
        a = SimpleNamespace()
        a.keys, a.key_bytes, a.storage = keys + keys_offset, N_BUF * key_bits // 8, storage + storage_offset
        a.values = values + values_offset if key_value else None
        a.offsets = offsets + offsets_offset if segmented else None
        a.indirect = indirect + indirect_offset if is_indirect else None
        a.required = self._requirement(bound, key_bits // 8, key_value).size
        if self.refuse:
            self.sticky |= api.STATUS_ENQUEUE_REFUSED
            if self.touch:
                _bytes(a.storage + a.required // 2, 1)[0] ^= 0xFF
            return
        k = _bytes(a.keys, a.key_bytes).view(np.uint32 if key_bits == 32 else np.uint64)
        v = _bytes(a.values, 4 * N_BUF).view(np.uint32) if key_value else None
        n = min(bound, int(_bytes(a.indirect, 4).view(np.uint32)[0])) if is_indirect else bound
        o = _bytes(a.offsets, 4 * (segment_count + 1)).view(np.uint32).copy() if segmented else None
        word = (ORDERS[order & 0xFF], bool(order & api.ORDER_DESCENDING)) if extra == "Ordered" else None
        if segmented:
            sorted_k, sorted_v = {None: lambda: segmented_cases.expected(k, v, o, bound),
                                  "Bits": lambda: segmented_bits_cases.expected(k, v, o, bound, begin_bit, end_bit),
                                  "Ordered": lambda: key_order_cases.expected_segments(k, v, o, bound, *word)}[extra]()
        else:
            sorted_k, sorted_v = {None: lambda: _sorted_prefix(k, v, n),
                                  "Bits": lambda: sort_bits_cases.reference(k, v, begin_bit, end_bit, n),
                                  "Ordered": lambda: key_order_cases.expected(k, v, *word, count=n)}[extra]()
        k[:] = sorted_k
        if key_value:
            v[:] = sorted_v
        scratch = _bytes(a.storage, a.required)
        scratch[:] = 0x11                         # the requirement is the sorter's to write
        scratch[:HEADER].view(np.uint32)[:] = [n, 0, 0, self.status]
        self.sticky |= self.status
        if self.fault is not None:
            _bytes(self.fault[3](a), 1)[0] ^= 0xFF


ORDERS = key_order_cases.ORDERS


def _sorted_prefix(keys, values, n):
    order = np.argsort(keys[:n], kind="stable")
    out_k, out_v = keys.copy(), (values.copy() if values is not None else None)
    out_k[:n] = keys[:n][order]
    if values is not None:
        out_v[:n] = values[:n][order]
    return out_k, out_v


def _method(call):
    names = [name for name, _ in call.parameters]

    def method(self, *args):
        assert len(args) == len(names), (call.method, len(args))
        self.record(call, **dict(zip(names, args)))
    return method


for _call in api.RECORDING_CALLS:
    setattr(FakeSorter, _call.method, _method(_call))


def _inputs(call):
    """what guarded_call is handed for this row, and the arrays it must return"""
    key_bits, segmented, indirect, key_value, extra = call.facts
    rng = np.random.default_rng(key_bits + 2 * segmented + 4 * indirect + 8 * key_value)
    keys = rng.integers(0, 1 << 16, size=N_BUF, dtype=np.uint64)   # (ties; for the bit range, random bits around the field)
    if key_bits == 64:
        keys = keys | (keys << np.uint64(47))
    else:
        keys = (keys * np.uint64(0x00010201) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    values = sort_bits_cases.payload(N_BUF) if key_value else None
    kw = dict(WHERE, count=COUNT)
    if segmented:
        kw.update(offsets=np.array(OFFSETS, np.uint32), offsets_off=12)
    if indirect:
        kw.update(device_count=DEVICE_COUNT, indirect_off=4)
    n = DEVICE_COUNT if indirect else COUNT
    order = ("float64", True)
    if extra == "Bits":
        kw.update(bit_range=BIT_RANGE)
        want = (segmented_bits_cases.expected(keys, values, OFFSETS, COUNT, *BIT_RANGE) if segmented
                else sort_bits_cases.reference(keys, values, *BIT_RANGE, n))
    elif extra == "Ordered":
        kw.update(order=ORDER)
        want = (key_order_cases.expected_segments(keys, values, OFFSETS, COUNT, *order) if segmented
                else key_order_cases.expected(keys, values, *order, count=n))
    else:
        want = segmented_cases.expected(keys, values, OFFSETS, COUNT) if segmented else _sorted_prefix(keys, values, n)
    return keys, values, kw, want


def _run(call, fake, **more):
    keys, values, kw, want = _inputs(call)
    got = guarded_call(torch, fake, keys, values, device="cpu", **dict(kw, **more))
    return got, want


ROW_IDS = [call.c_name for call in api.RECORDING_CALLS]


@pytest.mark.parametrize("call", api.RECORDING_CALLS, ids=ROW_IDS)
def test_every_row_passes_and_returns_the_reference(call):
    fake = FakeSorter()
    got, want = _run(call, fake, sticky=0, keep_before=True)
    assert np.array_equal(got.keys, want[0]) and not np.array_equal(got.keys[:COUNT], _inputs(call)[0][:COUNT])
    assert (got.values is None) == (want[1] is None) and (got.values is None or np.array_equal(got.values, want[1]))
    assert got.required == fake._requirement(COUNT, got.keys.itemsize, got.values is not None).size
    assert got.storage.numel() == WHERE["storage_off"] + got.required + BAND and got.before.shape == got.storage.shape
    assert fake.read_status(0, got.storage.data_ptr(), WHERE["storage_off"]) == 0


@pytest.mark.parametrize("call,fault", [(call, fault) for call in api.RECORDING_CALLS for fault in FAULTS if fault[2](call.facts)],
                         ids=lambda x: x.c_name if isinstance(x, api.RecordingCall) else x[0])
def test_every_fault_is_caught(call, fault):
    with pytest.raises(AssertionError, match=fault[1]):
        _run(call, FakeSorter(fault=fault))


@pytest.mark.parametrize("call", api.RECORDING_CALLS, ids=ROW_IDS)
def test_a_failure_word_is_caught_and_can_be_expected(call):
    with pytest.raises(AssertionError, match="the failure word is 0x1"):
        _run(call, FakeSorter(status=1))
    _run(call, FakeSorter(status=1), expect_status=1, sticky=1)
    with pytest.raises(AssertionError, match="sticky word"):
        _run(call, FakeSorter(status=1), expect_status=1, sticky=0)


@pytest.mark.parametrize("call", api.RECORDING_CALLS, ids=ROW_IDS)
def test_a_refusal_that_writes_the_storage_is_caught(call):
    got, _ = _run(call, FakeSorter(refuse=True), expect_refused=True)
    assert np.array_equal(got.keys, _inputs(call)[0]) and torch.equal(got.storage, got.before)
    with pytest.raises(AssertionError, match="a refused call wrote to the storage"):
        _run(call, FakeSorter(refuse=True, touch=True), expect_refused=True)
    with pytest.raises(AssertionError, match="must be refused"):
        _run(call, FakeSorter(), expect_refused=True)


def test_the_count_word_behind_the_keys():
    """the word shares the keys' buffer, 12 bytes behind the last key: read from there, and guarded on both sides"""
    call = next(c for c in api.RECORDING_CALLS if c.c_name == "vrdxHipCmdSort64KeyValueIndirect")
    got, want = _run(call, FakeSorter(), count_behind_keys=12)
    assert np.array_equal(got.keys, want[0]) and np.array_equal(got.values, want[1])
    for name, where in (("behind the keys", lambda a: a.keys + a.key_bytes + 11),
                        ("count word behind the keys changed", lambda a: a.indirect), ("behind the keys", lambda a: a.indirect + 4)):
        with pytest.raises(AssertionError, match=name):
            _run(call, FakeSorter(fault=(name, name, None, where)), count_behind_keys=12)


def test_a_callers_storage_is_used_as_it_is():
    call = api.RECORDING_CALLS[0]
    mine = torch.arange(4096, dtype=torch.int32).to(torch.uint8)
    got, want = _run(call, FakeSorter(), storage=mine)
    assert got.storage is mine and np.array_equal(got.keys, want[0])
    with pytest.raises(AssertionError, match="behind the storage requirement"):
        _run(call, FakeSorter(fault=(None, None, None, lambda a: a.storage + 4000 - WHERE["storage_off"])), storage=mine)


@pytest.mark.parametrize("kw", [dict(offsets=OFFSETS, device_count=5), dict(bit_range=(0, 8), order=0),
                                dict(order=0), dict(offsets=OFFSETS, order=0)], ids=str)
def test_a_combination_no_row_takes_is_a_type_error(kw):
    """segmented and indirect; a bit range and an order word; an order word over 32-bit keys"""
    with pytest.raises(TypeError, match="no recording call takes"):
        guarded_call(torch, FakeSorter(), np.arange(8, dtype=np.uint32), device="cpu", **kw)
    with pytest.raises(TypeError, match="no recording call takes"):
        guarded_call(torch, FakeSorter(), np.arange(8, dtype=np.uint64), bit_range=(0, 8), device="cpu")
