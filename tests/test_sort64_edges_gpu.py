"""GPU tests of what surrounds the two inner sorts of vrdxHipCmdSort64[KeyValue] -- the streaming kernels, MakeSort64Layout and
the recording order of RecordSort64 -- at the places where they can be wrong while the inner sorts are right:

  a. values that are not their own index (payload64): a permute that writes the index, or reads the values at another
     base, gives the right result on iota values;
  b. every alignment of the caller's arrays (keys 0 | 8 mod 16, values 0 | 4 | 8 | 12 mod 16) times every n mod 4, in one
     workgroup of the streaming kernels and in several, at tiny counts, and with the scalar tail in the last thread of a
     workgroup or the first of the next;
  c. keys and values in one buffer;
  d. the verdict and status words the header promises: those of the second inner sort, over the high words;
  e. one storage for 64-bit sorts of several counts, a 32-bit sort and a segmented sort, back to back;
  f. a captured call replayed at a size where the device decides each inner sort's plan at every replay;
  g. two sorts on two streams.

Every result is compared element for element with numpy (tests/sort64_model.py: the inputs, the reference, the model of the
verdict; tests/test_sort64_model.py shows without a GPU which mistakes these inputs tell from the right sort)."""
import functools

import numpy as np
import pytest

import plan_model
import segmented_cases
import sort64_model as model
from guarded_call import BAND_BYTE as STORAGE_GUARD
from guarded_call import GUARD_BYTE as GUARD
from guarded_call import sorter, torch_mod  # noqa: F401
from sort64_model import case_inputs, check64, with_tail
from test_sort64_gpu import run64
from test_sort_gpu import msd_capacity

pytestmark = pytest.mark.gpu

MSD_SIZE = 8_200_001       # the inner sorts record the MSD plan
HYBRID_SIZE = (1 << 18) + 3  # ... the hybrid plan


@functools.lru_cache(maxsize=None)
def _case(pattern, n):
    """(keys, values, order): one case's inputs and np.argsort(keys, kind="stable"), computed once for every test and mode
    that runs the case; nobody writes to them"""
    keys, values = case_inputs(pattern, n)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    for a in (keys, values, order):
        a.setflags(write=False)
    return keys, values, order


def _want(pattern, n, key_value):
    keys, values, order = _case(pattern, n)
    return keys[order], (values[order] if key_value else None)


@functools.lru_cache(maxsize=None)
def _verdict(pattern, n, plan, bits, cap):
    return model.second_sort_verdict(_case(pattern, n)[0], plan, bits, cap)


def model_verdict(s, pattern, n):
    """what the model says the device makes of the second inner sort: a key+value sort of n words, keys-only or not"""
    info = s.describe_plan(n, True)
    bits = int(info.bits)
    return _verdict(pattern, n, info.name, bits, msd_capacity(n, bits) if info.name == "msd" else 0)


def _status_is_clean(torch, s, storage, storage_off=0):
    stream = torch.cuda.current_stream().cuda_stream
    assert s.read_status(stream, storage.data_ptr(), storage_off) == 0
    assert s.read_sorter_status(stream) == 0


# ---- a. values that are not the index --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", model.VALUE_PATTERNS)
@pytest.mark.parametrize("n", model.VALUE_SIZES)
def test_values_that_are_not_their_index(torch_mod, sorter, n, pattern):
    keys, values, _ = _case(pattern, n)
    guarded_keys, guarded_values = with_tail(keys, values)
    got_keys, got_values = run64(torch_mod, sorter, guarded_keys, guarded_values, count=n)
    check64(got_keys, got_values, guarded_keys, guarded_values, count=n, want=_want(pattern, n, True))


# ---- b. alignment x tail -----------------------------------------------------------------------------------------------------

def _aligned_run(torch, s, n, key_value, keys_off, values_off):
    keys, values, _ = _case("dup-high", n)
    guarded_keys, guarded_values = with_tail(keys, values if key_value else None)
    try:
        got_keys, got_values = run64(torch, s, guarded_keys, guarded_values, keys_off=keys_off, values_off=values_off,
                                     count=n)
        check64(got_keys, got_values, guarded_keys, guarded_values, count=n, want=_want("dup-high", n, key_value))
    except AssertionError as e:
        raise AssertionError(f"n={n} keys at {keys_off} mod 16, values at {values_off} mod 16: {e}") from e


MATRIX_SIZES = [1024 * k + r for k in model.MATRIX_BLOCKS for r in range(4)] + model.TINY_SIZES


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_every_alignment_and_every_tail(torch_mod, sorter, key_value):
    """The caller's keys move as 16-byte accesses that may be 8-byte aligned only, the caller's values as 16-byte accesses
    that may be 4-byte aligned only, and the last n mod 4 elements one by one: every combination, with the tail in the
    only workgroup (1024 + r), in the last of several (37 * 1024 + r) and where it is all there is."""
    assert {n % 4 for n in MATRIX_SIZES[:8]} == {0, 1, 2, 3}
    for n in MATRIX_SIZES:
        for keys_off in (0, 8):
            for values_off in ((0, 4, 8, 12) if key_value else (0,)):
                _aligned_run(torch_mod, sorter, n, key_value, keys_off, values_off)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_the_tail_at_the_edge_of_a_workgroup(torch_mod, sorter, key_value):
    """A workgroup of the streaming kernels takes 256 x 4 elements: the thread with the scalar tail is the last of a
    workgroup (1021 ... 1023, 2047) or the first of the next (1025 ... 1027, 2049), at the least aligned arrays."""
    for n in model.EDGE_SIZES:
        _aligned_run(torch_mod, sorter, n, key_value, 8, 12)


# ---- c. keys and values in one buffer ------------------------------------------------------------------------------------

def test_keys_and_values_in_one_buffer(torch_mod, sorter):
    """keys at 8 mod 16, the values behind them at 4 mod 16, guard bytes in front, between and behind"""
    torch = torch_mod
    n = 100_003
    keys, values, _ = _case("dup-high", n)
    keys_off = 8
    values_off = (keys_off + keys.nbytes + 64 + 15) // 16 * 16 + 4
    end = values_off + values.nbytes
    assert keys_off % 16 == 8 and values_off % 16 == 4 and values_off >= keys_off + keys.nbytes + 64
    host = np.full(end + 256, GUARD, dtype=np.uint8)
    host[keys_off:keys_off + keys.nbytes] = keys.view(np.uint8)
    host[values_off:end] = values.view(np.uint8)
    buf = torch.from_numpy(host.copy()).cuda()
    assert buf.data_ptr() % 16 == 0
    required = sorter.storage_requirements64(n, True).size
    storage = torch.full((required + 256,), STORAGE_GUARD, dtype=torch.uint8, device="cuda")
    assert storage.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    sorter.cmd_sort64_key_value(stream, n, buf.data_ptr(), keys_off, buf.data_ptr(), values_off, storage.data_ptr(), 0)
    torch.cuda.synchronize()
    _status_is_clean(torch, sorter, storage)
    assert bool((storage[required:] == STORAGE_GUARD).all()), "the storage buffer behind the requirement was written"
    out = buf.cpu().numpy()
    for a, b in ((0, keys_off), (keys_off + keys.nbytes, values_off), (end, len(out))):
        assert (out[a:b] == GUARD).all(), f"guard bytes {a} ... {b} were written"
    check64(out[keys_off:keys_off + keys.nbytes].copy().view(np.uint64), out[values_off:end].copy().view(np.uint32), keys,
            values, want=_want("dup-high", n, True))


# ---- d. the verdict and the status -------------------------------------------------------------------------------------------

VERDICT_PATTERNS = ["uniform", "high-constant", "low-constant", "8-distinct", "bit63-mixed"]


@pytest.mark.parametrize("pattern", VERDICT_PATTERNS)
@pytest.mark.parametrize("n,plan", [(MSD_SIZE, "msd"), (HYBRID_SIZE, "hybrid-8")])
def test_the_verdict_is_that_of_the_sort_over_the_high_words(torch_mod, sorter, n, plan, pattern):
    """vrdxHipReadStatus and vrdxHipReadPlanVerdict on the storage of a 64-bit sort report the second inner sort: a key+value
    sort of the high words in the order the sort by the low words left them.  The expected verdict is plan_model's."""
    assert sorter.describe_plan(n, True).name == plan
    want = model_verdict(sorter, pattern, n)
    if plan == "msd" and pattern == "high-constant":
        assert want == plan_model.VERDICT_MSD_SORTED
    if plan == "msd" and pattern == "uniform":
        assert want == plan_model.VERDICT_MSD_RUNS
    keys, values, _ = _case(pattern, n)
    stream = torch_mod.cuda.current_stream().cuda_stream
    for key_value in (False, True):
        kept = []
        got_keys, got_values = run64(torch_mod, sorter, keys, values if key_value else None, storage_out=kept)
        check64(got_keys, got_values, keys, values if key_value else None, want=_want(pattern, n, key_value))
        got = sorter.read_plan_verdict(stream, kept[0].data_ptr(), 0)
        print(f"n={n} {pattern} {'pairs' if key_value else 'keys'}: verdict {got}, model {want}")
        assert got == want, (pattern, n, key_value, got, want)
        _status_is_clean(torch_mod, sorter, kept[0])


# ---- e. one storage, many calls ------------------------------------------------------------------------------------------

def test_one_storage_for_sorts_of_every_kind_and_count(torch_mod, sorter):
    """RecordSort64 carves the storage from the call's elementCount: the bytes that are a word array in one call are the
    inner histogram or scratch of the next.  Six calls on one storage and one stream, a host sync after every third only;
    every call has buffers of its own, and every result is checked."""
    torch = torch_mod
    stream = torch.cuda.current_stream().cuda_stream
    required = sorter.storage_requirements64(MSD_SIZE, True).size
    storage = torch.full((required + 256,), STORAGE_GUARD, dtype=torch.uint8, device="cuda")  # poisoned once
    assert storage.data_ptr() % 16 == 0
    st = storage.data_ptr()

    def dev64(a):
        return torch.from_numpy(a.view(np.int64).copy()).cuda()

    def dev32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()

    def sort64(pattern, n, key_value):
        keys, values, _ = _case(pattern, n)
        assert sorter.storage_requirements64(n, key_value).size <= required
        dk, dv = dev64(keys), (dev32(values) if key_value else None)

        def record():
            if key_value:
                sorter.cmd_sort64_key_value(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, st, 0)
            else:
                sorter.cmd_sort64(stream, n, dk.data_ptr(), 0, st, 0)

        def check():
            check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys,
                    values if key_value else None, want=_want(pattern, n, key_value))
        return record, check

    def sort32(n):
        rng = np.random.default_rng(32)
        keys = rng.integers(0, 1 << 20, size=n, dtype=np.uint64).astype(np.uint32)  # (ties: 300 000 keys of 20 bits)
        values = segmented_cases.payload(n)
        assert sorter.key_value_storage_requirements(n).size <= required
        dk, dv = dev32(keys), dev32(values)

        def record():
            sorter.cmd_sort_key_value(stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, st, 0)

        def check():
            order = np.argsort(keys, kind="stable")
            assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys[order])
            assert np.array_equal(dv.cpu().numpy().view(np.uint32), values[order])
        return record, check

    def segmented():
        rng = np.random.default_rng(33)
        offsets, n = segmented_cases.mixed_offsets(rng, [300, 5000, 20000, 0, 1, 40000])
        keys = segmented_cases.make_keys("uniform", n, rng)
        assert sorter.storage_requirements(n).size <= required
        dk, do = dev32(keys), dev32(offsets)

        def record():
            sorter.cmd_sort_segmented(stream, n, len(offsets) - 1, do.data_ptr(), 0, dk.data_ptr(), 0, st, 0)

        def check():
            want_keys, _ = segmented_cases.expected(keys, None, offsets, n)
            assert np.array_equal(dk.cpu().numpy().view(np.uint32), want_keys)
            assert np.array_equal(do.cpu().numpy().view(np.uint32), offsets)
        return record, check

    groups = [[sort64("dup-high", MSD_SIZE, True), sort64("tile-depth", 70_002, False), sort32(300_000)],
              [segmented(), sort64("dup-high", 16_385, True), sort64("uniform", MSD_SIZE, False)]]
    torch.cuda.synchronize()
    for group in groups:
        for record, _ in group:
            record()
        torch.cuda.synchronize()
        for _, check in group:
            check()
    assert sorter.read_plan_verdict(stream, st, 0) == model_verdict(sorter, "uniform", MSD_SIZE)
    _status_is_clean(torch, sorter, storage)
    assert bool((storage[required:] == STORAGE_GUARD).all()), "the storage buffer behind the requirement was written"


# ---- f. replay at an MSD size --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_a_captured_sort_replays_at_an_msd_size(torch_mod, sorter, key_value):
    """One call captured once at a size where both inner sorts record the MSD plan, which the device takes or turns down
    for each of them at every replay: inputs whose low words, high words or both make it decide otherwise than for the
    input before, and the first input again at the end."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    n = MSD_SIZE
    assert sorter.describe_plan(n, True).name == "msd"
    stream = torch.cuda.current_stream().cuda_stream
    dk = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
    storage = torch.empty(sorter.storage_requirements64(n, key_value).size, dtype=torch.uint8, device="cuda")
    vrdx.sort64(sorter, dk, dv, storage=storage)  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort64(sorter, dk, dv, storage=storage)
    seen = set()
    for pattern in ("uniform", "high-constant", "8-distinct", "low-constant", "uniform"):
        keys, values, _ = _case(pattern, n)
        dk.copy_(torch.from_numpy(keys.view(np.int64).copy()))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys,
                values if key_value else None, want=_want(pattern, n, key_value))
        want = model_verdict(sorter, pattern, n)
        got = sorter.read_plan_verdict(stream, storage.data_ptr(), 0)
        print(f"replay on {pattern}: verdict {got}, model {want}")
        assert got == want, (pattern, got, want)
        _status_is_clean(torch, sorter, storage)
        seen.add(want)
    assert {plan_model.VERDICT_MSD_RUNS, plan_model.VERDICT_MSD_SORTED, plan_model.VERDICT_NONE} <= seen


# ---- g. two streams ----------------------------------------------------------------------------------------------------------

def test_two_sorts_on_two_streams(torch_mod, sorter):
    """one sorter, two streams, two storages: a keys-only and a key+value sort of 500 000 elements in flight together"""
    torch = torch_mod
    n = 500_000
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    torch.cuda.synchronize()
    for st, pattern, key_value in zip(streams, ("uniform", "dup-high"), (False, True)):
        keys, values, _ = _case(pattern, n)
        with torch.cuda.stream(st):
            dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
            dv = torch.from_numpy(values.view(np.int32).copy()).cuda() if key_value else None
            storage = torch.full((sorter.storage_requirements64(n, key_value).size + 256,), STORAGE_GUARD, dtype=torch.uint8,
                                 device="cuda")
            for _ in range(3):  # sorting sorted pairs again changes nothing and keeps both streams busy
                if key_value:
                    sorter.cmd_sort64_key_value(st.cuda_stream, n, dk.data_ptr(), 0, dv.data_ptr(), 0, storage.data_ptr(), 0)
                else:
                    sorter.cmd_sort64(st.cuda_stream, n, dk.data_ptr(), 0, storage.data_ptr(), 0)
        runs.append((st, pattern, key_value, dk, dv, storage))
    torch.cuda.synchronize()
    for st, pattern, key_value, dk, dv, storage in runs:
        keys, values, _ = _case(pattern, n)
        check64(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None, keys,
                values if key_value else None, want=_want(pattern, n, key_value))
        required = sorter.storage_requirements64(n, key_value).size
        assert bool((storage[required:] == STORAGE_GUARD).all()), "the storage buffer behind the requirement was written"
        assert sorter.read_status(st.cuda_stream, storage.data_ptr(), 0) == 0
        assert sorter.read_sorter_status(st.cuda_stream) == 0
