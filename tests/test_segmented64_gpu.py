"""GPU tests of the segmented sort of 64-bit keys (vrdxHipCmdSortSegmented64[KeyValue], vulkan_radix_sort_amd.sort_segments64):
every segment must come out as a stable ascending sort of itself as unsigned 64-bit -- checked against
np.lexsort((keys, segment id)) over the whole call -- with nothing written outside the segments or the storage requirement,
whatever size class the device put each segment in, with both ranking modes, keys-only and key+value, through a captured
graph replayed on another segmentation, and through the single header's own launcher."""
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

from guarded_call import ballot_sorter, sorter, to_device, to_host, torch_mod  # noqa: F401
from segmented_cases import expected, mixed_offsets, payload
from segmented64_cases import (LARGE_TILE, MID_MAX, MID_MAX_KEY_VALUE, SMALL_MAX, both_forms, make_keys64,
                               run_segmented64, uniform64)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKINGS = ["atomic", "ballot"]
# every class bound of both forms (4096; 8192 key+value, 16384 keys-only) and tiles of 8192 and 16384
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 24577, 32768,
         32769, 50001]
KINDS = (["uniform", "all-equal", "descending", "low-word-only", "high-word-only", "tile_depth", "all-ones", "eighth-ones",
          "few-distinct", "word-boundary"]
         + [f"byte{p}-constant" for p in range(8)] + [f"only-byte{p}" for p in (0, 3, 4, 7)])


def _pick(ranking, sorter, ballot_sorter):
    return sorter if ranking == "atomic" else ballot_sorter


@pytest.fixture(scope="module")
def cus(torch_mod):
    return int(torch_mod.cuda.get_device_properties(0).multi_processor_count)


# ---- 1. every class and every edge in one call ----------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_size_class_in_one_call(torch_mod, sorter, ballot_sorter, ranking, kind):
    """Segments of 0 ... 50001 keys (every class bound of both forms, tiles of 8192 and 16384 on either side) shuffled into
    one call behind a head of 100 untouched elements and in front of a tail of 77."""
    s = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    offsets, n = mixed_offsets(rng, SIZES)
    keys = make_keys64(kind, n, rng)
    both_forms(torch_mod, s, keys, offsets, payload(n), keys_off=8, values_off=4, offsets_off=4, storage_off=16)


# ---- 2. large-path tile edges ---------------------------------------------------------------------------------------------

TILE_LENGTHS = sorted({f(t) for t in (8192, 16384)
                       for f in (lambda t: t - 1, lambda t: t, lambda t: t + 1, lambda t: 2 * t, lambda t: 2 * t + 1,
                                 lambda t: 3 * t + 255)})


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("p", [0, 4, 7])
@pytest.mark.parametrize("length", TILE_LENGTHS)
def test_large_path_tile_edges(torch_mod, sorter, ballot_sorter, length, p, ranking):
    """One segment that starts at an odd element index, its first 16384 elements holding one value of byte p and the rest
    mixed: the first tile(s) count one digit only; up to 16384 elements byte p is constant (seven active passes: a copy
    back), beyond it is not (eight: none)."""
    s = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(length * 8 + p)
    start = 37
    n = start + length + 6
    keys = make_keys64(f"tile-byte{p}", n + 16384, rng)[:n]
    keys[start:start + length] = make_keys64(f"tile-byte{p}", max(length, 16384), rng)[:length]
    keys[start + 5] = keys[start + 1]  # duplicates
    offsets = np.array([start, start + length], np.uint32)
    both_forms(torch_mod, s, keys, offsets, payload(n))


# ---- 3. workgroup reuse ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _small_reuse_case():
    rng = np.random.default_rng(20)
    sizes = rng.integers(0, 4, size=(1 << 20) + 5)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys, values = uniform64(n, rng), payload(n)
    keys[1::3] = keys[0:-1:3][:len(keys[1::3])]  # neighbours with equal keys
    return keys, values, offsets, expected(keys, values, offsets, n)


@functools.lru_cache(maxsize=None)
def _list_reuse_case(cus, kind):
    """More than 2 x CUs segments per list, alternating sizes: a workgroup's second segment has another size."""
    rng = np.random.default_rng(cus)
    count = 2 * cus + 3
    a, b = (SMALL_MAX + 1, MID_MAX_KEY_VALUE) if kind == "mid" else (MID_MAX + 1, MID_MAX + 1200)
    sizes = [a if i % 2 == 0 else b for i in range(count)]
    if kind == "mid":
        sizes += [MID_MAX, MID_MAX_KEY_VALUE + 1] * 3  # mid keys-only, large key+value
    offsets = (5 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint32)
    n = int(offsets[-1]) + 9
    keys, values = uniform64(n, rng), payload(n)
    keys[::5] = keys[2]
    return keys, values, offsets, expected(keys, values, offsets, n)


@pytest.mark.parametrize("ranking", RANKINGS)
def test_small_kernel_takes_a_second_segment(torch_mod, sorter, ballot_sorter, ranking):
    """2^20 + 5 segments of 0 ... 3 keys: the small launch's 2^20 workgroups take the last five in a second trip."""
    keys, values, offsets, want = _small_reuse_case()
    both_forms(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want)


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("kind", ["mid", "large"])
def test_list_kernels_take_a_second_segment_of_another_size(torch_mod, sorter, ballot_sorter, cus, kind, ranking):
    keys, values, offsets, want = _list_reuse_case(cus, kind)
    both_forms(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want)


# ---- 4. bad offsets -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_bad_offsets_leave_their_segments_alone_and_say_so(torch_mod, sorter, ballot_sorter, ranking, key_value):
    """A decreasing pair and a last offset behind maxElementCount: those segments are left alone, the valid ones sorted,
    the failure word and the sorter's word carry STATUS_SEGMENTS_INVALID.  The buffers reach 65536 elements in front of the
    arrays and behind maxElementCount, so a missing bound check would change a guard band, never memory outside an
    allocation."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    s = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    s.read_sorter_status(stream)  # (clears it)
    n = 50000
    rng = np.random.default_rng(3)
    keys = make_keys64("uniform", n, rng)
    keys[::9] = keys[4]
    values = payload(n) if key_value else None
    # [100, 1100) small, [1100, 21100) large, [21100, 9000) decreasing, [9000, 9000) empty, [9000, n + 5000) beyond the bound
    offsets = np.array([100, 1100, 21100, 9000, 9000, n + 5000], np.uint32)
    gk, gv, _ = run_segmented64(torch, s, keys, offsets, values, guard=65536, expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    ek, ev = expected(keys, values, offsets, n)
    assert np.array_equal(gk, ek)
    assert np.array_equal(gk[21100:], keys[21100:]) and np.array_equal(gk[:100], keys[:100])
    if key_value:
        assert np.array_equal(gv, ev)
    assert s.read_sorter_status(stream) & vrdx.STATUS_SEGMENTS_INVALID
    assert s.read_sorter_status(stream) == 0  # (reading it cleared it)


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_overlapping_segments_cannot_overfill_a_list(torch_mod, sorter, ballot_sorter, ranking, key_value):
    """Offsets 0, 5000, 0, 5000, ... list the mid segment [0, 5000) 64 times where the mid list has 10 slots: slots beyond
    the capacity are dropped.  A large segment in front of the pairs, a large and a small one behind them, all disjoint from
    [0, 5000), must come out sorted -- the large list lies right behind the mid list -- and everything else outside
    [0, 5000) untouched, with STATUS_SEGMENTS_INVALID from the decreasing pairs.  [0, 5000) is sorted by several workgroups
    at once: nothing is asserted about it."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    s = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    s.read_sorter_status(stream)
    pairs, raced, large_front, large_behind, small = 64, 5000, 20000, 17000, 300
    front = raced + large_behind + small + 50
    n = front + large_front + 33
    offsets = np.array([front, front + large_front] + [0, raced] * pairs + [raced + large_behind, raced + large_behind + small],
                       np.uint32)
    assert pairs > 4 * (n // (SMALL_MAX + 1))
    rng = np.random.default_rng(pairs)
    keys = make_keys64("uniform", n, rng)
    keys[::7] = keys[3]
    values = payload(n) if key_value else None
    gk, gv, _ = run_segmented64(torch, s, keys, offsets, values, guard=65536, expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    disjoint = np.array([raced, raced + large_behind, raced + large_behind + small], np.uint32)
    ek, ev = expected(keys, values, disjoint, n)  # ([front, front + large_front) below)
    order = np.argsort(keys[front:front + large_front], kind="stable")
    ek[front:front + large_front] = keys[front:front + large_front][order]
    assert np.array_equal(gk[raced:], ek[raced:])
    if key_value:
        ev[front:front + large_front] = values[front:front + large_front][order]
        assert np.array_equal(gv[raced:], ev[raced:])
    assert s.read_sorter_status(stream) & vrdx.STATUS_SEGMENTS_INVALID
    assert s.read_sorter_status(stream) == 0


# ---- 5. alignment and reused storage --------------------------------------------------------------------------------------

ALIGNMENTS = [(0, 0, 0, 0, 0), (8, 4, 4, 16, 1), (24, 12, 0, 48, 0), (8, 12, 4, 48, 1), (24, 0, 4, 16, 1), (0, 4, 0, 48, 0)]


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("keys_off,values_off,offsets_off,storage_off,start", ALIGNMENTS)
def test_every_alignment(torch_mod, sorter, ballot_sorter, keys_off, values_off, offsets_off, storage_off, start, ranking):
    """keysOffset in {0, 8, 24}, valuesOffset in {0, 4, 12}, offsetsOffset in {0, 4}, storageOffset in {0, 16, 48}, the first
    segment at an even and at an odd element."""
    s = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(keys_off + values_off + storage_off + start)
    offsets, n = mixed_offsets(rng, [3, 700, 4097, 9001, 16385, 20001], head=2 + start)
    keys = make_keys64("tile_depth", n, rng)
    both_forms(torch_mod, s, keys, offsets, payload(n), keys_off=keys_off, values_off=values_off, offsets_off=offsets_off,
               storage_off=storage_off)


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_storage_reused_for_a_call_of_another_shape(torch_mod, sorter, ballot_sorter, key_value, ranking):
    """A second call of another segmentation (fewer, other classes) on the storage the first left behind, not re-initialised:
    the fill resets the header and both list counters."""
    sorter = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(11)
    n = 120_000
    keys = make_keys64("uniform", n, rng)
    values = payload(n) if key_value else None
    storage = None
    for sizes in ([5000] * 8 + [20000] * 3 + [100] * 30, [9000, 2, 70000, 4096]):
        offsets, used = mixed_offsets(rng, sizes, head=1, tail=0)
        assert used <= n
        gk, gv, storage = run_segmented64(torch_mod, sorter, keys, offsets, values, storage=storage)
        ek, ev = expected(keys, values, offsets, n)
        assert np.array_equal(gk, ek)
        if key_value:
            assert np.array_equal(gv, ev)


# ---- 6. degenerate calls --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
def test_degenerate_calls_record_nothing(torch_mod, sorter, ballot_sorter, ranking):
    """segmentCount == 0 and maxElementCount == 0 touch nothing (every byte of the storage stays as it was), keys-only and
    key+value."""
    torch = torch_mod
    sorter = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    host = np.arange(1000, 0, -1, dtype=np.uint64) << np.uint64(33)
    keys, values = to_device(torch, host), to_device(torch, np.arange(1000, dtype=np.uint32))
    offsets = to_device(torch, np.array([0, 1000], np.uint32))
    storage = torch.full((sorter.storage_requirements64(1000, key_value=True).size,), 0xA5, dtype=torch.uint8, device="cuda")
    sorter.cmd_sort_segmented64(stream, 1000, 0, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)
    sorter.cmd_sort_segmented64(stream, 0, 1, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0)
    sorter.cmd_sort_segmented64_key_value(stream, 1000, 0, offsets.data_ptr(), 0, keys.data_ptr(), 0, values.data_ptr(), 0,
                                          storage.data_ptr(), 0)
    sorter.cmd_sort_segmented64_key_value(stream, 0, 1, offsets.data_ptr(), 0, keys.data_ptr(), 0, values.data_ptr(), 0,
                                          storage.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(keys), host) and np.array_equal(to_host(values), np.arange(1000, dtype=np.uint32))
    assert bool((storage == 0xA5).all())


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_degenerate_calls_record_their_timestamps(torch_mod, sorter, ballot_sorter, key_value, ranking):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    sorter = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    keys = to_device(torch, np.arange(8, dtype=np.uint64))
    values = to_device(torch, np.arange(8, dtype=np.uint32))
    offsets = to_device(torch, np.array([0, 8], np.uint32))
    storage = torch.empty(sorter.storage_requirements64(8, key_value=key_value).size, dtype=torch.uint8, device="cuda")
    for n, segments in ((8, 0), (0, 1)):
        pool = vrdx.QueryPool(15)
        if key_value:
            sorter.cmd_sort_segmented64_key_value(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                  values.data_ptr(), 0, storage.data_ptr(), 0, pool, 0)
        else:
            sorter.cmd_sort_segmented64(stream, n, segments, offsets.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0,
                                        pool, 0)
        torch.cuda.synchronize()
        ts = pool.results_ns(0, 15)
        assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
        pool.destroy()
    assert np.array_equal(to_host(keys), np.arange(8, dtype=np.uint64))


@pytest.mark.parametrize("ranking", RANKINGS)
def test_a_large_bound_and_a_small_use(torch_mod, sorter, ballot_sorter, ranking):
    """maxElementCount = 2^22 with segments over some 60000 elements near its far end."""
    s = _pick(ranking, sorter, ballot_sorter)
    n = 1 << 22
    rng = np.random.default_rng(22)
    offsets, end = mixed_offsets(rng, [300, 5000, 9000, 20000, 25000, 0, 1], head=n - 59301 - 3, tail=3)
    assert end == n
    keys = make_keys64("uniform", n, rng)
    keys[n - 59000::6] = keys[n - 1]
    both_forms(torch_mod, s, keys, offsets, payload(n))


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_query_pool_slots(torch_mod, sorter, ballot_sorter, key_value, ranking):
    """All 15 slots readable and non-decreasing, slots 5 ... 14 equal to slot 4."""
    import vulkan_radix_sort_amd as vrdx
    sorter = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(15)
    offsets, n = mixed_offsets(rng, [100, 6000, 40000, 2])
    keys = make_keys64("uniform", n, rng)
    values = payload(n) if key_value else None
    pool = vrdx.QueryPool(15)
    gk, gv, _ = run_segmented64(torch_mod, sorter, keys, offsets, values, pool=pool)
    ek, ev = expected(keys, values, offsets, n)
    assert np.array_equal(gk, ek) and (not key_value or np.array_equal(gv, ev))
    ts = pool.results_ns(0, 15)
    assert len(ts) == 15 and ts[0] == 0 and all(b >= a for a, b in zip(ts, ts[1:]))
    assert ts[4] > 0 and all(t == ts[4] for t in ts[5:])
    pool.destroy()


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_status_is_clear_and_the_plan_verdict_is_none(torch_mod, sorter, ballot_sorter, key_value, ranking):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    sorter = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    sorter.read_sorter_status(stream)
    rng = np.random.default_rng(9)
    offsets, n = mixed_offsets(rng, [300, 5000, 20000, 0, 1])
    keys = make_keys64("uniform", n, rng)
    values = payload(n) if key_value else None
    gk, gv, storage = run_segmented64(torch, sorter, keys, offsets, values)
    ek, ev = expected(keys, values, offsets, n)
    assert np.array_equal(gk, ek) and (not key_value or np.array_equal(gv, ev))
    assert sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == vrdx.VERDICT_NONE
    assert sorter.read_sorter_status(stream) == 0


# ---- 7. graph -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_captured_graph_replays_on_new_keys_and_a_new_segmentation(torch_mod, sorter, ballot_sorter, key_value, ranking):
    """One call captured in torch.cuda.graph sorts whatever keys AND whatever offsets it is replayed on, as long as
    segmentCount stays: segments move across all three classes between the replays."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    sorter = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(77)
    n = 400_000
    segmentations = [[300] * 60 + [5000] * 20 + [40000] * 4 + [0] * 16,
                     [20000] * 15 + [17] * 60 + [9000] * 5 + [3] * 20]
    offsets_list = []
    for sizes in segmentations:
        sizes = list(sizes)
        rng.shuffle(sizes)
        offsets_list.append(np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))
    assert len({len(o) for o in offsets_list}) == 1 and all(o[-1] <= n for o in offsets_list)
    dk, do = to_device(torch, np.zeros(n, np.uint64)), to_device(torch, offsets_list[0])
    dv = to_device(torch, np.zeros(n, np.uint32)) if key_value else None
    storage = torch.empty(sorter.storage_requirements64(n, key_value=key_value).size, dtype=torch.uint8, device="cuda")
    vrdx.sort_segments64(sorter, dk, do, values=dv, storage=storage)  # one eager call first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort_segments64(sorter, dk, do, values=dv, storage=storage)
    values = payload(n) if key_value else None
    for replay, offsets in enumerate(offsets_list + offsets_list[::-1]):
        keys = make_keys64("uniform" if replay % 2 == 0 else "tile_depth", n, rng)
        dk.copy_(to_device(torch, keys))
        if key_value:
            dv.copy_(to_device(torch, values))
        do.copy_(to_device(torch, offsets))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ek, ev = expected(keys, values, offsets, n)
        assert np.array_equal(to_host(dk), ek)
        if key_value:
            assert np.array_equal(to_host(dv), ev)
        assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0


# ---- 8. front end ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("with_values,own_storage", [(False, False), (True, False), (True, True), (False, True)])
def test_sort_segments64_python_front_end(torch_mod, sorter, ballot_sorter, with_values, own_storage, ranking):
    """torch.int64 keys with negative values among them, ordered as unsigned: the negatives end behind the others."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    sorter = _pick(ranking, sorter, ballot_sorter)
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, 3000, size=200)
    sizes[::50] = 20000
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = make_keys64("uniform", n, rng)
    assert (keys.view(np.int64) < 0).any() and (keys.view(np.int64) > 0).any()
    values = payload(n) if with_values else None
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    assert dk.dtype == torch.int64
    dv, do = (to_device(torch, values) if with_values else None), to_device(torch, offsets)
    mine = None
    if own_storage:
        mine = torch.empty(sorter.storage_requirements64(n, key_value=with_values).size + 64, dtype=torch.uint8, device="cuda")
    storage = vrdx.sort_segments64(sorter, dk, do, values=dv, storage=mine)
    torch.cuda.synchronize()
    assert mine is None or storage is mine
    ek, ev = expected(keys, values, offsets, n)
    assert np.array_equal(to_host(dk), ek)
    if with_values:
        assert np.array_equal(to_host(dv), ev)
    assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0


def test_sort_segments64_rejects_bad_device_arguments(torch_mod, sorter):
    """The refusals of sort_segments64 that need device tensors or a sorter (tests/test_segmented64_abi.py has those that do
    not): offsets of a wrong dtype, length, shape or device, values of a wrong dtype or length, a storage that is too small,
    of a wrong dtype or not on a 16-byte boundary -- the exception types of sort_segments and sort64, before anything is
    recorded."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    host_offsets = torch.tensor([0, 8, 16], dtype=torch.int32)
    dk, do = torch.zeros(16, dtype=torch.int64, device="cuda"), host_offsets.cuda()
    with pytest.raises(TypeError):
        vrdx.sort_segments64(None, dk, do.to(torch.int64))
    with pytest.raises(ValueError):
        vrdx.sort_segments64(None, dk, do[:0])
    with pytest.raises(ValueError):
        vrdx.sort_segments64(None, dk, do.view(1, 3))
    with pytest.raises(ValueError):
        vrdx.sort_segments64(None, dk, host_offsets)
    with pytest.raises(TypeError):
        vrdx.sort_segments64(None, dk, do, values=dk)
    with pytest.raises(ValueError):
        vrdx.sort_segments64(None, dk, do, values=torch.zeros(8, dtype=torch.int32, device="cuda"))
    need = sorter.storage_requirements64(16).size
    with pytest.raises(ValueError):
        vrdx.sort_segments64(sorter, dk, do, storage=torch.empty(need - 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        vrdx.sort_segments64(sorter, dk, do, storage=torch.empty(need, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):  # storageOffset is a multiple of 16: so is the address of a storage tensor
        vrdx.sort_segments64(sorter, dk, do, storage=torch.empty(need + 16, dtype=torch.uint8, device="cuda")[8:])
    assert bool((dk == 0).all())


# ---- 9. single header -----------------------------------------------------------------------------------------------------

SINGLE_HEADER_CASE = r"""
#define VRDX_IMPLEMENTATION
#include "vk_radix_sort.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

int main() {
  VrdxSorterCreateInfo info = {};
  VrdxSorter sorter = nullptr;
  if (vrdxCreateSorter(&info, &sorter) != VK_SUCCESS) { std::printf("no sorter\n"); return 2; }
  const std::vector<uint32_t> sizes = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4095, 4096, 4097, 8191, 8192, 8193, 16383,
                                       16384, 16385, 24577, 32768, 32769, 50001};
  std::vector<uint32_t> offsets = {100};
  for (uint32_t s : sizes) offsets.push_back(offsets.back() + s);
  const uint32_t n = offsets.back() + 77;
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> values(n);
  uint64_t x = 88172645463325252ull;
  for (uint32_t i = 0; i < n; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;  // uniform 64-bit keys
    keys[i] = i % 5 == 0 ? keys[i / 5] : x;
    values[i] = i ^ 0x80000000u;
  }
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  for (size_t s = 0; s < sizes.size(); ++s)
    std::stable_sort(idx.begin() + offsets[s], idx.begin() + offsets[s + 1], [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  uint64_t* dk; uint32_t *dv, *doff; uint8_t* st;
  VrdxSorterStorageRequirements req;
  vrdxHipGetSorter64KeyValueStorageRequirements(sorter, n, &req);
  if (hipMalloc(&dk, 8ull * n) != hipSuccess || hipMalloc(&dv, 4ull * n) != hipSuccess ||
      hipMalloc(&doff, 4 * offsets.size()) != hipSuccess || hipMalloc(&st, req.size) != hipSuccess) return 3;
  (void)hipMemcpy(doff, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice);
  size_t bad = 0;
  std::vector<uint64_t> gk(n);
  std::vector<uint32_t> gv(n);
  for (int keyValue = 0; keyValue < 2; ++keyValue) {
    (void)hipMemcpy(dk, keys.data(), 8ull * n, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv, values.data(), 4ull * n, hipMemcpyHostToDevice);
    if (keyValue)
      vrdxHipCmdSortSegmented64KeyValue(nullptr, sorter, n, (uint32_t)sizes.size(), (VkBuffer)doff, 0, (VkBuffer)dk, 0,
                                        (VkBuffer)dv, 0, (VkBuffer)st, 0, nullptr, 0);
    else
      vrdxHipCmdSortSegmented64(nullptr, sorter, n, (uint32_t)sizes.size(), (VkBuffer)doff, 0, (VkBuffer)dk, 0, (VkBuffer)st, 0,
                                nullptr, 0);
    (void)hipMemcpy(gk.data(), dk, 8ull * n, hipMemcpyDeviceToHost);
    (void)hipMemcpy(gv.data(), dv, 4ull * n, hipMemcpyDeviceToHost);
    for (uint32_t i = 0; i < n; ++i) bad += gk[i] != keys[idx[i]] || gv[i] != values[keyValue ? idx[i] : i];
  }
  const uint32_t status = vrdxHipReadSorterStatus(sorter, nullptr);
  std::printf("status %u, %zu mismatches\n", status, bad);
  vrdxDestroySorter(sorter);
  return (bad == 0 && status == 0) ? 0 : 1;
}
"""


def test_single_header_segmented64_parity(tmp_path):
    """Both entry points through the single header's own launcher (the kernels resolved by mangled name, with the LDS sizes
    of the launch layer it shares with the library), compiled with plain g++: the sizes of case 1 on uniform keys."""
    header = os.path.join(ROOT, "build", "single_header", "vk_radix_sort.h")
    if not os.path.exists(header):
        subprocess.run(["python3", os.path.join(ROOT, "tools", "generate_single_header.py"), "-o", header], check=True)
    src = tmp_path / "segmented64_single_header.cc"
    src.write_text(SINGLE_HEADER_CASE)
    exe = tmp_path / "segmented64_single_header"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.dirname(header), str(src), "-o", str(exe), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "status 0, 0 mismatches" in r.stdout, r.stdout + r.stderr
