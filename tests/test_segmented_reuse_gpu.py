"""GPU tests of the segmented sort where its kernels go round their loops: a workgroup that sorts a second and a third
segment out of the LDS it used for the first (more than 2^20 segments for the small kernel, more than 2 x CUs and 4 x CUs
listed segments for the mid and the large one), mid and large lists filled to their last slot and overfilled by overlapping
segments, the key and payload patterns of the plain sort's tests in every size class (0xFFFFFFFF -- the pad of every load
-- among the keys, one, two and three active passes, one digit filling the large path's first tile), a bound far above what
the offsets use, and the tile edges of the large path at every 16-byte phase.

The reference of every case is np.lexsort((keys, segment id)) over the whole call, compared bit for bit on keys and values
with np.array_equal, inside run_segmented's guard bands (segmented_cases.py).  The sizes follow the device's CU count, and
every case asserts that it still has more segments than the grid of the kernel it is about."""
import functools
import zlib

import numpy as np
import pytest

from guarded_call import ballot_sorter, sorter, to_device, to_host, torch_mod  # noqa: F401
from segmented_cases import check, expected, make_keys, payload, run_segmented

pytestmark = pytest.mark.gpu

SMALL_MAX, MID_MAX, TILE = 4096, 16384, 16384   # kSegSmallMax, kSegMidMax, kSegLargeTile (vrdx_kernels.h)
SMALL_GRID = 1 << 20                            # the small kernel's grid cap (RecordSegmentedSort)
RANKINGS = ["atomic", "ballot"]


@pytest.fixture(scope="module")
def cus(torch_mod):
    """The mid and the large kernel run min(segmentCount, list capacity, 2 x CUs) workgroups."""
    return int(torch_mod.cuda.get_device_properties(0).multi_processor_count)


def _pick(ranking, sorter, ballot_sorter):
    return sorter if ranking == "atomic" else ballot_sorter


def _offsets(sizes, head=0):
    o = head + np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    assert o[-1] < 1 << 32
    return o.astype(np.uint32)


def _with_duplicates(keys):
    keys[1::3] &= np.uint32(0xFF)  # equal keys in every segment of some length: stability has something to show
    return keys


def _both_modes(torch, s, keys, offsets, values, want=None, **kw):
    """Keys-only, then key+value, against one reference (the expected keys are the same in both)."""
    if want is None:
        want = expected(keys, values, offsets, len(keys))
    gk, _, _ = run_segmented(torch, s, keys, offsets, **kw)
    check(gk, None, keys, None, offsets, want=(want[0], None))
    gk, gv, _ = run_segmented(torch, s, keys, offsets, values, **kw)
    check(gk, gv, keys, values, offsets, want=want)


def _case(sizes, keys, head, tail):
    """(keys, values, offsets, reference) of a call whose keys are given for [head, head + sum(sizes)) and random around."""
    offsets = _offsets(sizes, head)
    n = int(offsets[-1]) + tail
    rng = np.random.default_rng(len(sizes))
    whole = make_keys("uniform", n, rng)
    whole[head:int(offsets[-1])] = keys
    values = payload(n)
    return whole, values, offsets, expected(whole, values, offsets, n)


# ---- A. a workgroup sorts more than one segment ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _small_reuse_case():
    rng = np.random.default_rng(101)
    count = 1_500_000
    sizes = rng.integers(0, 10, size=count)
    spots = rng.choice(count, 400, replace=False)
    sizes[spots] = rng.integers(2, SMALL_MAX + 1, size=400)
    # workgroup b takes segments b and b + 2^20: a full-LDS segment in front of a tiny one, and the other way round
    for j, b in enumerate(rng.choice(count - SMALL_GRID, 64, replace=False)):
        big = SMALL_MAX if j % 2 == 0 else int(rng.integers(3000, SMALL_MAX + 1))
        little = 3 if j % 2 == 0 else int(rng.integers(2, 10))
        sizes[b], sizes[b + SMALL_GRID] = (big, little) if j % 4 < 2 else (little, big)
    assert count > SMALL_GRID and int((sizes[SMALL_GRID:] > 9).sum()) >= 16 and sizes.max() == SMALL_MAX
    total = int(sizes.sum())
    return sizes, _case(sizes, _with_duplicates(make_keys("uniform", total, rng)), 5, 9)


@pytest.mark.parametrize("ranking", RANKINGS)
def test_small_kernel_takes_a_second_segment(torch_mod, sorter, ballot_sorter, ranking):
    """1.5 M segments of 0 ... 9 keys with 400 of 2 ... 4096 keys among them: the 2^20 workgroups of the small kernel take
    the segments from id 2^20 on in a second trip of their loop, some of them a 3-key segment behind a 4096-key one."""
    sizes, (keys, values, offsets, want) = _small_reuse_case()
    assert len(sizes) > SMALL_GRID
    _both_modes(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want, offsets_off=4)


@functools.lru_cache(maxsize=1)
def _mid_reuse_case(cus):
    rng = np.random.default_rng(202)
    count = 4 * cus + 9
    i = np.arange(count)
    # list neighbours and the trips of one workgroup (list entries w, w + 2 CUs, w + 4 CUs) differ widely
    wide = (i + i // (2 * cus)) % 3 == 0
    sizes = np.where(wide, rng.integers(15000, MID_MAX + 1, size=count), rng.integers(SMALL_MAX + 1, 4400, size=count))
    sizes[rng.choice(count, count // 8, replace=False)] = rng.integers(SMALL_MAX + 1, MID_MAX + 1, size=count // 8)
    sizes[0], sizes[1], sizes[-1] = SMALL_MAX + 1, MID_MAX, MID_MAX
    sizes = list(sizes)
    for extra in (0, 1, 7, 300, SMALL_MAX, 0, 2, SMALL_MAX - 1):  # small and empty ones in between
        sizes.insert(int(rng.integers(0, len(sizes))), extra)
    sizes = np.array(sizes)
    total = int(sizes.sum())
    return sizes, _case(sizes, _with_duplicates(make_keys("uniform", total, rng)), 3, 6)


@pytest.mark.parametrize("ranking", RANKINGS)
def test_mid_kernel_takes_a_second_and_a_third_segment(torch_mod, sorter, ballot_sorter, cus, ranking):
    """More than 4 x CUs segments of 4097 ... 16384 keys: the mid kernel's 2 x CUs workgroups sort two segments each and
    some of them three, a long one behind a short one and the other way round."""
    sizes, (keys, values, offsets, want) = _mid_reuse_case(cus)
    mid_segments = int(((sizes > SMALL_MAX) & (sizes <= MID_MAX)).sum())
    assert mid_segments > 4 * cus and len(keys) // (SMALL_MAX + 1) > 2 * cus
    _both_modes(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want, keys_off=8)


LARGE_KINDS = ["uniform", "8-bit", "24-bit", "all-equal", "bytes12-constant"]  # 4, 1, 3, 0 and 2 active passes


@functools.lru_cache(maxsize=1)
def _large_reuse_case(cus):
    rng = np.random.default_rng(303)
    count = 2 * cus + cus // 4 + 3
    sizes = rng.integers(MID_MAX + 1, 20001, size=count)
    sizes[0], sizes[1], sizes[-1] = MID_MAX + 1, 20000, MID_MAX + 1
    # the kind changes from one id to the next and between the two trips of a workgroup (list entries w and w + 2 CUs)
    kinds = [LARGE_KINDS[(i + i // (2 * cus)) % len(LARGE_KINDS)] for i in range(count)]
    parts = [make_keys(kind, int(size), rng) for kind, size in zip(kinds, sizes)]
    sizes, at = list(sizes), [int(rng.integers(0, count)) for _ in range(3)]
    for where, extra in zip(at, (0, 5, 5000)):
        sizes.insert(where, extra)
        parts.insert(where, make_keys("uniform", extra, rng))
    sizes = np.array(sizes)
    return sizes, _case(sizes, np.concatenate(parts), 7, 3)


@pytest.mark.parametrize("ranking", RANKINGS)
def test_large_kernel_takes_a_second_segment_of_another_kind(torch_mod, sorter, ballot_sorter, cus, ranking):
    """More than 2 x CUs segments of 16385 ... 20000 keys whose kind changes per segment -- uniform, 8-bit, 24-bit,
    all-equal, bytes 1 and 2 constant: four, one, three, no and two active passes -- so a workgroup's second segment needs
    another pass mask, other bases and the copy back where the first did not (or the other way round)."""
    sizes, (keys, values, offsets, want) = _large_reuse_case(cus)
    large_segments = int((sizes > MID_MAX).sum())
    assert large_segments > 2 * cus and len(keys) // (MID_MAX + 1) > 2 * cus
    _both_modes(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want, values_off=16)


@pytest.mark.parametrize("segments,length", [(65536, 256), (8192, 2048), (1024, 16384)])
def test_headline_shapes(torch_mod, sorter, cus, segments, length):
    """The three in-LDS shapes README.md quotes times for (16.8 M keys each), key+value."""
    assert segments > 2 * cus
    rng = np.random.default_rng(segments)
    n = segments * length
    keys = _with_duplicates(make_keys("uniform", n, rng))
    values = payload(n)
    offsets = _offsets([length] * segments)
    gk, gv, _ = run_segmented(torch_mod, sorter, keys, offsets, values)
    check(gk, gv, keys, values, offsets)


# ---- B. list capacity -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _full_list_case(length, cus):
    rng = np.random.default_rng(length)
    k = 2 * cus + 3
    n = k * length
    keys = _with_duplicates(make_keys("uniform", n, rng))
    values = payload(n)
    offsets = _offsets([length] * k)
    return k, keys, values, offsets, expected(keys, values, offsets, n)


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("length", [SMALL_MAX + 1, MID_MAX + 1])
def test_a_list_filled_to_its_last_slot(torch_mod, sorter, ballot_sorter, cus, length, ranking):
    """Nothing but segments of 4097 (16385) keys, o[0] = 0, no tail, maxElementCount = o[last]: the mid (large) list holds
    exactly its capacity maxElementCount / 4097 (/ 16385), which is more than the kernel's grid."""
    k, keys, values, offsets, want = _full_list_case(length, cus)
    assert len(keys) // length == k == len(offsets) - 1 and k > 2 * cus and int(offsets[0]) == 0 and int(offsets[-1]) == len(keys)
    _both_modes(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, values, want)


@pytest.mark.parametrize("n", [SMALL_MAX, SMALL_MAX + 1, MID_MAX, MID_MAX + 1])
def test_one_segment_that_is_the_whole_array(torch_mod, sorter, ballot_sorter, n):
    """maxElementCount on either side of a class boundary with one segment [0, maxElementCount): the list capacities are 0
    or 1 and the mid (large) launch is recorded only from 4097 (16385) on."""
    rng = np.random.default_rng(n)
    keys = _with_duplicates(make_keys("uniform", n, rng))
    offsets = np.array([0, n], np.uint32)
    for s in (sorter, ballot_sorter):
        _both_modes(torch_mod, s, keys, offsets, payload(n))


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("key_value", [False, True])
def test_overlapping_segments_cannot_overfill_a_list(torch_mod, sorter, ballot_sorter, ranking, key_value):
    """Offsets 0, 5000, 0, 5000, ... list the mid segment [0, 5000) 64 times where the mid list has 10 slots (documented:
    slots beyond the capacity are dropped, include/vk_radix_sort.h and DESIGN.md 4.10).  A large segment in front of the
    pairs, a large and a small one behind them, all three disjoint from [0, 5000), must come out sorted -- the large list
    lies right behind the mid list -- and everything else outside [0, 5000) untouched, with STATUS_SEGMENTS_INVALID from
    the decreasing pairs.  [0, 5000) is sorted by several workgroups at once: nothing is asserted about it.  64 surplus
    list words are far fewer than the words of storage behind the lists."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    s = _pick(ranking, sorter, ballot_sorter)
    stream = torch.cuda.current_stream().cuda_stream
    s.read_sorter_status(stream)  # (clears it)
    pairs, raced, large_front, large_behind, small = 64, 5000, 20000, 17000, 300
    front = raced + large_behind + small + 50
    n = front + large_front + 33
    offsets = np.array([front, front + large_front] + [0, raced] * pairs + [raced + large_behind, raced + large_behind + small],
                       np.uint32)
    mid_cap, large_cap = n // (SMALL_MAX + 1), n // (MID_MAX + 1)
    assert pairs > 4 * mid_cap and large_cap == 2 and pairs < n // 100
    rng = np.random.default_rng(pairs)
    keys = _with_duplicates(make_keys("uniform", n, rng))
    values = payload(n) if key_value else None
    gk, gv, _ = run_segmented(torch, s, keys, offsets, values, expect_status=vrdx.STATUS_SEGMENTS_INVALID)
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


# ---- C. key and payload patterns in every size class ----------------------------------------------------------------------

PATTERNS = (["all-sentinel", "eighth-sentinel", "few-distinct", "bytes12-constant", "byte0-only", "byte3-only"]
            + [f"digit{p}-constant" for p in range(4)])
PATTERN_SIZES = [3000, 9000, 2 * TILE + 5, 3 * TILE - 1]  # small, mid, large with a short last tile, large one short of full
PATTERN_CASES = ([(kind, size) for kind in PATTERNS for size in PATTERN_SIZES]
                 # one digit fills the first tile: the same as a constant digit below 16384 keys, so the large sizes only
                 + [(f"tile-digit{p}", size) for p in range(4) for size in PATTERN_SIZES if size > TILE])


@pytest.mark.parametrize("kind,size", PATTERN_CASES)
def test_key_patterns_in_every_size_class(torch_mod, sorter, ballot_sorter, kind, size):
    """One segment of the given kind between two short uniform ones, keys-only and key+value (payloads with the top bit
    set, a 0xFFFFFFFF and a 0 among them), both ranking forms."""
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{size}".encode()))
    sizes = [40, size, 11]
    parts = [make_keys("uniform", 40, rng), make_keys(kind, size, rng), make_keys("uniform", 11, rng)]
    keys, values, offsets, want = _case(sizes, np.concatenate(parts), 6, 5)
    for s in (sorter, ballot_sorter):
        _both_modes(torch_mod, s, keys, offsets, values, want)


# ---- D. a bound far above what the offsets use ----------------------------------------------------------------------------

@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("where", ["front", "far-end"])
def test_a_large_bound_and_a_small_use(torch_mod, sorter, ballot_sorter, where, ranking):
    """maxElementCount = 40 M with segments over some 260000 keys at one end of it (tail of 3 at the far end): the scratch
    of a large segment is the same index range of the storage as its keys, here its last (first) bytes."""
    n = 40_000_003
    rng = np.random.default_rng(40)
    sizes = [300, 150000, 0, 9000, 17, SMALL_MAX, 40000, MID_MAX, 2, 1000, 33000, 1]
    rng.shuffle(sizes)
    total = int(np.sum(sizes))
    head = 3 if where == "front" else n - 3 - total
    offsets = _offsets(sizes, head)
    assert int(offsets[-1]) == (n - 3 if where == "far-end" else 3 + total) and 100 * total < n
    keys = np.full(n, 0x01234567, np.uint32)
    lo, hi = max(head - 5000, 0), min(head + total + 5000, n)
    keys[lo:hi] = _with_duplicates(make_keys("uniform", hi - lo, rng))
    _both_modes(torch_mod, _pick(ranking, sorter, ballot_sorter), keys, offsets, payload(n))


# ---- E. tile edges of the large path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [0, 1, 2, 3])
@pytest.mark.parametrize("size", [TILE + 1, TILE + 255, TILE + 256, TILE + 257, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1,
                                  5 * TILE + 1])
def test_large_path_tile_edges(torch_mod, sorter, ballot_sorter, size, start):
    """One large segment whose last tile holds 1 ... 16384 keys (1 ... 255: one chunk, fifteen waves idle), starting at
    every 16-byte phase, key+value, both ranking forms."""
    rng = np.random.default_rng(size * 4 + start)
    n = start + size + 5
    keys = _with_duplicates(make_keys("uniform", n, rng))
    values = payload(n)
    offsets = np.array([start, start + size], np.uint32)
    want = expected(keys, values, offsets, n)
    for s in (sorter, ballot_sorter):
        gk, gv, _ = run_segmented(torch_mod, s, keys, offsets, values)
        check(gk, gv, keys, values, offsets, want=want)


# ---- F. captured graph, keys-only -----------------------------------------------------------------------------------------

def test_captured_graph_keys_only_moves_segments_across_the_classes(torch_mod, sorter, cus):
    """A keys-only call captured on a segmentation of mostly small segments, replayed on one with more than 2 x CUs mid
    segments (every one of them was small, large or empty at the capture) and back: the grids are those of the capture, the
    classes and the lists are made anew on the device at every replay."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    rng = np.random.default_rng(78)
    mids = 2 * cus + 8
    count = mids + 40
    first = [40000] * 4 + [5000] * 20 + [0] * 16 + [300] * (count - 40)
    second = list(rng.integers(SMALL_MAX + 1, 6000, size=mids)) + [20000] * 10 + [17] * 20 + [0] * 10
    third = [MID_MAX + 1] * 30 + [MID_MAX] * 10 + [3] * (count - 40)
    offsets_list = []
    for sizes in (first, second, third):
        sizes = [int(x) for x in sizes]
        rng.shuffle(sizes)
        offsets_list.append(_offsets(sizes, 1))
    n = max(int(o[-1]) for o in offsets_list) + 10
    assert len({len(o) for o in offsets_list}) == 1 and mids > 2 * cus
    dk, do = to_device(torch, np.zeros(n, np.uint32)), to_device(torch, offsets_list[0])
    storage = torch.empty(sorter.storage_requirements(n).size, dtype=torch.uint8, device="cuda")
    vrdx.sort_segments(sorter, dk, do, storage=storage)  # one eager call first (test_sort_gpu.py explains why)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort_segments(sorter, dk, do, storage=storage)
    for replay, offsets in enumerate(offsets_list + offsets_list[:2]):
        keys = make_keys("uniform" if replay % 2 == 0 else "24-bit", n, rng)
        dk.copy_(to_device(torch, keys))
        do.copy_(to_device(torch, offsets))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(to_host(dk), None, keys, None, offsets)
        assert sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0) == 0
