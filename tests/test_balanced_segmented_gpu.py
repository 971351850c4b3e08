"""GPU tests of the balanced segmented sort (vrdxHipCmdBalancedSortSegmented[KeyValue]), through the
shared guarded call (tests/balanced_guarded_call.py): guard bytes around keys, values and offsets, bands around the poisoned
storage requirement.  Every case of tests/balanced_segmented_cases.py, sized by the CU count the describe call reports, is
compared bit for bit with np.lexsort((keys, segment id)) AND with what vrdxHipCmdSortSegmented[KeyValue] returns on the same
input; the failure word is 0; and vrdxHipReadBalancedSplit must return the model's four words, so a build that sends every
segment down the one-workgroup kernel fails.  Values are random, never the index."""
import numpy as np
import pytest

import balanced_segmented_cases as model
from balanced_guarded_call import (POISON_BYTE, ballot_sorter, balanced_call, sorter, to_device, to_host, torch_mod,  # noqa: F401
                                   twin_call)

pytestmark = pytest.mark.gpu

CASE_NAMES = ("n65536", "n65537", "k_quarter", "k_half", "one_among", "one_among_spread", "two_tiles", "neighbours0",
              "neighbours1", "neighbours2", "neighbours3", "passes")
BOTH_MODES_UP_TO = 1 << 21   # cases of more elements run key+value only here; test_both_rankings_and_modes has keys-only


@pytest.fixture(scope="module")
def cus(sorter):
    info = sorter.describe_balanced_segmented_plan(model.MAX_ELEMENTS, 1, False)
    assert info.name == "balanced" and info.pieceCap > info.spreadCap > 0
    return info.pieceCap - info.spreadCap   # pieceCap = min(CUs, N / 16384) + spreadCap


@pytest.fixture(scope="module")
def cases(cus):
    got = model.cases(cus)
    assert tuple(got) == CASE_NAMES
    return got


@pytest.fixture(scope="module")
def references():
    return {}


def reference_of(references, cases, name):
    if name not in references:   # computed once, shared, left unchanged
        references[name] = model.reference(*cases[name])
        for a in references[name]:
            a.setflags(write=False)
    return references[name]


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def check(torch, sorter, cus, case, want, key_value, twin=True, **kw):
    keys, values, offsets = case
    vals = values if key_value else None
    n = len(keys)
    got = balanced_call(torch, sorter, keys, vals, offsets, **kw)
    words = sorter.read_balanced_split(stream_of(torch), got.storage.data_ptr(), n, kw.get("storage_off", 0))
    assert np.array_equal(got.keys, want[0]), np.flatnonzero(got.keys != want[0])[:8]
    assert not key_value or np.array_equal(got.values, want[1]), np.flatnonzero(got.values != want[1])[:8]
    expect = model.split_words(offsets, cus) if n > model.SPREAD_FROM else (0, 0, 0, 0)
    assert (words.listedSegments, words.spreadSegments, words.pieces, words.pieceKeys) == expect
    assert sorter.read_plan_verdict(stream_of(torch), got.storage.data_ptr(), kw.get("storage_off", 0)) == 0   # VERDICT_NONE
    if twin:
        same = twin_call(torch, sorter, keys, vals, offsets, **kw)
        assert np.array_equal(got.keys, same.keys) and (not key_value or np.array_equal(got.values, same.values))
    return got


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case_against_lexsort_the_twin_and_the_model_s_split(torch_mod, sorter, cus, cases, references, name):
    want = reference_of(references, cases, name)
    check(torch_mod, sorter, cus, cases[name], want, True)
    if len(cases[name][0]) <= BOTH_MODES_UP_TO:
        check(torch_mod, sorter, cus, cases[name], want, False)


@pytest.mark.parametrize("name", ["n65537", "neighbours2", "passes"])
def test_both_rankings_and_modes(torch_mod, sorter, ballot_sorter, cus, cases, references, name):
    want = reference_of(references, cases, name)
    for which in (sorter, ballot_sorter):
        for key_value in (False, True):
            check(torch_mod, which, cus, cases[name], want, key_value, twin=which is ballot_sorter)


@pytest.mark.parametrize("keys_off", [0, 4, 8, 12])
def test_the_keys_array_at_every_alignment(torch_mod, sorter, cus, cases, references, keys_off):
    want = reference_of(references, cases, "neighbours1")
    check(torch_mod, sorter, cus, cases["neighbours1"], want, True, twin=False, keys_off=keys_off, values_off=(keys_off + 8) % 16,
          offsets_off=4, storage_off=16 * (keys_off // 4))


def test_an_all_equal_spread_segment_leaves_its_scratch_range_alone(torch_mod, sorter, cus, cases, references):
    keys, values, offsets = cases["passes"]
    n = len(keys)
    got = check(torch_mod, sorter, cus, cases["passes"], reference_of(references, cases, "passes"), True, twin=False)
    where = model.layout(n, cus, address=got.storage.data_ptr())
    assert where["valuesScratch"] + 4 * n <= got.required
    at = model.PASS_KINDS.index("equal")
    b, e = int(offsets[at]), int(offsets[at + 1])
    storage = got.storage.cpu().numpy()
    for name in ("keysScratch", "valuesScratch"):
        assert (storage[where[name] + 4 * b:where[name] + 4 * e] == POISON_BYTE).all(), name
        # (and a segment of uniform keys went through its range: the offsets are the device's)
        first = storage[where[name] + 4 * int(offsets[0]):where[name] + 4 * int(offsets[1])]
        assert (first != POISON_BYTE).mean() > 0.9, name


def test_up_to_65536_elements_the_call_records_the_twin(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    rng = np.random.default_rng(65536)
    for offsets in ([0, 65536], [3, 20000, 20010, 45000, 65530]):
        keys = rng.integers(0, 1 << 32, 65536, dtype=np.uint64).astype(np.uint32)
        values = rng.integers(0, 1 << 32, 65536, dtype=np.uint64).astype(np.uint32)
        want = model.reference(keys, values, offsets)
        for vals in (None, values):
            info = sorter.describe_balanced_segmented_plan(65536, len(offsets) - 1, vals is not None)
            assert (info.name, info.launches, info.spreadCap, info.pieceCap) == ("twin", 4, 0, 0)
            pools = [vrdx.QueryPool(15), vrdx.QueryPool(15)]
            got = balanced_call(torch_mod, sorter, keys, vals, offsets, pool=pools[0])
            same = twin_call(torch_mod, sorter, keys, vals, offsets, pool=pools[1])
            assert np.array_equal(got.keys, want[0]) and np.array_equal(same.keys, want[0])
            assert vals is None or (np.array_equal(got.values, want[1]) and np.array_equal(same.values, want[1]))
            # the storage, byte for byte -- but for the order of the ids in the two lists, which workgroups append in the
            # order they happen to run in
            ours, theirs = got.storage.cpu().numpy().copy(), same.storage.cpu().numpy().copy()
            where = model.layout(65536, 256, address=got.storage.data_ptr())
            assert got.storage.data_ptr() % 128 == same.storage.data_ptr() % 128
            for name, cap in (("midList", 65536 // 4097), ("largeList", 65536 // 16385)):
                for raw in (ours, theirs):
                    ids = raw[where[name]:where[name] + 4 * cap].view(np.uint32)
                    ids[:] = np.sort(ids)
            differ = np.flatnonzero(ours != theirs)
            assert differ.size == 0, f"the storage bytes differ from the twin's at {differ[:8].tolist()} ({differ.size} bytes)"
            for pool in pools:   # the same slots: fill, small, mid, large, the rest coincide
                ts = pool.results_ns()
                assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:])) and len(set(ts[4:])) == 1 and ts[4] > ts[0]
                pool.destroy()


def test_empty_calls_touch_nothing(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1 << 32, 70000, dtype=np.uint64).astype(np.uint32)
    values = keys[::-1].copy()
    for vals in (None, values):
        for offsets, count in (([5], 70000), ([0, 70000], 0)):   # no segments | no elements
            pool = vrdx.QueryPool(15)
            got = balanced_call(torch_mod, sorter, keys, vals, offsets, count=count, pool=pool, keep_before=True, recorded=False)
            assert np.array_equal(got.keys, keys) and (vals is None or np.array_equal(got.values, vals))
            assert torch_mod.equal(got.storage, got.before), "an empty call wrote to the storage"
            ts = pool.results_ns()
            assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
            pool.destroy()
    assert sorter.describe_balanced_segmented_plan(70000, 0, False).name == "none"
    assert sorter.describe_balanced_segmented_plan(0, 3, False).name == "none"
    assert sorter.read_sorter_status(stream_of(torch_mod)) == 0


def test_bad_offsets_inside_a_spread_segment(torch_mod, sorter, cus):
    """a decreasing pair and an overlap inside the range of a spread segment, an end behind the bound: the invalid bit is
    raised, the guard bytes hold (the guarded call), the disjoint valid segments are sorted and nothing else moves"""
    import vulkan_radix_sort_amd as vrdx
    rng = np.random.default_rng(404)
    n = 300000
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    values = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    stream = stream_of(torch_mod)
    sorter.read_sorter_status(stream)   # (clears the word)
    # [0, 70000) spread | (70000, 60000) decreasing | [60000, 140000) overlaps the first | [140000, 215000) disjoint, spread |
    # [215000, 215100) | (215100, n + 7) ends behind the bound
    offsets = [0, 70000, 60000, 140000, 215000, 215100, n + 7]
    for vals in (None, values):
        got = balanced_call(torch_mod, sorter, keys, vals, offsets, expect_status=vrdx.STATUS_SEGMENTS_INVALID,
                            sticky=vrdx.STATUS_SEGMENTS_INVALID)
        for b, e in ((140000, 215000), (215000, 215100)):
            order = np.argsort(keys[b:e], kind="stable")
            assert np.array_equal(got.keys[b:e], keys[b:e][order]), (b, e)
            assert vals is None or np.array_equal(got.values[b:e], vals[b:e][order]), (b, e)
        assert np.array_equal(got.keys[215100:], keys[215100:]) and (vals is None or np.array_equal(got.values[215100:], vals[215100:]))
        words = sorter.read_balanced_split(stream, got.storage.data_ptr(), n)
        assert words.listedSegments == 3 and words.spreadSegments >= 1
    # a decreasing pair between valid segments: [150000, 149000) is refused, [149000, 150000) overlaps the spread segment in
    # front of it; the three disjoint valid segments are sorted as ever
    offsets = [0, 70000, 150000, 149000, 150000, 230000, n]
    got = balanced_call(torch_mod, sorter, keys, values, offsets, expect_status=vrdx.STATUS_SEGMENTS_INVALID,
                        sticky=vrdx.STATUS_SEGMENTS_INVALID)
    for b, e in ((0, 70000), (150000, 230000), (230000, n)):
        order = np.argsort(keys[b:e], kind="stable")
        assert np.array_equal(got.keys[b:e], keys[b:e][order]) and np.array_equal(got.values[b:e], values[b:e][order]), (b, e)


def test_timestamps_of_all_15_slots(torch_mod, sorter, cus, cases):
    import vulkan_radix_sort_amd as vrdx
    keys, values, offsets = cases["neighbours0"]
    for vals in (None, values):
        info = sorter.describe_balanced_segmented_plan(len(keys), len(offsets) - 1, vals is not None)
        assert (info.name, info.launches) == ("balanced", 18)
        pool = vrdx.QueryPool(15)
        balanced_call(torch_mod, sorter, keys, vals, offsets, pool=pool)
        ts = pool.results_ns()
        assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:])), ts
        assert all(ts[i] > ts[i - 1] for i in range(1, 14)), ts   # a launch at least ends every slot 1 ... 13
        assert ts[14] == ts[13], ts
        pool.destroy()


def test_describe_balanced_segmented_plan(sorter, cus):
    for n, segments in ((65537, 1), (1 << 22, 4), (model.MAX_ELEMENTS, 100000), (1 << 31, 3)):
        for key_value in (False, True):
            info = sorter.describe_balanced_segmented_plan(n, segments, key_value)
            bound = min(n, model.MAX_ELEMENTS)   # the clamp
            assert (info.name, info.launches, info.spreadFrom, info.spreadShares, info.minPieceKeys) == ("balanced", 18, 65536, 3, 16384)
            assert (info.spreadCap, info.pieceCap) == (model.spread_cap(bound, cus), model.piece_cap(bound, cus))


def test_storage_left_behind_by_other_sorts_and_left_to_them(torch_mod, sorter, cus, cases, references):
    """the storage reused behind an MSD-size sort, a chunked range sort and the twin, and each of those behind this call"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = stream_of(torch)
    rng = np.random.default_rng(8400)
    big = 8_400_000
    flat = rng.integers(0, 1 << 32, big, dtype=np.uint64).astype(np.uint32)
    flat_sorted = np.sort(flat)
    assert sorter.describe_plan(big, False).name == "msd"
    keys, values, offsets = cases["passes"]
    want = reference_of(references, cases, "passes")
    n = len(keys)
    storage = torch.full((sorter.key_value_storage_requirements(big).size,), 0xA5, dtype=torch.uint8, device="cuda")
    d_flat, d_keys, d_values = to_device(torch, flat), to_device(torch, keys), to_device(torch, values)
    d_offsets = to_device(torch, np.asarray(offsets, dtype=np.uint32))
    segments = len(offsets) - 1

    def others():
        def msd():
            d_flat.copy_(to_device(torch, flat))
            sorter.cmd_sort(stream, big, d_flat.data_ptr(), 0, storage.data_ptr(), 0)
            return lambda: np.array_equal(to_host(d_flat), flat_sorted)

        def chunked():
            d_flat.copy_(to_device(torch, flat))
            sorter.cmd_range_sort(stream, big, d_flat.data_ptr(), 0, 8, 24, storage.data_ptr(), 0)
            field = (flat >> np.uint32(8)) & np.uint32(0xFFFF)
            return lambda: np.array_equal(to_host(d_flat), flat[np.argsort(field, kind="stable")])

        def twin():
            d_keys.copy_(to_device(torch, keys))
            d_values.copy_(to_device(torch, values))
            sorter.cmd_sort_segmented_key_value(stream, n, segments, d_offsets.data_ptr(), 0, d_keys.data_ptr(), 0,
                                                d_values.data_ptr(), 0, storage.data_ptr(), 0)
            return lambda: np.array_equal(to_host(d_keys), want[0]) and np.array_equal(to_host(d_values), want[1])
        return (msd, chunked, twin)

    def balanced():
        d_keys.copy_(to_device(torch, keys))
        d_values.copy_(to_device(torch, values))
        sorter.cmd_balanced_sort_segmented_key_value(stream, n, segments, d_offsets.data_ptr(), 0, d_keys.data_ptr(), 0,
                                                     d_values.data_ptr(), 0, storage.data_ptr(), 0)
        torch.cuda.synchronize()
        words = sorter.read_balanced_split(stream, storage.data_ptr(), n)
        assert (words.listedSegments, words.spreadSegments, words.pieces, words.pieceKeys) == model.split_words(offsets, cus)
        assert np.array_equal(to_host(d_keys), want[0]) and np.array_equal(to_host(d_values), want[1])
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0 and sorter.read_plan_verdict(stream, storage.data_ptr(), 0) == 0

    for other in others():
        right = other()
        torch.cuda.synchronize()
        assert right(), other.__name__
        balanced()                     # behind it
        right = other()                # and it behind this call
        torch.cuda.synchronize()
        assert right(), other.__name__
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


def test_one_captured_call_replays_on_other_segmentations(torch_mod, sorter, cus):
    """spread to none, none to spread, other pieces: the same segmentCount, the offsets rewritten between replays"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    stream = stream_of(torch)
    n = 300000
    rng = np.random.default_rng(300000)
    dk = torch.zeros(n, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda")
    do = torch.tensor([0, 100000, 200000, 300000], dtype=torch.int32, device="cuda")   # captured: three spread segments
    storage = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
    vrdx.sort_segments_balanced(sorter, dk, do, values=dv, storage=storage)   # one eager call first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vrdx.sort_segments_balanced(sorter, dk, do, values=dv, storage=storage)
    replays = ([0, 60000, 120000, 180000],      # none spread (three listed)
               [0, 250000, 260000, 300000],     # one spread, other pieces
               [5, 70001, 140001, 299999],      # three spread again, odd bounds
               [0, 100, 200, 300])              # nothing listed
    spread_seen = []
    for offsets in replays:
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        values = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        dk.copy_(torch.from_numpy(keys.view(np.int32)))
        dv.copy_(torch.from_numpy(values.view(np.int32)))
        do.copy_(torch.tensor(offsets, dtype=torch.int32))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = model.reference(keys, values, offsets)
        assert np.array_equal(to_host(dk), want[0]) and np.array_equal(to_host(dv), want[1]), offsets
        words = sorter.read_balanced_split(stream, storage.data_ptr(), n)
        assert (words.listedSegments, words.spreadSegments, words.pieces, words.pieceKeys) == model.split_words(offsets, cus), offsets
        spread_seen.append(words.spreadSegments)
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert spread_seen[0] == 0 and spread_seen[-1] == 0 and spread_seen[1] >= 1 and spread_seen[2] >= 1
    assert sorter.read_sorter_status(stream) == 0


def test_the_front_end_against_torch_sort_per_segment(torch_mod, sorter, cus):
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    rng = np.random.default_rng(11)
    n, offsets = 200000, [0, 90000, 95000, 95000, 200000]
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[:90000] &= np.uint32(0xFF00FF)   # (many equal keys: stability shows in the values)
    values = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for with_values in (True, False):
        dk, dv = to_device(torch, keys), to_device(torch, values) if with_values else None
        do = torch.tensor(offsets, dtype=torch.int32, device="cuda")
        want_k, want_v = dk.clone(), dv.clone() if with_values else None
        for b, e in zip(offsets, offsets[1:]):
            order = torch.sort(dk[b:e].to(torch.int64) & 0xFFFFFFFF, stable=True).indices
            want_k[b:e] = dk[b:e][order]
            if with_values:
                want_v[b:e] = dv[b:e][order]
        storage = vrdx.sort_segments_balanced(sorter, dk, do, values=dv)
        assert torch.equal(dk, want_k) and (not with_values or torch.equal(dv, want_v))
        req = sorter.key_value_storage_requirements(n) if with_values else sorter.storage_requirements(n)
        assert storage.numel() == req.size
        words = sorter.read_balanced_split(stream_of(torch), storage.data_ptr(), n)
        assert (words.listedSegments, words.spreadSegments) == model.split_words(offsets, cus)[:2] == (2, 2)
