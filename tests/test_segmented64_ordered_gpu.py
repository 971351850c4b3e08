"""GPU tests of the key orders of the segmented sort of 64-bit keys (vrdxHipCmdSortSegmented64Ordered[KeyValue],
vulkan_radix_sort_amd.sort_segments64 with `order` / `descending`), through the C ABI and bit for bit against the reference
of tests/key_order_cases.py: np.lexsort((T(keys), segment id)).  Every call runs between guard words
(tests/guarded_call.py).  Segment sizes sit at the edges of the three size classes of both forms: 4096 | 4097, keys-only
16384 | 16385, key+value 8192 | 8193, large segments that end inside a tile of 8192 and that are whole tiles."""
import functools

import numpy as np
import pytest

from guarded_call import ballot_sorter, guarded_call, sorter, torch_mod  # noqa: F401
from key_order_cases import (DIRECTIONS, ORDERS, SIGN, all_ones_key, assert_same, expected_segments, order_word, payload,
                             segment_case)
from segmented64_cases import run_segmented64

pytestmark = pytest.mark.gpu


def run_segmented64_ordered(torch, s, keys, offsets, values, word, *, expect_status=0, storage_out=None, **kw):
    """One segmented call with the order word `word` and maxElementCount = len(keys) (guarded_call: keys_off, values_off,
    storage_off, pool, expect_refused).  Unless the call is refused, the failure word and the sorter's sticky word must both be
    expect_status afterwards.  Returns keys and values as the device left them."""
    got = guarded_call(torch, s, keys, values, offsets=offsets, order=word, tail=8 * 256, expect_status=expect_status,
                       recorded=True, sticky=expect_status, **kw)
    if storage_out is not None:
        storage_out.append(got.storage)
    return got.keys, got.values

# both in-LDS kernels at their edges for both forms, the large kernel with one tile plus one key (key+value), two tiles plus
# one key (keys-only), a last tile that is ragged, exactly two tiles (key+value) and exactly three (both)
EDGE_SIZES = [0, 1, 2, 4096, 4097, 8192, 8193, 16384, 16385, 20001, 24576]
CASES = [(o, d) for o in ORDERS for d in DIRECTIONS]
IDS = [f"{o}-{'descending' if d else 'ascending'}" for o, d in CASES]


@functools.lru_cache(maxsize=None)
def _case(builder, sizes, order, descending):
    keys, values, offsets = segment_case(builder, list(sizes), order, descending)
    want = expected_segments(keys, values, offsets, len(keys), order, descending)
    for a in (keys, values, offsets) + want:
        a.setflags(write=False)
    return keys, values, offsets, want


def _both_forms(torch, s, builder, sizes, order, descending, **kw):
    keys, values, offsets, want = _case(builder, tuple(sizes), order, descending)
    word = order_word(order, descending)
    what = f"{builder} {order} descending={descending}"
    got = run_segmented64_ordered(torch, s, keys, offsets, None, word, **kw)
    assert_same(*got, want, what + " keys-only")
    got = run_segmented64_ordered(torch, s, keys, offsets, values, word, **kw)
    assert_same(*got, want, what + " key+value")


@pytest.mark.parametrize("builder", ["float-specials", "duplicates", "mixed-int"])
@pytest.mark.parametrize("order,descending", CASES, ids=IDS)
def test_every_order_and_direction_at_the_class_edges(torch_mod, sorter, order, descending, builder):
    _both_forms(torch_mod, sorter, builder, EDGE_SIZES, order, descending)


@pytest.mark.parametrize("order,descending", [("float64", True), ("int64", False)], ids=["float64-descending", "int64-ascending"])
def test_the_ballot_ranking_forms(torch_mod, ballot_sorter, order, descending):
    _both_forms(torch_mod, ballot_sorter, "float-specials", EDGE_SIZES, order, descending)


@pytest.mark.parametrize("order,descending", CASES, ids=IDS)
def test_plus_and_minus_x_in_every_class(torch_mod, sorter, order, descending):
    """+x and -x differ in one raw bit; as float64 their T differ in up to 63: what varies has to be taken over T(key)"""
    _both_forms(torch_mod, sorter, "plus-minus-x", [1000, 4097, 8193, 16385, 20001], order, descending)


@pytest.mark.parametrize("order,descending", CASES, ids=IDS)
def test_the_key_that_ties_with_the_pads(torch_mod, sorter, order, descending):
    """copies of the key T maps to all ones, with distinct values, at the end of segments that are no multiple of the tile
    or of a wave's 256-key chunk: they stay in front of the pads, in input order"""
    sizes = [3, 257, 1000, 4095, 4097, 8191, 8193, 16383, 16385, 20001]
    _both_forms(torch_mod, sorter, "ones-in-T", sizes, order, descending)
    keys, values, offsets, want = _case("ones-in-T", tuple(sizes), order, descending)
    assert (keys == all_ones_key(order, descending)).sum() > len(sizes) * 2
    # a segment of nothing but that key
    n = 5000
    ones = np.full(n, all_ones_key(order, descending), np.uint64)
    got = run_segmented64_ordered(torch_mod, sorter, ones, [0, 300, 4800, n], payload(n), order_word(order, descending))
    assert_same(*got, (ones, payload(n)))


@pytest.mark.parametrize("order,descending", [("float64", True), ("int64", False)], ids=["float64-descending", "int64-ascending"])
def test_a_workgroup_sorts_several_segments_in_a_row(torch_mod, sorter, order, descending):
    """2^20 + 40 segments: the small launch's 2^20 workgroups take the last forty, real ones of up to 700 keys, in a second
    trip, with the order word still in place"""
    rng = np.random.default_rng(11)
    sizes = np.concatenate([rng.integers(0, 3, size=1 << 20), rng.integers(100, 700, size=40)])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    keys[1::3] = keys[0:-1:3][:len(keys[1::3])]   # neighbours with equal keys
    keys[::5] |= SIGN
    values = payload(n)
    want = expected_segments(keys, values, offsets, n, order, descending)
    word = order_word(order, descending)
    assert_same(*run_segmented64_ordered(torch_mod, sorter, keys, offsets, None, word), want)
    assert_same(*run_segmented64_ordered(torch_mod, sorter, keys, offsets, values, word), want)


def test_bad_offsets_are_left_alone(torch_mod, sorter):
    import vulkan_radix_sort_amd as vrdx
    keys, values, _, _ = _case("float-specials", (30000,), "float64", True)
    n = len(keys)
    offsets = np.array([100, 1100, 21100, 9000, 9000, n + 5000], np.uint32)   # decreasing, then ending behind maxElementCount
    want = expected_segments(keys, values, offsets, n, "float64", True)
    assert np.array_equal(want[0][21100:], keys[21100:])
    for v in (None, values):
        got = run_segmented64_ordered(torch_mod, sorter, keys, offsets, v, order_word("float64", True),
                                      expect_status=vrdx.STATUS_SEGMENTS_INVALID)
        assert_same(*got, want)


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_the_unsigned_order_is_the_twin(torch_mod, sorter, key_value):
    """VRDX_HIP_KEY_UINT64 records what vrdxHipCmdSortSegmented64[KeyValue] records: the same arrays, the same header words"""
    keys, values, offsets, want = _case("uniform", tuple(EDGE_SIZES), "uint64", False)
    values = values if key_value else None
    ordered = []
    tk, tv, twin = run_segmented64(torch_mod, sorter, keys, offsets, values)
    got = run_segmented64_ordered(torch_mod, sorter, keys, offsets, values, 0, storage_out=ordered)
    assert_same(*got, (tk, tv))
    assert_same(*got, want)
    assert torch_mod.equal(twin[:16], ordered[0][:16]), "header words 0-3"


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("word", [3, 0x200, 0x103, 0x80000002])
def test_a_word_that_is_no_order_is_refused(torch_mod, sorter, word, key_value):
    import vulkan_radix_sort_amd as vrdx
    keys, values, offsets, _ = _case("float-specials", (1000, 4097), "float64", False)
    values = values if key_value else None
    pool = vrdx.QueryPool(15)
    got = run_segmented64_ordered(torch_mod, sorter, keys, offsets, values, word, pool=pool, expect_refused=True)
    assert_same(*got, (keys, values), "a refused call changed the arrays")
    ts = pool.results_ns(0, 15)
    assert len(ts) == 15 and all(b >= a for a, b in zip(ts, ts[1:]))
    pool.destroy()


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
def test_timestamps_in_all_15_slots(torch_mod, sorter, key_value):
    import vulkan_radix_sort_amd as vrdx
    keys, values, offsets, want = _case("float-specials", tuple(EDGE_SIZES), "float64", True)
    pool = vrdx.QueryPool(15)
    got = run_segmented64_ordered(torch_mod, sorter, keys, offsets, values if key_value else None, order_word("float64", True),
                                  pool=pool)
    assert_same(*got, want)
    ts = pool.results_ns(0, 15)
    print("segmented64 ordered slots (ns):", ts)
    assert len(ts) == 15 and ts[0] == 0 and all(b >= a for a, b in zip(ts, ts[1:])), ts
    assert all(t == ts[4] for t in ts[4:]), ts
    pool.destroy()


@pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_a_captured_call_replays_on_another_segmentation(torch_mod, sorter, descending, key_value):
    torch = torch_mod
    order = "float64"
    word = order_word(order, descending)
    first = segment_case("float-specials", [5, 4097, 20001, 300, 8193], order, descending, tag="capture")
    n, segments = len(first[0]), len(first[2]) - 1
    dk = torch.zeros(n, dtype=torch.int64, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
    do = torch.zeros(segments + 1, dtype=torch.int32, device="cuda")
    storage = torch.empty(sorter.storage_requirements64(n, key_value).size, dtype=torch.uint8, device="cuda")

    def record():
        stream = torch.cuda.current_stream().cuda_stream
        if key_value:
            sorter.cmd_sort_segmented64_ordered_key_value(stream, n, segments, do.data_ptr(), 0, dk.data_ptr(), 0, dv.data_ptr(),
                                                          0, word, storage.data_ptr(), 0)
        else:
            sorter.cmd_sort_segmented64_ordered(stream, n, segments, do.data_ptr(), 0, dk.data_ptr(), 0, word,
                                                storage.data_ptr(), 0)

    def load(keys, values, offsets):
        dk.copy_(torch.from_numpy(keys.view(np.int64).copy()))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        do.copy_(torch.from_numpy(np.asarray(offsets, np.uint32).view(np.int32).copy()))
        torch.cuda.synchronize()

    load(*first)
    record()  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        record()
    stream = torch.cuda.current_stream().cuda_stream
    # the same segmentCount, other keys, other sizes in other classes
    keys, values = first[0][::-1].copy(), first[1]
    offsets = np.array([0, 9000, 9002, 26000, 30100, n - 3], np.uint32)
    assert len(offsets) == segments + 1 and offsets[-1] <= n
    load(keys, values, offsets)
    g.replay()
    torch.cuda.synchronize()
    assert_same(dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32) if key_value else None,
                expected_segments(keys, values, offsets, n, order, descending))
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0
    assert sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_sort_segments64_of_float64_tensors(torch_mod, sorter, descending):
    """the Python front end on a torch.float64 tensor, against torch.sort segment by segment (no NaNs, no zeros)"""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    keys, values, offsets = segment_case("float-values", [0, 1, 700, 4097, 9000, 17000], "float64", descending, tag="torch")
    b, e = int(offsets[0]), int(offsets[-1])
    keys[:b] = np.array([1.0]).view(np.uint64)[0]
    keys[e:] = np.array([-1.0]).view(np.uint64)[0]
    t = torch.from_numpy(keys.view(np.float64).copy()).cuda()
    do = torch.from_numpy(offsets.view(np.int32).copy()).cuda()
    dk, dv = t.clone(), torch.arange(len(keys), dtype=torch.int32, device="cuda")
    vrdx.sort_segments64(sorter, dk, do, dv, order="float64", descending=descending)
    torch.cuda.synchronize()
    want_k, want_v = t.clone(), torch.arange(len(keys), dtype=torch.int64, device="cuda")
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        lo, hi = int(lo), int(hi)
        sorted_keys, index = torch.sort(t[lo:hi], stable=True, descending=descending)
        want_k[lo:hi] = sorted_keys
        want_v[lo:hi] = index + lo
    assert torch.equal(dk.view(torch.int64), want_k.view(torch.int64)) and torch.equal(dv.to(torch.int64), want_v)
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0
