"""GPU: vrdxHipCmdOrderedSortSegmented[KeyValue] -- int32, float32 and descending orders of the segmented 32-bit sort -- bit
for bit against np.lexsort((T(keys), segment id)) (tests/key_order32_cases.py), between guard bytes
(tests/ordered_guarded_call.py): every order, direction and mode over segments of every size class and either side of the
class bounds; the key patterns that decide how many passes the large class runs; more segments than resident workgroups; bad
offsets; alignments; order word 0 against the twin and refused words; graph replay on another segmentation; the torch front
end."""
import numpy as np
import pytest

from key_order32_cases import (DIRECTIONS, ORDERS, TILE, assert_same, expected_segments, order_word, segment_case)
from ordered_guarded_call import ballot_sorter, ordered_call, sorter, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 4095, 4096, 4097, 16383, 16384, 16385]
LARGE = 3 * TILE + 1234   # three full tiles of the large kernel and a partial one
MODES = pytest.mark.parametrize("key_value", [False, True], ids=["keys", "pairs"])
EVERY_ORDER = pytest.mark.parametrize("order,descending", [(o, d) for o in ORDERS for d in DIRECTIONS],
                                      ids=[f"{o}-{'descending' if d else 'ascending'}" for o in ORDERS for d in DIRECTIONS])


def _builder(order):
    return {"uint32": "duplicates", "int32": "mixed-int", "float32": "float-specials"}[order]


def _check(torch, sorter, builder, sizes, order, descending, modes=(False, True), tag="", **kw):
    keys, values, offsets = segment_case(builder, sizes, order, descending, tag)
    want = expected_segments(keys, values, offsets, len(keys), order, descending)
    for key_value in modes:
        got = ordered_call(torch, sorter, keys, values if key_value else None, offsets=offsets,
                           order=order_word(order, descending), **kw)
        assert_same(got.keys, got.values, want, f"{builder} {order} {descending} {'pairs' if key_value else 'keys'} {kw}")


@EVERY_ORDER
def test_every_order_direction_and_mode_at_every_size_class(torch_mod, sorter, order, descending):
    _check(torch_mod, sorter, _builder(order), SIZES + [LARGE], order, descending)
    assert sorter.read_sorter_status(torch_mod.cuda.current_stream().cuda_stream) == 0


@EVERY_ORDER
@pytest.mark.parametrize("builder", ["all-equal", "one-byte", "three-bytes", "plus-minus-x", "ones-in-T"])
def test_the_key_patterns_of_the_large_class(torch_mod, sorter, builder, order, descending):
    """no pass (the keys come back raw), exactly one, exactly three (an odd count: the copy back), +x / -x (one raw bit, up to
    31 bits of T), and the key that ties with the pads -- in a large segment with a partial tile, a mid and a small one"""
    _check(torch_mod, sorter, builder, [LARGE, 16385, 9000, 300], order, descending)


@EVERY_ORDER
def test_the_ballot_ranking(torch_mod, ballot_sorter, order, descending):
    _check(torch_mod, ballot_sorter, _builder(order), [300, 4097, 16384, 16385 + 777], order, descending, tag="ballot")
    _check(torch_mod, ballot_sorter, "three-bytes", [20000], order, descending, tag="ballot")


@pytest.mark.parametrize("order,descending", [("float32", True), ("int32", False)])
def test_more_segments_than_resident_workgroups(torch_mod, sorter, order, descending):
    """the mid and the large launch take their lists by grid stride with at most two workgroups per CU: 700 mid and 700 large
    segments make every workgroup sort more than one"""
    _check(torch_mod, sorter, _builder(order), [4100] * 700 + [16390] * 700 + [17] * 50, order, descending, modes=(True,))


@MODES
def test_bad_offsets_are_flagged_and_their_segments_left_alone(torch_mod, sorter, key_value):
    import vulkan_radix_sort_amd as vrdx
    order, descending = "float32", True
    keys, values, offsets = segment_case("float-specials", [500, 5000, 17000, 40], order, descending, "bad")
    values = values if key_value else None
    bad = offsets.copy()
    bad[2] = bad[1] - 7                       # segment 1 decreases (and segment 2 then starts in front of segment 1's begin)
    got = ordered_call(torch_mod, sorter, keys, values, offsets=bad, order=order_word(order, descending),
                       expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    lo, hi = int(bad[3]), int(bad[4])         # the last segment overlaps nothing: sorted; in front of offsets[0]: untouched
    want = expected_segments(keys, values, np.array([lo, hi]), len(keys), order, descending)
    assert np.array_equal(got.keys[lo:], want[0][lo:]) and np.array_equal(got.keys[:int(bad[0])], keys[:int(bad[0])])
    behind = offsets.copy()
    behind[-1] = len(keys) + 1                # the last segment ends behind maxElementCount: left alone, the others sorted
    got = ordered_call(torch_mod, sorter, keys, values, offsets=behind, order=order_word(order, descending),
                       expect_status=vrdx.STATUS_SEGMENTS_INVALID)
    assert_same(got.keys, got.values, expected_segments(keys, values, behind, len(keys), order, descending))
    stream = torch_mod.cuda.current_stream().cuda_stream
    assert sorter.read_sorter_status(stream) == vrdx.STATUS_SEGMENTS_INVALID and sorter.read_sorter_status(stream) == 0


@EVERY_ORDER
def test_every_4_byte_alignment(torch_mod, sorter, order, descending):
    for i, keys_off in enumerate((4, 8, 12)):
        _check(torch_mod, sorter, _builder(order), [1000, 4097, 16385 + 333], order, descending, tag=f"align{keys_off}",
               keys_off=keys_off, values_off=(keys_off + 4 + 4 * i) % 16, offsets_off=4 * (i + 1), storage_off=16 * (i + 1))


@MODES
def test_order_word_0_is_the_twin_and_other_words_are_refused(torch_mod, sorter, key_value):
    keys, values, offsets = segment_case("uniform", [300, 5000, 17000], "uint32", False, "twin")
    values = values if key_value else None
    got = ordered_call(torch_mod, sorter, keys, values, offsets=offsets, order=0)
    twin = ordered_call(torch_mod, sorter, keys, values, offsets=offsets, order=None, twin=True)
    assert_same(got.keys, got.values, (twin.keys, twin.values))
    assert_same(got.keys, got.values, expected_segments(keys, values, offsets, len(keys), "uint32", False))
    assert torch_mod.equal(got.storage[:16], twin.storage[:16])
    for word in (3, 0x200, 0x103):
        got = ordered_call(torch_mod, sorter, keys, values, offsets=offsets, order=word, expect_refused=True)
        assert_same(got.keys, got.values, (keys, values))


@MODES
def test_a_captured_call_replays_on_another_segmentation(torch_mod, sorter, key_value):
    torch = torch_mod
    order, descending = "float32", True
    word = order_word(order, descending)
    first = segment_case("float-specials", [17000, 5000, 300, 2], order, descending, "replay0")
    second = segment_case("duplicates", [22000, 9, 0, 277], order, descending, "replay1")
    n = max(len(first[0]), len(second[0]))
    segments = len(first[2]) - 1
    dk = torch.zeros(n, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n, dtype=torch.int32, device="cuda") if key_value else None
    do = torch.zeros(segments + 1, dtype=torch.int32, device="cuda")
    req = sorter.key_value_storage_requirements(n) if key_value else sorter.storage_requirements(n)
    storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")

    def record():
        stream = torch.cuda.current_stream().cuda_stream
        if key_value:
            sorter.cmd_ordered_sort_segmented_key_value(stream, n, segments, do.data_ptr(), 0, dk.data_ptr(), 0, dv.data_ptr(), 0,
                                                        word, storage.data_ptr(), 0)
        else:
            sorter.cmd_ordered_sort_segmented(stream, n, segments, do.data_ptr(), 0, dk.data_ptr(), 0, word, storage.data_ptr(), 0)

    record()  # one eager call first, as the other capture tests do
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        record()
    stream = torch.cuda.current_stream().cuda_stream
    for keys, values, offsets in (first, second):
        pad = n - len(keys)
        keys, values = np.concatenate([keys, np.zeros(pad, np.uint32)]), np.concatenate([values, np.zeros(pad, np.uint32)])
        dk.copy_(torch.from_numpy(keys.view(np.int32).copy()))
        if key_value:
            dv.copy_(torch.from_numpy(values.view(np.int32).copy()))
        do.copy_(torch.from_numpy(offsets.view(np.int32).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same(dk.cpu().numpy().view(np.uint32), dv.cpu().numpy().view(np.uint32) if key_value else None,
                    expected_segments(keys, values if key_value else None, offsets, n, order, descending))
        assert sorter.read_status(stream, storage.data_ptr(), 0) == 0 and sorter.read_sorter_status(stream) == 0


@pytest.mark.parametrize("descending", DIRECTIONS, ids=["ascending", "descending"])
def test_sort_segments_ordered_against_torch_sort_per_segment(torch_mod, sorter, descending):
    import vulkan_radix_sort_amd as vrdx
    from key_order32_cases import case_keys
    torch = torch_mod
    sizes = [300, 0, 4097, 17001, 1]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    keys, _ = case_keys("float-values", int(offsets[-1]), "float32", descending, tag="torch-segments")
    t = torch.from_numpy(keys.view(np.float32).copy()).cuda()
    dk, dv = t.clone(), torch.arange(len(keys), dtype=torch.int32, device="cuda")
    vrdx.sort_segments_ordered(sorter, dk, torch.from_numpy(offsets).cuda(), dv, order="float32", descending=descending)
    torch.cuda.synchronize()
    for b, e in zip(offsets[:-1], offsets[1:]):
        want, index = torch.sort(t[b:e], stable=True, descending=descending)
        assert torch.equal(dk[b:e].view(torch.int32), want.view(torch.int32)) and torch.equal(dv[b:e].to(torch.int64), index + int(b))
    assert sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream) == 0
