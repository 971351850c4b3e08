"""GPU test of the segmented sorts' launches that are NOT recorded: under a bound no mid or large segment fits in, the planner
(vrdx_plan.h, PlanSegmentedSort) lists no launch for that class, and the timestamp slot the launch would have ended shares
the event of the slot before it -- so the times read back are equal to the nanosecond, which no launch in between could
give.  Each of the four forms (whole key, bit range, 64-bit keys, 64-bit keys with an order word), keys-only, two segments of
8 keys."""
import numpy as np
import pytest

from guarded_call import sorter, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

BEGIN, END = 3, 20  # the bit range of the range form


def _field(keys):
    return (keys >> np.uint32(BEGIN)) & np.uint32((1 << (END - BEGIN)) - 1)


def _int64_descending(keys):
    return np.sort(keys.view(np.int64))[::-1].view(np.uint64)


# form -> (key dtype, the call -- front: the arguments up to the keys, back: from the storage on --, one segment sorted)
def _forms(vrdx):
    word = vrdx.order_word("int64", descending=True)
    return {
        "whole-key": (np.uint32, lambda s, front, back: s.cmd_sort_segmented(*front, *back), np.sort),
        "bit-range": (np.uint32, lambda s, front, back: s.cmd_sort_segmented_bits(*front, BEGIN, END, *back),
                      lambda k: k[np.argsort(_field(k), kind="stable")]),
        "64-bit": (np.uint64, lambda s, front, back: s.cmd_sort_segmented64(*front, *back), np.sort),
        "64-bit-ordered": (np.uint64, lambda s, front, back: s.cmd_sort_segmented64_ordered(*front, word, *back),
                           _int64_descending),
    }


@pytest.mark.parametrize("bound", [4096, 4097])
@pytest.mark.parametrize("form", ["whole-key", "bit-range", "64-bit", "64-bit-ordered"])
def test_a_launch_that_is_not_recorded_leaves_its_slot_to_the_one_before(torch_mod, sorter, form, bound):
    """bound 4096: no segment can be mid or large (4096 / 4097 == 0 list entries), so slots 3 ... 14 are slot 2's event.
    bound 4097: one mid segment fits and none that is large (4097 / 16385 == 0), so the mid launch ends slot 3 and slots
    4 ... 14 are its event."""
    import vulkan_radix_sort_amd as vrdx
    torch = torch_mod
    dtype, call, sorted_segment = _forms(vrdx)[form]
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(bound)
    keys = rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), size=bound, dtype=np.uint64).astype(dtype)
    signed = np.int32 if dtype == np.uint32 else np.int64
    dk = torch.from_numpy(keys.view(signed).copy()).cuda()
    offsets = torch.from_numpy(np.array([0, 8, 16], np.uint32).view(np.int32)).cuda()
    need = sorter.storage_requirements(bound).size if dtype == np.uint32 else sorter.storage_requirements64(bound).size
    storage = torch.empty(need, dtype=torch.uint8, device="cuda")
    pool = vrdx.QueryPool(15)
    call(sorter, (stream, bound, 2, offsets.data_ptr(), 0, dk.data_ptr(), 0), (storage.data_ptr(), 0, pool, 0))
    torch.cuda.synchronize()
    assert sorter.read_status(stream, storage.data_ptr(), 0) == 0 and sorter.read_sorter_status(stream) == 0
    ts = pool.results_ns(0, 15)
    pool.destroy()
    print(form, bound, ts)
    assert ts[0] == 0 and ts[1] >= 0 and ts[2] > 0 and ts[2] >= ts[1]
    if bound == 4096:
        assert ts[3:] == [ts[2]] * 12
    else:
        assert ts[3] >= ts[2] and ts[4:] == [ts[3]] * 11
    got = dk.cpu().numpy().view(dtype)
    want = keys.copy()
    want[0:8] = sorted_segment(keys[0:8])
    want[8:16] = sorted_segment(keys[8:16])
    assert np.array_equal(got, want)
