"""What tools/sort64_bench.py --order and tools/segmented_bench.py --order share: the keys, the order's bijection T as torch
operations (the workaround a caller of the unordered 64-bit sorts has to write: transform, sort, transform back), and the
loop that lets the ways take turns in one process.

  ordered     the ordered call (vrdxHipCmdSort64Ordered* / vrdxHipCmdSortSegmented64Ordered*) on the keys
  workaround  T in torch, in place; the unordered call; the inverse of T in torch, in place
  unordered   the unordered call on keys that are T(keys) already (prepared outside the timed region): the same sort work as
              `ordered`, so ordered / unordered is what the fused transform costs
"""
import json

import numpy as np

MIN = -(1 << 63)


def make_keys(torch, n, gen):
    """64 random bits: both signs, and as float64 every class of value, NaNs included"""
    return torch.randint(MIN, (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)


def transform_(keys, order, descending):
    """keys <- T(keys), in place, with as few torch kernels as eager mode allows"""
    if order == "float64":
        keys.bitwise_xor_((keys >> 63).bitwise_or_(MIN))   # negative: all bits; the others: bit 63
    elif order == "int64":
        keys.bitwise_xor_(MIN)
    if descending:
        keys.bitwise_not_()


def inverse_(keys, order, descending):
    if descending:
        keys.bitwise_not_()
    if order == "float64":
        keys.bitwise_xor_((keys.bitwise_not() >> 63).bitwise_or_(MIN))   # T's bit 63 clear: the key was negative
    elif order == "int64":
        keys.bitwise_xor_(MIN)


def take_turns(torch, ways, fns, fresh, prepare, rounds, steps, warmup):
    """ms per way: [round][step]; the ways take turns step by step, so that a drift of the clocks meets all of them alike"""
    times = {w: [] for w in ways}
    step = 0
    for r in range(rounds):
        this = {w: [] for w in ways}
        for i in range((warmup if r == 0 else 0) + steps):
            for way in ways:
                fresh(step)
                prepare[way]()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[way]()
                e1.record()
                torch.cuda.synchronize()
                if r > 0 or i >= warmup:
                    this[way].append(e0.elapsed_time(e1))
            step += 1
        for way in ways:
            times[way].append(this[way])
    return times


def summarise(result, ways, times):
    for way in ways:
        result[way + "_ms"] = float(np.median(np.concatenate(times[way])))
        result[way + "_ms_min"] = float(np.min(np.concatenate(times[way])))
        result[way + "_round_medians_ms"] = [float(np.median(t)) for t in times[way]]
    result["unordered_spread_ms"] = max(result["unordered_round_medians_ms"]) - min(result["unordered_round_medians_ms"])
    result["ordered_vs_workaround"] = result["workaround_ms"] / result["ordered_ms"]
    result["ordered_over_unordered"] = result["ordered_ms"] / result["unordered_ms"]
    return json.dumps(result)
