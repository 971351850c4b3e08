#!/usr/bin/env python3
"""Times the key orders of the 32-bit sorts (vrdxHipCmdOrderedSort[KeyValue], vrdxHipCmdOrderedSortSegmented[KeyValue]) on one
GPU, three ways taking turns step by step in one process (tools/key_order_ways.py: each way between one pair of events with
the device idle before it, fresh keys every step, medians over --rounds rounds of --steps timed steps), on keys of 32 random
bits (both signs; as float32 every class of value, NaNs included):

  ordered     the ordered call on the keys
  workaround  T in torch, in place; the unordered call (vrdxCmdSort[KeyValue], vrdxHipCmdSortSegmented[KeyValue]); the inverse
              of T in torch, in place
  unordered   the unordered call on keys that are T(keys) already (prepared outside the timed region): the same sort work as
              `ordered`, so ordered - unordered is what the order costs

Shapes: flat sorts of --sizes keys and the segmented --shapes (segments x keys per segment), every order of --orders (a
trailing "-" is descending), keys-only and key+value.  Each row prints ONE JSON line; on one extra, untimed input `ordered`
must equal `workaround` bit for bit ("match").  For a flat sort beyond 16384 keys the line also carries "order_cost_ms" =
ordered - unordered, next to "two_trips_ms_at" = the time two streaming trips of 8 bytes per key take at --stream-gbs (the
rate the 64-bit split and merge were measured at): the ordered sort runs two streaming launches around
the unordered plan, and a form with T fused into that plan's kernels has this number to beat.

usage: python tools/sort_ordered_bench.py [--sizes 4096,16384,262144,4194304,33554432]
       [--shapes 65536x256,8192x2048,1024x16384,64x262144] [--orders int32,float32,float32-,uint32-] [--modes keys,kv]
       [--steps 5] [--rounds 3] [--warmup 2] [--stream-gbs 5500] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

MIN = -(1 << 31)


def transform_(keys, order, descending):
    """keys <- T(keys), in place, with as few torch kernels as eager mode allows"""
    if order == "float32":
        keys.bitwise_xor_((keys >> 31).bitwise_or_(MIN))   # negative: all bits; the others: bit 31
    elif order == "int32":
        keys.bitwise_xor_(MIN)
    if descending:
        keys.bitwise_not_()


def inverse_(keys, order, descending):
    if descending:
        keys.bitwise_not_()
    if order == "float32":
        keys.bitwise_xor_((keys.bitwise_not() >> 31).bitwise_or_(MIN))   # T's bit 31 clear: the key was negative
    elif order == "int32":
        keys.bitwise_xor_(MIN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,262144,4194304,33554432")
    ap.add_argument("--shapes", default="65536x256,8192x2048,1024x16384,64x262144")
    ap.add_argument("--orders", default="int32,float32,float32-,uint32-")
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stream-gbs", type=float, default=5500.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx
    from key_order_ways import summarise, take_turns

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    ways = ("ordered", "workaround", "unordered")
    out = open(args.out, "a") if args.out else None
    stream = torch.cuda.current_stream().cuda_stream
    shapes = [(None, int(x)) for x in args.sizes.split(",") if x]
    shapes += [tuple(int(y) for y in x.split("x")) for x in args.shapes.split(",") if x]
    for segments, per in shapes:
        n = per if segments is None else segments * per
        offsets = None if segments is None else torch.arange(0, n + 1, per, dtype=torch.int32, device="cuda")
        for spelled in args.orders.split(","):
            order, descending = spelled.rstrip("-"), spelled.endswith("-")
            word = vrdx.order_word32(order, descending)
            for mode in args.modes.split(","):
                kv = mode == "kv"
                keys = torch.empty(n, dtype=torch.int32, device="cuda")
                values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
                iota = torch.arange(n, dtype=torch.int32, device="cuda")
                req = sorter.key_value_storage_requirements(n) if kv else sorter.storage_requirements(n)
                storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")
                gen = torch.Generator(device="cuda")

                def fresh(step):
                    gen.manual_seed(args.seed * 1000003 + step)
                    keys.copy_(torch.randint(MIN, (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=gen))
                    if kv:
                        values.copy_(iota)

                def record(w):
                    # (sorter, stream, count, offsets, segment count, indirect, keys, values, order, storage)
                    if w is not None:
                        vrdx.api.record_ordered_sort(sorter, stream, n, offsets, segments, None, keys, values, w, storage)
                    else:
                        vrdx.api.record_sort(sorter, 32, stream, n, offsets, segments, None, keys, values, None, None, storage)

                def run_workaround():
                    transform_(keys, order, descending)
                    record(None)
                    inverse_(keys, order, descending)

                fns = {"ordered": lambda: record(word), "workaround": run_workaround, "unordered": lambda: record(None)}
                prepare = {"ordered": lambda: None, "workaround": lambda: None,
                           "unordered": lambda: transform_(keys, order, descending)}
                times = take_turns(torch, ways, fns, fresh, prepare, args.rounds, args.steps, args.warmup)
                outputs = {}
                for way in ("ordered", "workaround"):
                    fresh(1 << 20)
                    fns[way]()
                    torch.cuda.synchronize()
                    outputs[way] = (keys.clone(), values.clone() if kv else None)
                (a, av), (b, bv) = outputs["ordered"], outputs["workaround"]
                plan = sorter.describe_ordered_sort_plan(n, kv, word)
                result = {"shape": str(n) if segments is None else f"{segments}x{per}", "n": n, "order": order,
                          "descending": descending, "key_value": kv, "rounds": args.rounds, "steps_per_round": args.steps,
                          "plan": "segmented" if segments is not None else plan.name, "launches": int(plan.launches),
                          "match": bool(torch.equal(a, b) and (not kv or torch.equal(av, bv))),
                          "status": sorter.read_sorter_status(stream)}
                line = json.loads(summarise(result, ways, times))
                if segments is None and n > 16384:
                    line["order_cost_ms"] = line["ordered_ms"] - line["unordered_ms"]
                    line["two_trips_ms_at"] = {"gbs": args.stream_gbs, "ms": 2 * 8 * n / (args.stream_gbs * 1e9) * 1e3}
                line = json.dumps(line)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del keys, values, storage, iota, outputs
                torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


if __name__ == "__main__":
    main()
