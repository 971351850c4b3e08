#!/usr/bin/env python3
"""Times the 64-bit sorts (vrdxHipCmdSort64[KeyValue], with --indirect vrdxHipCmdSort64[KeyValue]Indirect) on one GPU, step by step, against two yardsticks outside them:

  sort64      one vrdxHipCmdSort64[KeyValue] call, stamped with a 15-slot query pool: the call (slot 14 - slot 0) and each of
              its steps (split | first sort | gather | second sort | merge or permute | copy back)
  torch_sort  torch.sort of the same int64 tensor in the same process (keys below 2^63, so that the signed and the unsigned
              order agree); key+value: a stable torch.sort and the gather of the values by its indices
  two_sorts   two vrdxCmdSortKeyValue of N on the keys' own words, (low, high) and then (high, low): the floor of the
              composition -- what is left of sort64_ms above it is the price of the kernels around the sorts

Every step sorts a fresh copy of the same keys (generated on the device, seeded); times are medians over --steps.  The
streaming steps are also given as achieved bytes per second, priced with the bytes they have to move per element: split and
merge 16, gather 12 (index, one word of the key, the word out), permute 28 (index, high word, low word and value in; key and
value out), copy back 24.  Each shape prints ONE JSON line; the sort64 result of the last step is compared with torch's.

--indirect records the sort64 step through the indirect forms instead, with N as the bound and a count equal to N held in
a device word, and adds "indirect": true to every line: the same work by the same kernels and grids, so its sort64_ms over
that of a run without the flag is the price of reading the count on the device.

--order ORDER [--descending] (ORDER: uint64, int64, float64) times the key orders instead (vrdxHipCmdSort64Ordered[KeyValue]),
three ways taking turns in one process, each between one pair of events, on keys of 64 random bits (tools/key_order_ways.py):
`ordered`, the `workaround` in torch around the unordered call, and the `unordered` call on keys that are T(keys) already.
The timed steps come in --rounds rounds; on one extra, untimed input `ordered` must equal `workaround` bit for bit (`"match"`).

usage: python tools/sort64_bench.py [--sizes 1048576,4194304,33554432] [--patterns uniform,bits32,tile_depth]
       [--modes keys,kv] [--steps 7] [--warmup 2] [--indirect] [--out FILE]
       [--order ORDER [--descending] [--rounds 3]]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_BYTES = {"split": 16, "merge": 16, "gather": 12, "permute": 28, "copy_back": 24}


def make_keys(torch, pattern, n, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    if pattern == "uniform":  # 63 random bits
        return torch.randint(0, (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
    if pattern == "bits32":  # 32 significant bits: the high word is constant
        return torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=gen)
    if pattern == "tile_depth":  # a 16-bit tile id over the bits of a positive float depth
        tile = torch.randint(0, 1 << 16, (n,), dtype=torch.int64, device="cuda", generator=gen)
        depth = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen) * 100.0 + 0.1
        return (tile << 32) | depth.view(torch.int32).to(torch.int64)
    raise ValueError(pattern)


def main_order(args):
    import torch
    import vulkan_radix_sort_amd as vrdx
    from key_order_ways import inverse_, make_keys as random_keys, summarise, take_turns, transform_

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    ways = ("ordered", "workaround", "unordered")
    out = open(args.out, "a") if args.out else None
    order, descending = args.order, args.descending
    for n in (int(x) for x in args.sizes.split(",")):
        for mode in args.modes.split(","):
            kv = mode == "kv"
            keys = torch.empty(n, dtype=torch.int64, device="cuda")
            values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
            iota = torch.arange(n, dtype=torch.int32, device="cuda")
            storage = torch.empty(sorter.storage_requirements64(n, kv).size, dtype=torch.uint8, device="cuda")
            gen = torch.Generator(device="cuda")

            def fresh(step):
                gen.manual_seed(args.seed * 1000003 + step)
                keys.copy_(random_keys(torch, n, gen))
                if kv:
                    values.copy_(iota)

            def run_ordered():
                vrdx.sort64(sorter, keys, values, storage=storage, order=order, descending=descending)

            def run_workaround():
                transform_(keys, order, descending)
                vrdx.sort64(sorter, keys, values, storage=storage)
                inverse_(keys, order, descending)

            def run_unordered():
                vrdx.sort64(sorter, keys, values, storage=storage)

            fns = {"ordered": run_ordered, "workaround": run_workaround, "unordered": run_unordered}
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
            result = {"n": n, "order": order, "descending": descending, "key_value": kv, "rounds": args.rounds,
                      "steps_per_round": args.steps, "match": bool(torch.equal(a, b) and (not kv or torch.equal(av, bv))),
                      "status": sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream)}
            line = summarise(result, ways, times)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del keys, values, storage, iota, outputs
            torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,4194304,33554432")
    ap.add_argument("--patterns", default="uniform,bits32,tile_depth")
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--indirect", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--order", default="", choices=["", "uint64", "int64", "float64"],
                    help="time the key orders: ordered, workaround, unordered")
    ap.add_argument("--descending", action="store_true")
    ap.add_argument("--rounds", type=int, default=3, help="--order: rounds of --steps timed steps")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    if not torch.cuda.is_available():
        sys.exit("sort64_bench.py needs a GPU (there is no CPU fallback)")
    if args.order:
        return main_order(args)
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    pool, pool_lo, pool_hi = vrdx.QueryPool(15), vrdx.QueryPool(15), vrdx.QueryPool(15)
    out = open(args.out, "a") if args.out else None

    def median(xs):
        return float(np.median(xs))

    for n in (int(x) for x in args.sizes.split(",")):
        for pattern in args.patterns.split(","):
            master = make_keys(torch, pattern, n, args.seed)
            for mode in args.modes.split(","):
                kv = mode == "kv"
                keys = torch.empty_like(master)
                values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
                iota = torch.arange(n, dtype=torch.int32, device="cuda")
                storage = torch.empty(sorter.storage_requirements64(n, kv).size, dtype=torch.uint8, device="cuda")
                inner = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
                lo = torch.empty(n, dtype=torch.int32, device="cuda")
                hi = torch.empty(n, dtype=torch.int32, device="cuda")
                count = torch.tensor([n], dtype=torch.int32, device="cuda") if args.indirect else None
                slots, torch_ms, floor_ms = [], [], []
                torch_keys = torch_values = None
                for step in range(args.warmup + args.steps):
                    timed = step >= args.warmup
                    # sort64
                    keys.copy_(master)
                    if kv:
                        values.copy_(iota)
                    torch.cuda.synchronize()
                    if kv and args.indirect:
                        sorter.cmd_sort64_key_value_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0,
                                                             values.data_ptr(), 0, storage.data_ptr(), 0, pool, 0)
                    elif kv:
                        sorter.cmd_sort64_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, storage.data_ptr(), 0,
                                                    pool, 0)
                    elif args.indirect:
                        sorter.cmd_sort64_indirect(stream, n, count.data_ptr(), 0, keys.data_ptr(), 0, storage.data_ptr(), 0,
                                                   pool, 0)
                    else:
                        sorter.cmd_sort64(stream, n, keys.data_ptr(), 0, storage.data_ptr(), 0, pool, 0)
                    torch.cuda.synchronize()
                    if timed:
                        slots.append(pool.results_ns(0, 15))
                    # torch.sort of the same tensor
                    fresh = master.clone()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if kv:
                        torch_keys, idx = torch.sort(fresh, stable=True)
                        torch_values = iota[idx]
                    else:
                        torch_keys, _ = torch.sort(fresh)
                    e1.record()
                    torch.cuda.synchronize()
                    if timed:
                        torch_ms.append(e0.elapsed_time(e1))
                    del fresh
                    # the two inner sorts alone, on the keys' own words
                    lo.copy_((master & 0xFFFFFFFF).to(torch.int32))  # (wraps like the uint32 bit pattern)
                    hi.copy_((master >> 32).to(torch.int32))
                    torch.cuda.synchronize()
                    sorter.cmd_sort_key_value(stream, n, lo.data_ptr(), 0, hi.data_ptr(), 0, inner.data_ptr(), 0, pool_lo, 0)
                    sorter.cmd_sort_key_value(stream, n, hi.data_ptr(), 0, lo.data_ptr(), 0, inner.data_ptr(), 0, pool_hi, 0)
                    torch.cuda.synchronize()
                    if timed:
                        floor_ms.append((pool_lo.results_ns(0, 15)[14] + pool_hi.results_ns(0, 15)[14]) / 1e6)
                ts = np.median(np.array(slots, dtype=np.float64), axis=0) / 1e6  # ms since slot 0, per slot
                names = (["split", "sort_low", "gather", "sort_high", "permute", "copy_back"] if kv
                         else ["split", "sort_low", None, "sort_high", "merge"])
                result = {"n": n, "pattern": pattern, "key_value": kv, "sort64_ms": float(ts[14])}
                if args.indirect:
                    result["indirect"] = True
                for i, name in enumerate(names):
                    if name is not None:
                        result[name + "_ms"] = float(ts[i + 1] - ts[i])
                        if name in STEP_BYTES and ts[i + 1] > ts[i]:
                            result[name + "_GBps"] = STEP_BYTES[name] * n / ((ts[i + 1] - ts[i]) * 1e6)
                result["torch_sort_ms"] = median(torch_ms)
                result["two_sorts_ms"] = median(floor_ms)
                result["speedup_vs_torch_sort"] = result["torch_sort_ms"] / result["sort64_ms"]
                result["over_two_sorts"] = result["sort64_ms"] / result["two_sorts_ms"]
                result["sort64_gkeys_s"] = n / (result["sort64_ms"] * 1e6)
                result["status"] = sorter.read_status(stream, storage.data_ptr(), 0)
                result["match"] = bool(torch.equal(keys, torch_keys) and (not kv or torch.equal(values, torch_values)))
                line = json.dumps(result)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del keys, values, storage, inner, lo, hi, count, torch_keys, torch_values
                torch.cuda.empty_cache()
            del master
    if out:
        out.close()
    for p in (pool, pool_lo, pool_hi):
        p.destroy()
    sorter.destroy()


if __name__ == "__main__":
    main()
