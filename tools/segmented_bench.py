#!/usr/bin/env python3
"""Times three ways of sorting many independent arrays packed back to back (CSR offsets) on one GPU:

  segmented   one vrdxHipCmdSortSegmented[KeyValue] call (vulkan_radix_sort_amd.sort_segments)
  per_array   one vrdxCmdSort[KeyValue] per segment on one stream and storage -- what HipShardExecutor.enqueue does today
  torch_sort  torch.sort(stable=True) of the packed int64 (segment << 32) | key, unpacked again (values gathered by the
              returned indices)

Every step sorts fresh keys (seeded, generated on the device outside the timed region); the time of a step is the device
event interval around the enqueue of the whole job, so a host-bound loop of enqueues is charged what it costs.  Each shape
prints ONE JSON line; the segmented result of the last step is compared with the torch_sort result (`"match"`).

--keys64 times the same for uint64 keys (vrdxHipCmdSortSegmented64[KeyValue]), four ways, alternating in one process:

  segmented64  one vrdxHipCmdSortSegmented64[KeyValue] call (vulkan_radix_sort_amd.sort_segments64)
  composed     what the 32-bit entry points offer: split into words with torch ops, sort_segments(lo, values=hi), then
               sort_segments(hi, values=lo), recombine; key+value: the words carry an index (sort_segments(lo, values=index),
               gather the high words by it, sort_segments(hi, values=index)) and keys and values are gathered by it at the end
  per_array    one vrdxHipCmdSort64[KeyValue] per segment on one stream and storage
  torch_sort   two stable torch.sort: by key, then by segment id
Every way's result on one extra, untimed input is compared with np.lexsort((keys, segment id)) on the host (`"match_*"`).

--bits BEGIN END (repeatable) times the segmented sort by the bit range [BEGIN, END) of uint32 keys
(vrdxHipCmdSortSegmentedBits[KeyValue]), three ways taking turns in one process, each between one pair of events:

  range        one vrdxHipCmdSortSegmentedBits[KeyValue] call (vulkan_radix_sort_amd.sort_segments_bits)
  workaround   what the whole-key entry points offer: the field and an iota with torch ops, sort_segments(field, values=iota),
               then the keys (and values) gathered by the sorted iota
  whole_key    sort_segments of the same keys: ANOTHER result (the whole key orders it), timed as the price of four digits
The timed steps come in --rounds rounds (default 5); a way's time is the median over all of them, and `whole_key_spread_ms` is
the range of the whole-key sort's five per-round medians -- the run-to-run spread the range sort at [0, 8) is held against.
On one extra, untimed input `range` must equal `workaround` bit for bit (`"match"`) and differ from `whole_key`.

--order ORDER [--descending] (ORDER: uint64, int64, float64) times the key orders of the segmented sort of uint64 keys
(vrdxHipCmdSortSegmented64Ordered[KeyValue]), three ways taking turns in one process on keys of 64 random bits
(tools/key_order_ways.py): `ordered`, the `workaround` in torch around sort_segments64, and the `unordered` sort_segments64 on
keys that are T(keys) already.  --rounds rounds of --steps steps; `ordered` must equal `workaround` bit for bit (`"match"`).

usage: python tools/segmented_bench.py [--shapes 65536x256,8192x2048,...,mixed] [--steps 5] [--warmup 2] [--loop-steps 3]
       [--modes keys,kv] [--only segmented] [--out FILE] [--keys64 [--patterns uniform,tile_depth]]
       [--bits BEGIN END [--bits BEGIN END ...] [--rounds 5]]
       [--order ORDER [--descending] [--rounds 5]]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_SHAPES = "65536x256,8192x2048,1024x16384,64x262144,4x4194304,mixed"
BITS_SHAPES = "65536x256,8192x2048,1024x16384,64x262144"


def segment_sizes(shape, rng):
    """Sizes of the segments of a shape: 'SxL' = S segments of L keys; 'mixed' = sizes log-uniform in [1, 100000] (every
    16th segment empty) until about 2^24 keys."""
    if shape == "mixed":
        sizes, total = [], 0
        while total < (1 << 24):
            s = 0 if len(sizes) % 16 == 15 else int(math.exp(rng.uniform(0.0, math.log(100000.0))))
            s = min(s, (1 << 24) - total) if total + s > (1 << 24) else s
            sizes.append(s)
            total += s
        return np.array(sizes, dtype=np.int64)
    count, length = (int(x) for x in shape.split("x"))
    return np.full(count, length, dtype=np.int64)


def make_keys64(torch, pattern, n, gen):
    if pattern == "uniform":  # 63 random bits
        return torch.randint(0, (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
    if pattern == "tile_depth":  # a 16-bit tile id over the bits of a positive float depth (tools/sort64_bench.py)
        tile = torch.randint(0, 1 << 16, (n,), dtype=torch.int64, device="cuda", generator=gen)
        depth = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen) * 100.0 + 0.1
        return (tile << 32) | depth.view(torch.int32).to(torch.int64)
    raise ValueError(pattern)


def main64(args):
    import torch
    import vulkan_radix_sort_amd as vrdx

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    all_ways = ("segmented64", "composed", "per_array", "torch_sort")
    ways = [w for w in all_ways if not args.only or w in args.only.split(",")]
    out = open(args.out, "a") if args.out else None
    verify_step = 1 << 20  # the seed offset of the one input every way is checked on

    for shape in args.shapes.split(","):
        rng = np.random.default_rng(args.seed)
        sizes = segment_sizes(shape, rng)
        offsets_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(offsets_h[-1])
        offsets = torch.from_numpy(offsets_h.astype(np.uint32).view(np.int32)).cuda()
        seg_h = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
        seg_ids = torch.from_numpy(seg_h).cuda()
        starts = [int(x) for x in offsets_h[:-1]]
        lengths = [int(x) for x in sizes]
        big = max(lengths) if lengths else 0
        for pattern in args.patterns.split(","):
            order = None  # np.lexsort of the verification input: the same for both modes
            for mode in args.modes.split(","):
                kv = mode == "kv"
                keys = torch.empty(n, dtype=torch.int64, device="cuda")
                values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
                storage = torch.empty(sorter.storage_requirements64(n, key_value=kv).size, dtype=torch.uint8, device="cuda")
                req32 = (sorter.key_value_storage_requirements(n)).size
                storage32 = torch.empty(req32, dtype=torch.uint8, device="cuda")
                loop_storage = torch.empty(max(16, sorter.storage_requirements64(big, key_value=kv).size), dtype=torch.uint8,
                                           device="cuda")
                gen = torch.Generator(device="cuda")
                stream = torch.cuda.current_stream()
                iota = torch.arange(n, dtype=torch.int32, device="cuda")

                def fresh(step):
                    gen.manual_seed(args.seed * 1000003 + step)
                    keys.copy_(make_keys64(torch, pattern, n, gen))
                    if kv:
                        values.copy_(iota)

                def run_segmented64():
                    vrdx.sort_segments64(sorter, keys, offsets, values=values, storage=storage)

                def run_composed():
                    lo = (keys & 0xFFFFFFFF).to(torch.int32)
                    hi = (keys >> 32).to(torch.int32)
                    if not kv:
                        vrdx.sort_segments(sorter, lo, offsets, values=hi, storage=storage32)
                        vrdx.sort_segments(sorter, hi, offsets, values=lo, storage=storage32)
                        keys.copy_((hi.to(torch.int64) << 32) | (lo.to(torch.int64) & 0xFFFFFFFF))
                        return
                    index = iota.clone()
                    vrdx.sort_segments(sorter, lo, offsets, values=index, storage=storage32)
                    hi = hi[index.to(torch.int64)]
                    vrdx.sort_segments(sorter, hi, offsets, values=index, storage=storage32)
                    gather = index.to(torch.int64)
                    keys.copy_(keys[gather])
                    values.copy_(values[gather])

                def run_per_array():
                    s = stream.cuda_stream
                    kp, sp = keys.data_ptr(), loop_storage.data_ptr()
                    for b, m in zip(starts, lengths):
                        if kv:
                            sorter.cmd_sort64_key_value(s, m, kp, 8 * b, values.data_ptr(), 4 * b, sp, 0)
                        else:
                            sorter.cmd_sort64(s, m, kp, 8 * b, sp, 0)

                def run_torch_sort():
                    by_key, first = torch.sort(keys, stable=True)  # (63-bit keys: the signed order is the unsigned one)
                    _, second = torch.sort(seg_ids[first], stable=True)
                    keys.copy_(by_key[second])
                    if kv:
                        values.copy_(values[first[second]])

                fns = {"segmented64": run_segmented64, "composed": run_composed, "per_array": run_per_array,
                       "torch_sort": run_torch_sort}
                result = {"shape": shape, "keys64": True, "pattern": pattern, "segments": len(sizes), "keys": n,
                          "key_value": kv, "max_segment": big}
                times = {w: [] for w in ways}
                # the ways take turns step by step, so that a drift of the clocks meets all of them alike
                for step in range(args.warmup + args.steps):
                    for way in ways:
                        if way == "per_array" and step >= min(args.warmup, 1) + args.loop_steps:
                            continue
                        fresh(step)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fns[way]()
                        e1.record()
                        torch.cuda.synchronize()
                        if step >= (min(args.warmup, 1) if way == "per_array" else args.warmup):
                            times[way].append(e0.elapsed_time(e1))
                fresh(verify_step)
                torch.cuda.synchronize()
                if order is None:
                    order = np.lexsort((keys.cpu().numpy().view(np.uint64), seg_h))
                want = keys.cpu().numpy()[order]
                for way in ways:
                    fresh(verify_step)
                    fns[way]()
                    torch.cuda.synchronize()
                    ok = np.array_equal(keys.cpu().numpy(), want)
                    if kv:
                        ok = ok and np.array_equal(values.cpu().numpy().astype(np.int64), order)
                    result["match_" + way] = bool(ok)
                    result[way + "_ms"] = float(np.median(times[way]))
                    result[way + "_ms_min"] = float(np.min(times[way]))
                    result[way + "_steps"] = len(times[way])
                if "segmented64" in ways:
                    result["status"] = sorter.read_status(stream.cuda_stream, storage.data_ptr(), 0)
                    for way in ways[1:]:
                        result["speedup_vs_" + way] = result[way + "_ms"] / result["segmented64_ms"]
                    result["segmented64_gkeys_s"] = n / (result["segmented64_ms"] * 1e6)
                line = json.dumps(result)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del keys, values, storage, storage32, loop_storage, iota
                torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


def main_bits(args):
    import torch
    import vulkan_radix_sort_amd as vrdx

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    ways = ("range", "workaround", "whole_key")
    out = open(args.out, "a") if args.out else None
    verify_step = 1 << 20  # the seed offset of the one input the ways are compared on

    for shape in (args.shapes or BITS_SHAPES).split(","):
        rng = np.random.default_rng(args.seed)
        sizes = segment_sizes(shape, rng)
        offsets_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(offsets_h[-1])
        offsets = torch.from_numpy(offsets_h.astype(np.uint32).view(np.int32)).cuda()
        for begin, end in args.bits:
            if not 0 <= begin < end <= 32:
                sys.exit(f"--bits {begin} {end}: not a range with 0 <= BEGIN < END <= 32")
            mask = (1 << (end - begin)) - 1
            for mode in args.modes.split(","):
                kv = mode == "kv"
                keys = torch.empty(n, dtype=torch.int32, device="cuda")
                values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
                req = (sorter.key_value_storage_requirements(n) if kv else sorter.storage_requirements(n)).size
                storage = torch.empty(req, dtype=torch.uint8, device="cuda")
                storage_kv = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
                gen = torch.Generator(device="cuda")
                payload = torch.arange(n, dtype=torch.int32, device="cuda") * 3 + 1

                def fresh(step):
                    gen.manual_seed(args.seed * 1000003 + step)
                    keys.copy_(torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32))
                    if kv:
                        values.copy_(payload)

                def run_range():
                    vrdx.sort_segments_bits(sorter, keys, offsets, begin, end, values=values, storage=storage)

                def run_workaround():
                    field = (((keys.to(torch.int64) & 0xFFFFFFFF) >> begin) & mask).to(torch.int32)
                    index = torch.arange(n, dtype=torch.int32, device="cuda")
                    vrdx.sort_segments(sorter, field, offsets, values=index, storage=storage_kv)
                    gather = index.to(torch.int64)
                    keys.copy_(keys[gather])
                    if kv:
                        values.copy_(values[gather])

                def run_whole_key():
                    vrdx.sort_segments(sorter, keys, offsets, values=values, storage=storage)

                fns = {"range": run_range, "workaround": run_workaround, "whole_key": run_whole_key}
                result = {"shape": shape, "bits": [begin, end], "segments": len(sizes), "keys": n, "key_value": kv,
                          "rounds": args.rounds, "steps_per_round": args.steps}
                rounds = {w: [] for w in ways}
                step = 0
                for r in range(args.rounds):
                    times = {w: [] for w in ways}
                    # the ways take turns step by step, so that a drift of the clocks meets all of them alike
                    for i in range((args.warmup if r == 0 else 0) + args.steps):
                        for way in ways:
                            fresh(step)
                            torch.cuda.synchronize()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fns[way]()
                            e1.record()
                            torch.cuda.synchronize()
                            if r > 0 or i >= args.warmup:
                                times[way].append(e0.elapsed_time(e1))
                        step += 1
                    for way in ways:
                        rounds[way].append(times[way])
                outputs = {}
                for way in ways:
                    fresh(verify_step)
                    fns[way]()
                    torch.cuda.synchronize()
                    outputs[way] = (keys.clone(), values.clone() if kv else None)
                    medians = [float(np.median(t)) for t in rounds[way]]
                    result[way + "_ms"] = float(np.median(np.concatenate(rounds[way])))
                    result[way + "_ms_min"] = float(np.min(np.concatenate(rounds[way])))
                    result[way + "_round_medians_ms"] = medians
                result["whole_key_spread_ms"] = max(result["whole_key_round_medians_ms"]) - min(result["whole_key_round_medians_ms"])
                (a, av), (b, bv), (c, _) = outputs["range"], outputs["workaround"], outputs["whole_key"]
                result["match"] = bool(torch.equal(a, b) and (not kv or torch.equal(av, bv)))
                result["whole_key_differs"] = not bool(torch.equal(a, c))
                result["status"] = sorter.read_status(torch.cuda.current_stream().cuda_stream, storage.data_ptr(), 0)
                result["range_vs_workaround"] = result["workaround_ms"] / result["range_ms"]
                result["range_vs_whole_key"] = result["whole_key_ms"] / result["range_ms"]
                result["range_gkeys_s"] = n / (result["range_ms"] * 1e6)
                line = json.dumps(result)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del keys, values, storage, storage_kv, payload, outputs
                torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


def main_order(args):
    import torch
    import vulkan_radix_sort_amd as vrdx
    from key_order_ways import inverse_, make_keys as random_keys, summarise, take_turns, transform_

    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    ways = ("ordered", "workaround", "unordered")
    out = open(args.out, "a") if args.out else None
    order, descending = args.order, args.descending
    for shape in (args.shapes or BITS_SHAPES).split(","):
        sizes = segment_sizes(shape, np.random.default_rng(args.seed))
        offsets_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(offsets_h[-1])
        offsets = torch.from_numpy(offsets_h.astype(np.uint32).view(np.int32)).cuda()
        for mode in args.modes.split(","):
            kv = mode == "kv"
            keys = torch.empty(n, dtype=torch.int64, device="cuda")
            values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
            payload = torch.arange(n, dtype=torch.int32, device="cuda") * 3 + 1
            storage = torch.empty(sorter.storage_requirements64(n, key_value=kv).size, dtype=torch.uint8, device="cuda")
            gen = torch.Generator(device="cuda")

            def fresh(step):
                gen.manual_seed(args.seed * 1000003 + step)
                keys.copy_(random_keys(torch, n, gen))
                if kv:
                    values.copy_(payload)

            def run_ordered():
                vrdx.sort_segments64(sorter, keys, offsets, values=values, storage=storage, order=order, descending=descending)

            def run_workaround():
                transform_(keys, order, descending)
                vrdx.sort_segments64(sorter, keys, offsets, values=values, storage=storage)
                inverse_(keys, order, descending)

            def run_unordered():
                vrdx.sort_segments64(sorter, keys, offsets, values=values, storage=storage)

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
            result = {"shape": shape, "segments": len(sizes), "keys": n, "order": order, "descending": descending,
                      "key_value": kv, "rounds": args.rounds, "steps_per_round": args.steps,
                      "match": bool(torch.equal(a, b) and (not kv or torch.equal(av, bv))),
                      "status": sorter.read_sorter_status(torch.cuda.current_stream().cuda_stream)}
            line = summarise(result, ways, times)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del keys, values, storage, payload, outputs
            torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="")
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-steps", type=int, default=3, help="timed steps of the per-array loop (slow for many segments)")
    ap.add_argument("--only", default="", help="comma list of the ways to run (default: all three)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--keys64", action="store_true", help="uint64 keys: segmented64, composed, per_array, torch_sort")
    ap.add_argument("--patterns", default="uniform,tile_depth", help="--keys64: key patterns")
    ap.add_argument("--bits", type=int, nargs=2, action="append", metavar=("BEGIN", "END"),
                    help="sort by the key bits [BEGIN, END): range, workaround, whole_key (repeatable)")
    ap.add_argument("--rounds", type=int, default=5, help="--bits, --order: rounds of --steps timed steps")
    ap.add_argument("--order", default="", choices=["", "uint64", "int64", "float64"],
                    help="uint64 keys in a key order: ordered, workaround, unordered")
    ap.add_argument("--descending", action="store_true")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    if not torch.cuda.is_available():
        sys.exit("segmented_bench.py needs a GPU (there is no CPU fallback)")
    if args.bits:
        return main_bits(args)
    if args.order:
        return main_order(args)
    args.shapes = args.shapes or DEFAULT_SHAPES
    if args.keys64:
        return main64(args)
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    ways = [w for w in ("segmented", "per_array", "torch_sort") if not args.only or w in args.only.split(",")]
    out = open(args.out, "a") if args.out else None

    for shape in args.shapes.split(","):
        rng = np.random.default_rng(args.seed)
        sizes = segment_sizes(shape, rng)
        offsets_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(offsets_h[-1])
        offsets = torch.from_numpy(offsets_h.astype(np.uint32).view(np.int32)).cuda()
        seg_ids = torch.from_numpy(np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)).cuda()
        starts = [int(x) for x in offsets_h[:-1]]
        lengths = [int(x) for x in sizes]
        for mode in args.modes.split(","):
            kv = mode == "kv"
            keys = torch.empty(n, dtype=torch.int32, device="cuda")
            values = torch.empty(n, dtype=torch.int32, device="cuda") if kv else None
            req = (sorter.key_value_storage_requirements(n) if kv else sorter.storage_requirements(n)).size
            storage = torch.empty(req, dtype=torch.uint8, device="cuda")
            # the per-array loop's storage: the largest single sort's requirement
            big = max(lengths) if lengths else 0
            loop_storage = torch.empty(max(16, (sorter.key_value_storage_requirements(big) if kv
                                                else sorter.storage_requirements(big)).size), dtype=torch.uint8, device="cuda")
            gen = torch.Generator(device="cuda")
            stream = torch.cuda.current_stream()

            def fresh(step):
                gen.manual_seed(args.seed * 1000003 + step)
                keys.copy_(torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32))
                if kv:
                    values.copy_(torch.arange(n, dtype=torch.int32, device="cuda"))

            def run_segmented():
                vrdx.sort_segments(sorter, keys, offsets, values=values, storage=storage)

            def run_per_array():
                s = stream.cuda_stream
                kp, sp = keys.data_ptr(), loop_storage.data_ptr()
                for b, m in zip(starts, lengths):
                    if kv:
                        sorter.cmd_sort_key_value(s, m, kp, 4 * b, values.data_ptr(), 4 * b, sp, 0)
                    else:
                        sorter.cmd_sort(s, m, kp, 4 * b, sp, 0)

            torch_out = {}

            def run_torch_sort():
                packed = (seg_ids << 32) | (keys.to(torch.int64) & 0xFFFFFFFF)
                sorted_packed, idx = torch.sort(packed, stable=True)
                torch_out["keys"] = (sorted_packed & 0xFFFFFFFF).to(torch.int32)  # (wraps like the uint32 bit pattern)
                if kv:
                    torch_out["values"] = values[idx]

            fns = {"segmented": run_segmented, "per_array": run_per_array, "torch_sort": run_torch_sort}
            result = {"shape": shape, "segments": len(sizes), "keys": n, "key_value": kv,
                      "max_segment": big, "empty_segments": int((sizes == 0).sum())}
            outputs = {}
            for way in ways:
                steps = args.loop_steps if way == "per_array" else args.steps
                times = []
                for step in range(args.warmup + steps):
                    fresh(step)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[way]()
                    e1.record()
                    torch.cuda.synchronize()
                    if step >= args.warmup:
                        times.append(e0.elapsed_time(e1))
                result[way + "_ms"] = float(np.median(times))
                result[way + "_ms_min"] = float(np.min(times))
                if way == "segmented":
                    outputs["segmented"] = (keys.clone(), values.clone() if kv else None)
                    result["status"] = sorter.read_status(stream.cuda_stream, storage.data_ptr(), 0)
                elif way == "torch_sort":
                    outputs["torch_sort"] = (torch_out["keys"], torch_out.get("values"))
            if "segmented" in outputs and "torch_sort" in outputs:
                (a, av), (b, bv) = outputs["segmented"], outputs["torch_sort"]
                result["match"] = bool(torch.equal(a, b) and (not kv or torch.equal(av, bv)))  # (the same seeds: same input)
            if "segmented_ms" in result:
                for way in ("per_array", "torch_sort"):
                    if way + "_ms" in result:
                        result["speedup_vs_" + way] = result[way + "_ms"] / result["segmented_ms"]
                result["segmented_gkeys_s"] = n / (result["segmented_ms"] * 1e6)
            line = json.dumps(result)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del keys, values, storage, loop_storage
            torch.cuda.empty_cache()
    if out:
        out.close()
    sorter.destroy()


if __name__ == "__main__":
    main()
