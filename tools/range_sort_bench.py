#!/usr/bin/env python3
"""Times the range sorts at every size (vrdxHipCmdRangeSort[KeyValue]) on one GPU against what a caller had without them,
beyond the 16384 elements of vrdxHipCmdSortBits.  All variants run in ONE process and take turns, step by step, on fresh
copies of the same seeded keys; times are device-event times (a pair of torch events around what the variant enqueues, inputs
prepared and the device idle before the first event), medians over the steps after --warmup rounds; each row prints ONE
JSON line.

  range       (a) one vrdxHipCmdRangeSort[KeyValue] call
  workaround  (b) the documented workaround: extract the field and an iota in torch, vrdxCmdSortKeyValue on (field, iota),
              gather the keys (and the values) by the sorted index
  torch_sort  (c) a stable torch.sort of the field, and the same gathers
  masked      (d) vrdxCmdSort[KeyValue] on keys pre-masked to the field (the masking is not timed).  NOT the same result --
              the keys come back without their other bits -- quoted only as the price of the whole-key kernels
  segment     (e) vrdxHipCmdSortSegmentedBits[KeyValue] with the array as ONE segment: what the interface offered until now (one
              workgroup sorts it; its runs stop once they have taken --segment-budget-ms in a row, at least one is taken)

On one extra input per row (another seed) the result of (a) must equal that of (b) bit for bit ("match"); the program exits
with status 1 if any row does not.  Sizes beyond --large-from take --large-steps steps.

usage: python tools/range_sort_bench.py [--sizes 65536,...] [--ranges 0:1,0:8,8:24,4:28] [--modes keys,kv] [--steps 11]
       [--large-steps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(1 << k) for k in (16, 18, 20, 22, 24, 25, 27)))
    ap.add_argument("--ranges", default="0:1,0:8,8:24,4:28")
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--large-steps", type=int, default=5)
    ap.add_argument("--large-from", type=int, default=(1 << 24))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--segment-budget-ms", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    if not torch.cuda.is_available():
        sys.exit("range_sort_bench.py needs a GPU (there is no CPU fallback)")
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = open(args.out, "a") if args.out else None
    all_match = True

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        result = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), result

    def random_keys(n, seed):   # every bit random: 32-bit patterns held in int32
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        return torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)

    for n in (int(x) for x in args.sizes.split(",")):
        master = random_keys(n, args.seed)
        payload = (torch.arange(n, dtype=torch.int64, device="cuda") * 2654435761 & 0xFFFFFFFF).to(torch.int32)  # wraps to the bit pattern
        iota = torch.arange(n, dtype=torch.int32, device="cuda")
        offsets = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        steps = args.steps if n < args.large_from else args.large_steps
        for spec in args.ranges.split(","):
            begin, end = (int(x) for x in spec.split(":"))
            mask = (1 << (end - begin)) - 1

            def field_of(t):  # the field as a non-negative int32 bit pattern (width <= 31 here)
                return ((t.to(torch.int64) & 0xFFFFFFFF) >> begin & mask).to(torch.int32)

            for mode in args.modes.split(","):
                kv = mode == "kv"
                req = sorter.key_value_storage_requirements(n) if kv else sorter.storage_requirements(n)
                storage = torch.empty(req.size, dtype=torch.uint8, device="cuda")
                pair_storage = torch.empty(sorter.key_value_storage_requirements(n).size, dtype=torch.uint8, device="cuda")
                keys = torch.empty_like(master)
                values = torch.empty_like(payload) if kv else None
                masked_master = field_of(master)

                def load(source):
                    keys.copy_(source)
                    if kv:
                        values.copy_(payload)

                def range_sort():
                    if kv:
                        sorter.cmd_range_sort_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, begin, end,
                                                        storage.data_ptr(), 0)
                    else:
                        sorter.cmd_range_sort(stream, n, keys.data_ptr(), 0, begin, end, storage.data_ptr(), 0)

                def workaround(source):   # field + iota, a key+value sort, gathers
                    f = field_of(source)
                    index = iota.clone()
                    sorter.cmd_sort_key_value(stream, n, f.data_ptr(), 0, index.data_ptr(), 0, pair_storage.data_ptr(), 0)
                    index = index.to(torch.int64)
                    return source[index], (payload[index] if kv else None)

                def torch_sort():   # a stable torch.sort of the field, and the gathers
                    _, index = torch.sort(field_of(master), stable=True)
                    return master[index], (payload[index] if kv else None)

                def segment_sort():
                    if kv:
                        sorter.cmd_sort_segmented_bits_key_value(stream, n, 1, offsets.data_ptr(), 0, keys.data_ptr(), 0,
                                                                 values.data_ptr(), 0, begin, end, storage.data_ptr(), 0)
                    else:
                        sorter.cmd_sort_segmented_bits(stream, n, 1, offsets.data_ptr(), 0, keys.data_ptr(), 0, begin, end,
                                                       storage.data_ptr(), 0)

                times = {"range": [], "workaround": [], "torch_sort": [], "masked": [], "segment": []}
                segment_spent, segment_last = 0.0, None
                for step in range(args.warmup + steps):
                    keep = step >= args.warmup
                    load(master)
                    ms, _ = timed(range_sort)
                    if keep:
                        times["range"].append(ms)
                    ms, _ = timed(lambda: workaround(master))
                    if keep:
                        times["workaround"].append(ms)
                    ms, _ = timed(torch_sort)
                    if keep:
                        times["torch_sort"].append(ms)
                    # (d) the whole-key sort of masked keys (another result)
                    masked = masked_master.clone()
                    masked_values = payload.clone() if kv else None

                    def masked_sort():
                        if kv:
                            sorter.cmd_sort_key_value(stream, n, masked.data_ptr(), 0, masked_values.data_ptr(), 0,
                                                      storage.data_ptr(), 0)
                        else:
                            sorter.cmd_sort(stream, n, masked.data_ptr(), 0, storage.data_ptr(), 0)

                    ms, _ = timed(masked_sort)
                    if keep:
                        times["masked"].append(ms)
                    del masked, masked_values
                    # (e) the array as one segment
                    if segment_last is None or segment_spent < args.segment_budget_ms:
                        load(master)
                        segment_last, _ = timed(segment_sort)
                        segment_spent += segment_last
                        if keep:
                            times["segment"].append(segment_last)
                if not times["segment"]:   # (the budget ran out in the warm-up rounds)
                    times["segment"].append(segment_last)
                # one extra input: (a) against (b), bit for bit
                extra = random_keys(n, args.seed + 1000)
                load(extra)
                range_sort()
                want_keys, want_values = workaround(extra)
                torch.cuda.synchronize()
                match = bool(torch.equal(keys, want_keys) and (not kv or torch.equal(values, want_values)))
                all_match = all_match and match
                info = sorter.describe_range_sort_plan(n, kv, begin, end)
                result = {"n": n, "begin_bit": begin, "end_bit": end, "key_value": kv, "form": info.name, "chunks": info.chunks,
                          "keys_per_chunk": info.keysPerChunk, "digits": info.digits, "launches": info.launches,
                          "bytes_per_element_per_pass": info.bytesPerElementPerPass,
                          "bytes_per_element_copy_back": info.bytesPerElementCopyBack, "steps": steps,
                          "segment_steps": len(times["segment"])}
                for name, xs in times.items():
                    result[name + "_ms"] = float(np.median(xs))
                    result[name + "_min_ms"] = float(np.min(xs))
                    result[name + "_max_ms"] = float(np.max(xs))
                for name in ("workaround", "torch_sort", "masked", "segment"):
                    result[name + "_over_range"] = result[name + "_ms"] / result["range_ms"]
                result["masked_plan"] = sorter.describe_plan(n, kv).name
                result["status"] = sorter.read_status(stream, storage.data_ptr(), 0)
                result["match"] = match
                line = json.dumps(result)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del storage, pair_storage, keys, values, masked_master, extra, want_keys, want_values
                torch.cuda.empty_cache()
        del master, payload, iota, offsets
    if out:
        out.close()
    sorter.destroy()
    sys.exit(0 if all_match else 1)


if __name__ == "__main__":
    main()
