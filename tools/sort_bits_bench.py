#!/usr/bin/env python3
"""Times the bit-range sorts (vrdxHipCmdSortBits[KeyValue]) on one GPU against what a caller has without them, at the sizes
they are built for (one workgroup: up to 16384 elements -- latencies, not bandwidth).  All variants run in ONE process and
take turns, step by step, on fresh copies of the same seeded keys; times are device-event times, medians over --steps
after --warmup rounds; each shape prints ONE JSON line.

ONE clock for all four: a pair of torch events around what the variant enqueues, inputs prepared and the device idle before
the first event.  At these sizes that is mostly the time the host needs to launch the variant's kernels -- one for (a), six
or more for (b) and (c) -- which is what a caller of a sort this small pays; `range_kernel_ms` adds, for (a) only, the span of
its one kernel by the call's own query pool (ts[14] - ts[0]) in a second, stamped call; no timed call carries a pool.

  range       (a) one vrdxHipCmdSortBits[KeyValue] call
  workaround  (b) what a caller does without it: extract the field and an iota in torch, vrdxCmdSortKeyValue on (field, iota),
              gather the keys (and the values) by the sorted index -- three extra kernels and two extra arrays
  torch_sort  (c) a stable torch.sort of the field, and the same gathers
  masked      (d) vrdxCmdSort[KeyValue] on keys pre-masked to the field (the masking is not timed).  NOT the same result --
              the keys come back without their other bits -- quoted only as the price of the whole-key plans on such keys

The result of (a) in the last round is compared with that of (b) and (c), element for element ("match").  bytes_per_element is
what vrdxHipDescribeSortBitsPlan states for (a).

usage: python tools/sort_bits_bench.py [--sizes 4096,16384] [--ranges 0:8,8:24,4:28] [--modes keys,kv] [--steps 51]
       [--warmup 5] [--out FILE]
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
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--ranges", default="0:8,8:24,4:28")
    ap.add_argument("--modes", default="keys,kv")
    ap.add_argument("--steps", type=int, default=51)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import vulkan_radix_sort_amd as vrdx

    if not torch.cuda.is_available():
        sys.exit("sort_bits_bench.py needs a GPU (there is no CPU fallback)")
    torch.cuda.set_device(0)
    sorter = vrdx.Sorter(0)
    stream = torch.cuda.current_stream().cuda_stream
    pool = vrdx.QueryPool(15)
    out = open(args.out, "a") if args.out else None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        result = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), result

    for n in (int(x) for x in args.sizes.split(",")):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(args.seed)
        # every bit random: 32-bit patterns held in int32
        master = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)
        payload = (torch.arange(n, dtype=torch.int64, device="cuda") * 2654435761 & 0xFFFFFFFF).to(torch.int32)  # wraps to the bit pattern
        iota = torch.arange(n, dtype=torch.int32, device="cuda")
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
                times = {"range": [], "range_kernel": [], "workaround": [], "torch_sort": [], "masked": []}
                last = {}
                for step in range(args.warmup + args.steps):
                    keep = step >= args.warmup
                    # (a) the range sort
                    keys.copy_(master)
                    if kv:
                        values.copy_(payload)

                    def range_sort(query_pool=None):
                        if kv:
                            sorter.cmd_sort_bits_key_value(stream, n, keys.data_ptr(), 0, values.data_ptr(), 0, begin, end,
                                                           storage.data_ptr(), 0, query_pool, 0)
                        else:
                            sorter.cmd_sort_bits(stream, n, keys.data_ptr(), 0, begin, end, storage.data_ptr(), 0, query_pool, 0)

                    range_sort(pool)   # (once more with the call's own stamps, on the keys as they are: the kernel's span)
                    torch.cuda.synchronize()
                    if keep:
                        times["range_kernel"].append(pool.results_ns(0, 15)[14] / 1e6)
                    keys.copy_(master)
                    if kv:
                        values.copy_(payload)
                    ms, _ = timed(range_sort)
                    if keep:
                        times["range"].append(ms)

                    # (b) field + iota, a key+value sort, gathers
                    def workaround():
                        f = field_of(master)
                        index = iota.clone()
                        sorter.cmd_sort_key_value(stream, n, f.data_ptr(), 0, index.data_ptr(), 0, pair_storage.data_ptr(), 0)
                        gathered = master[index.to(torch.int64)]
                        return gathered, (payload[index.to(torch.int64)] if kv else None)

                    ms, last["workaround"] = timed(workaround)
                    if keep:
                        times["workaround"].append(ms)

                    # (c) a stable torch.sort of the field, and the gathers
                    def torch_sort():
                        _, index = torch.sort(field_of(master), stable=True)
                        return master[index], (payload[index] if kv else None)

                    ms, last["torch_sort"] = timed(torch_sort)
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
                info = sorter.describe_sort_bits_plan(n, kv, begin, end)
                whole = sorter.describe_plan(n, kv)
                result = {"n": n, "begin_bit": begin, "end_bit": end, "key_value": kv, "plan": info.name, "launches": info.launches,
                          "bytes_per_element": info.bytesPerElement}
                for name, xs in times.items():
                    result[name + "_ms"] = float(np.median(xs))
                    result[name + "_min_ms"] = float(np.min(xs))
                    result[name + "_max_ms"] = float(np.max(xs))
                result["workaround_over_range"] = result["workaround_ms"] / result["range_ms"]
                result["torch_sort_over_range"] = result["torch_sort_ms"] / result["range_ms"]
                result["masked_plan"] = whole.name
                result["masked_over_range"] = result["masked_ms"] / result["range_ms"]
                result["status"] = sorter.read_status(stream, storage.data_ptr(), 0)
                result["match"] = bool(all(torch.equal(keys, last[v][0]) and (not kv or torch.equal(values, last[v][1]))
                                           for v in ("workaround", "torch_sort")))
                line = json.dumps(result)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del storage, pair_storage, keys, values, masked_master, last
                torch.cuda.empty_cache()
        del master, payload, iota
    if out:
        out.close()
    pool.destroy()
    sorter.destroy()


if __name__ == "__main__":
    main()
