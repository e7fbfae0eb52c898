#!/usr/bin/env python
"""Times of the border-keeping max pool (csrc/pool_border.hip) beside the cuDNN-mode max pool (csrc/pool.hip), in one process.

The stem geometry of the 512 x 512 benchmark: N = 32, 256 x 256 x 64 in, 3 x 3 stride 2 -> 128 x 128 out (`P.B[3,2]` clips its last
window; `P[3,2,1]` pads by one). Device events around single launches, warm-up, the two kernels of a pass alternated, median of
the repeats. GB/s counts the bytes the pass must move: forward x + y (+ the argmax bytes of the cuDNN mode), backward
dy + dx (+ argmax, cuDNN mode) or x + y + dy + dx (border-keeping: it tests x == y instead of reading an argmax tensor).
Prints a table and one JSON line.

    python tools/bench_pool_border.py [--reps 50] [--warmup 5] [--batch 32] [--size 256] [--channels 64]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402


def alternate_ms(fns, reps, warmup):
    """fns: {name: callable}; every repeat runs each once, in turn -> {name: (median, min, max)} in ms"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=64)
    args = ap.parse_args()
    N, H, C = args.batch, args.size, args.channels
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(N, H, H, C, generator=g).cuda()
    yb = ops.maxpool_border_fwd(x, (3, 3), (2, 2))
    yc, arg = ops.maxpool_fwd(x, 3, 2, 1)
    assert tuple(yb.shape) == tuple(yc.shape)
    dy = torch.randn(tuple(yb.shape), generator=g).cuda()
    nx, ny = x.numel() * 4, yb.numel() * 4
    fwd = alternate_ms({"border": lambda: ops.maxpool_border_fwd(x, (3, 3), (2, 2)),
                        "cudnn": lambda: ops.maxpool_fwd(x, 3, 2, 1)}, args.reps, args.warmup)
    bwd = alternate_ms({"border": lambda: ops.maxpool_border_bwd(x, yb, dy, (3, 3), (2, 2)),
                        "cudnn": lambda: ops.maxpool_bwd(dy, arg, tuple(x.shape), 3, 2, 1)}, args.reps, args.warmup)
    nbytes = {("fwd", "border"): nx + ny, ("fwd", "cudnn"): nx + ny + arg.numel(),
              ("bwd", "border"): 2 * nx + 2 * ny, ("bwd", "cudnn"): nx + ny + arg.numel()}
    rows = []
    print("%-5s %-22s %9s %9s %9s %8s" % ("pass", "kernel", "median ms", "min", "max", "GB/s"))
    for pname, res in (("fwd", fwd), ("bwd", bwd)):
        for k, (med, lo, hi) in res.items():
            name = "P.B[3,2] (pool_border)" if k == "border" else "P[3,2,1] (pool)"
            rows.append({"pass": pname, "kernel": name, "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                         "gbps": round(nbytes[(pname, k)] / med * 1e-6, 1)})
            print("%-5s %-22s %9.4f %9.4f %9.4f %8.1f" % (pname, name, med, lo, hi, rows[-1]["gbps"]))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "HW": H, "C": C, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
