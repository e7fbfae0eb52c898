#!/usr/bin/env python
"""Rates of the per-axis convolution kernel (csrc/conv_rect.hip) beside the square direct kernels, in one process.

N = 32, 64 x 64, C = K = 128, stride 1, `half`: the three passes of conv_rect for 1x7, 7x1 and 3x3, and the square direct kernels
(denet_conv_fwd / _dgrad / _wgrad, no Winograd) on the same 3x3. Device events around single launches, warm-up, median of the
repeats. Prints a table and one JSON line.

    python tools/bench_conv_rect.py [--reps 30] [--warmup 5] [--batch 32] [--size 64] [--channels 128]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--channels", type=int, default=128)
    args = ap.parse_args()
    N, H, C = args.batch, args.size, args.channels
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(N, H, H, C, generator=g).cuda()
    dy = torch.randn(N, H, H, C, generator=g).cuda()
    rows = []

    def add(name, R, S, passes):
        flops = 2.0 * N * H * H * C * C * R * S
        for pname, fn in passes:
            med, lo, hi = median_ms(fn, args.reps, args.warmup)
            rows.append({"kernel": name, "filter": "%dx%d" % (R, S), "pass": pname, "ms": round(med, 4), "min_ms": round(lo, 4),
                         "max_ms": round(hi, 4), "tflops": round(flops / med * 1e-9, 2)})

    for R, S in ((1, 7), (7, 1), (3, 3)):
        w = (torch.randn(C, R, S, C, generator=g) / (C * R * S) ** 0.5).cuda()
        kw = dict(stride=(1, 1), pad=(R // 2, S // 2))
        y, dx, dw = ops.empty(N, H, H, C), ops.empty(N, H, H, C), ops.empty(C, R, S, C)
        add("conv_rect", R, S, [("fwd", lambda: ops.conv_rect_fwd(x, w, out=y, **kw)),
                                ("dgrad", lambda: ops.conv_rect_dgrad(dy, w, tuple(x.shape), out=dx, **kw)),
                                ("wgrad", lambda: ops.conv_rect_wgrad(x, dy, tuple(w.shape), out=dw, **kw))])
    # the square direct kernels on the 3x3 (ops.POLICY pins the direct implementation: no Winograd, no fused kernel)
    w = (torch.randn(C, 3, 3, C, generator=g) / (C * 9) ** 0.5).cuda()
    ops._load_tuned_once()             # (before the table is emptied: the first decision would load the committed file)
    saved = (ops.POLICY, dict(ops._WINO))
    ops._WINO.clear()
    ops.POLICY = lambda mode, gg: 0
    try:
        y, dx, dw = ops.empty(N, H, H, C), ops.empty(N, H, H, C), ops.empty(C, 3, 3, C)
        add("igemm (square direct)", 3, 3, [("fwd", lambda: ops.conv_fwd(x, w, stride=1, pad=1, out=y)),
                                            ("dgrad", lambda: ops.conv_dgrad(dy, w, tuple(x.shape), stride=1, pad=1, out=dx)),
                                            ("wgrad", lambda: ops.conv_wgrad(x, dy, tuple(w.shape), stride=1, pad=1, out=dw))])
    finally:
        ops.POLICY = saved[0]
        ops._WINO.clear()
        ops._WINO.update(saved[1])
    base = {r["pass"]: r["ms"] for r in rows if r["kernel"].startswith("igemm")}
    print("%-22s %-6s %-6s %9s %9s %9s %8s %s" % ("kernel", "filter", "pass", "median ms", "min", "max", "TFLOP/s", "vs square 3x3"))
    for r in rows:
        ratio = "%.2fx" % (r["ms"] / base[r["pass"]]) if r["kernel"] == "conv_rect" and r["filter"] == "3x3" else ""
        print("%-22s %-6s %-6s %9.4f %9.4f %9.4f %8.2f %s" % (r["kernel"], r["filter"], r["pass"], r["ms"], r["min_ms"], r["max_ms"],
                                                              r["tflops"], ratio))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "HW": H, "C": C, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
