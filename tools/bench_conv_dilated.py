#!/usr/bin/env python
"""The dilated convolution kernel (csrc/conv_rect.hip, conv_dil_kernel) beside the undilated one (conv_rect_kernel), in one process.

Per pass, `conv_dil_*` with dilation (2, 2) against `conv_rect_*` (dilation 1) at the same N, H, W, C, K, 3x3 filter and `half`
padding: the same output size and the same FLOPs, and the conv_rect instantiations are the undilated layers' own device code.
Geometries: 32 x 64x64 x 128 -> 128 and 32 x 32x32 x 256 -> 256. The two calls alternate; one run is the median of --reps (20)
calls of each, timed with device events around single launches; --runs (5) runs, of which the median and the range are printed.
Prints a table and one JSON line.

    python tools/bench_conv_dilated.py [--reps 20] [--runs 5] [--warmup 5] [--dilation 2]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402

GEOMETRIES = [(32, 64, 128), (32, 32, 256)]          # N, H = W, C = K


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved_medians(fa, fb, reps, warmup):
    """the medians of `reps` calls of fa and of fb, the calls alternating"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed_ms(fa))
        tb.append(timed_ms(fb))
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dilation", type=int, default=2)
    args = ap.parse_args()
    d = args.dilation
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for N, H, C in GEOMETRIES:
        x = torch.randn(N, H, H, C, generator=g).cuda()
        dy = torch.randn(N, H, H, C, generator=g).cuda()
        w = (torch.randn(C, 3, 3, C, generator=g) / (9 * C) ** 0.5).cuda()
        y, dx, dw = ops.empty(N, H, H, C), ops.empty(N, H, H, C), ops.empty(C, 3, 3, C)
        rect = dict(stride=(1, 1), pad=(1, 1))
        dil = dict(stride=(1, 1), pad=(d, d), dilation=(d, d))
        assert ops.conv_dil_geom(tuple(x.shape), tuple(w.shape), (1, 1), (d, d), (d, d))[14:] == (H, H)
        passes = [("fwd", lambda: ops.conv_rect_fwd(x, w, out=y, **rect), lambda: ops.conv_dil_fwd(x, w, out=y, **dil)),
                  ("dgrad", lambda: ops.conv_rect_dgrad(dy, w, tuple(x.shape), out=dx, **rect),
                   lambda: ops.conv_dil_dgrad(dy, w, tuple(x.shape), out=dx, **dil)),
                  ("wgrad", lambda: ops.conv_rect_wgrad(x, dy, tuple(w.shape), out=dw, **rect),
                   lambda: ops.conv_dil_wgrad(x, dy, tuple(w.shape), out=dw, **dil))]
        flops = 2.0 * N * H * H * C * C * 9
        for pname, f_rect, f_dil in passes:
            runs = [interleaved_medians(f_rect, f_dil, args.reps, args.warmup) for _ in range(args.runs)]
            r_ms, d_ms = [r for r, _ in runs], [v for _, v in runs]
            rm, dm = statistics.median(r_ms), statistics.median(d_ms)
            rows.append({"geometry": "%dx%dx%dx%d->%d" % (N, H, H, C, C), "pass": pname, "dilation": d,
                         "rect_ms": round(rm, 4), "rect_min": round(min(r_ms), 4), "rect_max": round(max(r_ms), 4),
                         "dil_ms": round(dm, 4), "dil_min": round(min(d_ms), 4), "dil_max": round(max(d_ms), 4),
                         "ratio": round(dm / rm, 3), "rect_tflops": round(flops / rm * 1e-9, 1), "dil_tflops": round(flops / dm * 1e-9, 1)})
    print("%-20s %-6s %28s %28s %7s" % ("geometry", "pass", "conv_rect d1: ms (range) TFLOP/s", "conv_dil d%d: ms (range) TFLOP/s" % d,
                                        "ratio"))
    for r in rows:
        print("%-20s %-6s %8.4f (%.4f-%.4f) %6.1f %8.4f (%.4f-%.4f) %6.1f %6.3fx" % (
            r["geometry"], r["pass"], r["rect_ms"], r["rect_min"], r["rect_max"], r["rect_tflops"], r["dil_ms"], r["dil_min"],
            r["dil_max"], r["dil_tflops"], r["ratio"]))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "runs": args.runs, "rows": rows}))


if __name__ == "__main__":
    main()
