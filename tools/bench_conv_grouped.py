#!/usr/bin/env python
"""The grouped convolution kernel (csrc/conv_rect.hip, conv_grp_kernel) alone, per pass, against two yardsticks.

Geometries: the grouped 3x3 layers of ResNeXt-50 32x4d at 224 x 224, batch 32, at each of its four widths (128 @ 56x56, 256 @ 28x28,
512 @ 14x14, 1024 @ 7x7, 32 groups: Cg = 4, 8, 16 on the slab path, 32 on the window path), at stride 1 - where `zoo.resnext50`
has them: this grammar's bottleneck strides its first 1x1 layer - and the three stride-2 forms of the published layout (256 @ 56x56,
512 @ 28x28, 1024 @ 14x14), and a depthwise 3x3 on 128 channels at 64x64. Per pass the median of --reps (20) calls after --warmup,
timed with device events around the whole call (the slab path's filter expansion is made once and kept, as in a layer; its
gradient compaction is part of the filter-gradient call), beside
  (a) the dense layer of the same C, K and geometry on ops.conv_rect_* (calls alternating), and
  (b) the time the pass's compulsory bytes - input, output and the compact filter, once each - take at the copy rate on record
      (EXPERIMENTS.md / VERDICT.md: 6.29 TB/s).
Every geometry runs in a child process of its own under a time limit; the first one that fails ends the run. Prints a table and
one JSON line.

    python tools/bench_conv_grouped.py [--reps 20] [--warmup 5] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29
#             name                        N   H    C     g     stride
GEOMETRIES = [("resnext50 128@56 s1", 32, 56, 128, 32, 1), ("resnext50 256@28 s1", 32, 28, 256, 32, 1),
              ("resnext50 512@14 s1", 32, 14, 512, 32, 1), ("resnext50 1024@7 s1", 32, 7, 1024, 32, 1),
              ("published 256@56 s2", 32, 56, 256, 32, 2), ("published 512@28 s2", 32, 28, 512, 32, 2),
              ("published 1024@14 s2", 32, 14, 1024, 32, 2), ("depthwise 128@64 s1", 32, 64, 128, 128, 1)]


def one(index, reps, warmup):
    import torch
    from denet_amd import ops
    name, N, H, C, groups, st = GEOMETRIES[index]
    Cg = C // groups
    gen = torch.Generator(device="cpu").manual_seed(index)
    OH = (H + 2 - 3) // st + 1
    x = torch.randn(N, H, H, C, generator=gen).cuda()
    dy = torch.randn(N, OH, OH, C, generator=gen).cuda()
    w = (torch.randn(C, 3, 3, Cg, generator=gen) / (9 * Cg) ** 0.5).cuda()
    wd = (torch.randn(C, 3, 3, C, generator=gen) / (9 * C) ** 0.5).cuda()
    y, dx, dw, dwd = ops.empty(N, OH, OH, C), ops.empty(N, H, H, C), ops.empty(C, 3, 3, Cg), ops.empty(C, 3, 3, C)
    kw = dict(stride=(st, st), pad=(1, 1))
    cache = {}
    passes = [("fwd", lambda: ops.conv_grp_fwd(x, w, groups, out=y, cache=cache, **kw), lambda: ops.conv_rect_fwd(x, wd, out=y, **kw)),
              ("dgrad", lambda: ops.conv_grp_dgrad(dy, w, tuple(x.shape), groups, out=dx, cache=cache, **kw),
               lambda: ops.conv_rect_dgrad(dy, wd, tuple(x.shape), out=dx, **kw)),
              ("wgrad", lambda: ops.conv_grp_wgrad(x, dy, tuple(w.shape), groups, out=dw, **kw),
               lambda: ops.conv_rect_wgrad(x, dy, tuple(wd.shape), out=dwd, **kw))]

    def timed_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    rows = []
    for pname, f_grp, f_dense in passes:
        for _ in range(warmup):
            f_grp()
            f_dense()
        torch.cuda.synchronize()
        tg, td = [], []
        for _ in range(reps):
            tg.append(timed_ms(f_grp))
            td.append(timed_ms(f_dense))
        gm, dm = statistics.median(tg), statistics.median(td)
        nbytes = 4.0 * (x.numel() + y.numel() + w.numel())
        floor_ms = nbytes / (COPY_TBS * 1e12) * 1e3
        flops = 2.0 * N * OH * OH * C * 9 * Cg
        rows.append({"geometry": name, "Cg": Cg, "pass": pname, "grp_ms": round(gm, 4), "grp_min": round(min(tg), 4),
                     "dense_ms": round(dm, 4), "vs_dense": round(gm / dm, 3), "floor_ms": round(floor_ms, 4),
                     "vs_floor": round(gm / floor_ms, 2), "grp_tflops": round(flops / gm * 1e-9, 2)})
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds one geometry's child process may take")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.reps, args.warmup)
    rows, device = [], None
    for i in range(len(GEOMETRIES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(i), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit("%s: no result within %d s - stopping" % (GEOMETRIES[i][0], args.limit))
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit("%s: exit status %d - stopping" % (GEOMETRIES[i][0], r.returncode))
        out = json.loads(r.stdout.strip().splitlines()[-1])
        device = out["device"]
        rows += out["rows"]
    print("%-22s %3s %-6s %10s %10s %9s %10s %9s %9s" % ("geometry", "Cg", "pass", "grouped ms", "dense ms", "vs dense", "floor ms",
                                                         "vs floor", "TFLOP/s"))
    for r in rows:
        print("%-22s %3d %-6s %10.4f %10.4f %8.3fx %10.4f %8.2fx %9.2f" % (
            r["geometry"], r["Cg"], r["pass"], r["grp_ms"], r["dense_ms"], r["vs_dense"], r["floor_ms"], r["vs_floor"], r["grp_tflops"]))
    print(json.dumps({"device": device, "reps": args.reps, "copy_tbs": COPY_TBS, "rows": rows}))


if __name__ == "__main__":
    main()
