#!/usr/bin/env python
"""A plain training step against a step with global-norm gradient clipping (`model-train --gradient-clip`, csrc/grad_norm.hip), in
ONE process.

  1. DeNet-34 skip 512x512 training steps at batch 32 (the model and batch of bench.py): one plain model and one whose limit lies
     far above the norm (coef = 1: both train alike; their RoI draws come from one shared random stream, so their parameters are
     not compared bit for bit here - tests/test_grad_clip_gpu.py does that on seeded twins), blocks of steps of the two interleaved (the order inside a pair
     alternates), host clock around a synchronised block; median, minimum and maximum ms per step, images/s.
  2. the norm pass alone (grad_norm_partial_kernel + grad_norm_finish_kernel over the clipped model's gradient buffer, nothing
     beside it): event pairs around blocks of calls, the bytes of G the pass reads and the GB/s that amounts to.

The cost is one extra read of the gradient buffer and two launch boundaries in front of the solver; the tool reports it against the
plain model of the same process and promises nothing. bench.py never sets a limit.

    python tools/bench_grad_clip.py [--pairs 6] [--steps 3] [--warmup 3] [--batch 32] [--image 512]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402
from denet_amd.model import zoo  # noqa: E402

KINDS = ("plain", "clipped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--alone-calls", type=int, default=20)
    args = ap.parse_args()
    B, image = args.batch, args.image
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    lr, mom, decay = 0.1, [0.9], 1e-4
    models = {k: zoo.denet34(B, "skip", image, class_num=80, seed=1) for k in KINDS}
    models["clipped"].gradient_clip = 1e30
    it = {k: 0 for k in KINDS}

    def run(k, n):
        for _ in range(n):
            cost, _ = models[k].train_step(xd, metas, 0, it[k], lr, mom, decay)
            it[k] += 1
        return cost

    for k in KINDS:
        models[k].build_train_func("nesterov")
        run(k, max(args.warmup, 2))
    torch.cuda.synchronize()
    ms, costs = {k: [] for k in KINDS}, {k: [] for k in KINDS}
    for i in range(args.pairs):
        for k in (KINDS if i % 2 == 0 else KINDS[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cost = run(k, args.steps)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            costs[k].append(round(float(cost), 4))
    m = models["clipped"]
    norm, coef = m.last_grad_norm()
    st = m.grad_norm_stats()
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "image": image, "pairs": args.pairs, "steps_per_block": args.steps,
           "last_norm": norm, "last_coef": coef, "steps_recorded": st["steps"], "steps_clipped": st["clipped"],
           "same_parameters": bool(torch.equal(models["plain"].P, m.P))}
    for k in KINDS:
        med = statistics.median(ms[k])
        out[k] = {"median_ms_per_step": round(med, 3), "min_ms_per_step": round(min(ms[k]), 3), "max_ms_per_step": round(max(ms[k]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "cost_after_each_block": costs[k]}
    out["clipped_over_plain_time"] = round(out["clipped"]["median_ms_per_step"] / out["plain"]["median_ms_per_step"], 4)
    # the two new launches alone
    nt = m._norm
    alone = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.alone_calls):
            ops.grad_norm(m.G, nt, 1.0, 1e30)
        e1.record()
        e1.synchronize()
        alone.append(e0.elapsed_time(e1) / args.alone_calls)
    alone_ms = statistics.median(alone)
    out["norm_pass"] = {"chunks": nt.n_chunks, "segments": nt.n_segments, "bytes_read": nt.bytes_read, "alone_ms": round(alone_ms, 4),
                        "alone_ms_min": round(min(alone), 4), "alone_ms_max": round(max(alone), 4),
                        "gb_per_s": round(nt.bytes_read / (alone_ms * 1e-3) / 1e9, 1)}
    print("train_step B=%d %dx%d: plain %.3f ms (min %.3f, max %.3f) = %.1f img/s | clipped %.3f ms (min %.3f, max %.3f) = %.1f img/s | "
          "clipped / plain time %.4f | same parameters: %s" % (
              B, image, image, out["plain"]["median_ms_per_step"], out["plain"]["min_ms_per_step"], out["plain"]["max_ms_per_step"],
              out["plain"]["images_per_s"], out["clipped"]["median_ms_per_step"], out["clipped"]["min_ms_per_step"],
              out["clipped"]["max_ms_per_step"], out["clipped"]["images_per_s"], out["clipped_over_plain_time"], out["same_parameters"]),
          flush=True)
    print("  norm pass alone: %d chunks, %d segments, %.1f MB of G read in %.4f ms (min %.4f, max %.4f) = %.1f GB/s" % (
        nt.n_chunks, nt.n_segments, nt.bytes_read / 1e6, alone_ms, min(alone), max(alone), out["norm_pass"]["gb_per_s"]))
    print("  costs after each timed block: plain %s | clipped %s" % (costs["plain"], costs["clipped"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
