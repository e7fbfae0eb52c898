#!/usr/bin/env python
"""Plain batch norm against batch renormalisation (`model-modify --modify-bn-renorm 3 5 0`, csrc/bn_renorm.hip), in ONE process.

  1. DeNet-34 skip 512x512 training steps at batch 32 (the model and batch of bench.py): one plain model and one whose every batch
     norm is renorm-active (same weights), blocks of steps of the two interleaved (the order inside a pair alternates), host clock
     around a synchronised block; median, minimum and maximum ms per step, images/s.
  2. one profiled step of the renorm model (event pairs around the launches, the step's two streams kept): the summed time of the
     bn_renorm_stats_finish_kernel / bn_renorm_grad_fold_kernel launches and their count.

A renorm-active layer gives up the linked, pool-fused and producer-finished forms of the batch norm, so the
renorm model is expected to be slower; the tool reports by how much and promises nothing. bench.py never builds such a model.

    python tools/bench_bn_renorm.py [--pairs 6] [--steps 3] [--warmup 3] [--batch 32] [--image 512]"""
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
from denet_amd.layer.batch_norm import renorm_layers  # noqa: E402
from denet_amd.model import modify, zoo  # noqa: E402

KINDS = ("plain", "renorm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=512)
    args = ap.parse_args()
    B, image = args.batch, args.image
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    lr, mom, decay = 0.1, [0.9], 1e-4
    plain = zoo.denet34(B, "skip", image, class_num=80, seed=1)
    models = {"plain": plain, "renorm": modify.modify_bn_renorm(plain, 3, 5, 0)}
    active = len(renorm_layers(models["renorm"]))
    assert active > 0 and not renorm_layers(plain)
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
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "image": image, "pairs": args.pairs, "steps_per_block": args.steps,
           "renorm_active_layers": active}
    for k in KINDS:
        med = statistics.median(ms[k])
        out[k] = {"median_ms_per_step": round(med, 3), "min_ms_per_step": round(min(ms[k]), 3), "max_ms_per_step": round(max(ms[k]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "cost_after_each_block": costs[k]}
    out["renorm_over_plain_time"] = round(out["renorm"]["median_ms_per_step"] / out["plain"]["median_ms_per_step"], 3)
    # the new launches inside one step of the renorm model
    ops.PROFILE = ops.KernelProfile(alone=False)
    try:
        models["renorm"].train_step(xd, metas, 0, it["renorm"], lr, mom, decay)
        agg = ops.PROFILE.summary()
    finally:
        ops.PROFILE = None
    new = {n: {"launches": agg[n]["launches"], "ms": round(agg[n]["ms"], 4)} for n in ops.RENORM_KERNELS if n in agg}
    out["new_launches"] = new
    out["new_launches_ms_per_step"] = round(sum(v["ms"] for v in new.values()), 4)
    print("train_step B=%d %dx%d, %d renorm-active layers: plain %.3f ms (min %.3f, max %.3f) = %.1f img/s | renorm %.3f ms (min %.3f, "
          "max %.3f) = %.1f img/s | renorm / plain time %.3f" % (
              B, image, image, active, out["plain"]["median_ms_per_step"], out["plain"]["min_ms_per_step"],
              out["plain"]["max_ms_per_step"], out["plain"]["images_per_s"], out["renorm"]["median_ms_per_step"],
              out["renorm"]["min_ms_per_step"], out["renorm"]["max_ms_per_step"], out["renorm"]["images_per_s"],
              out["renorm_over_plain_time"]), flush=True)
    print("  new launches in one step: %s = %.4f ms" % (
        ", ".join("%s x%d %.4f ms" % (n, v["launches"], v["ms"]) for n, v in new.items()), out["new_launches_ms_per_step"]))
    print("  costs after each timed block: plain %s | renorm %s" % (costs["plain"], costs["renorm"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
