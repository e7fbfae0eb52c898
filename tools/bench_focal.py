#!/usr/bin/env python
"""Plain against focal cost (focalGamma 2 on the corner and the detection layer; csrc/focal.hip), in ONE process.

DeNet-34 skip 512x512, two models from the same seed that differ in the two layers' focalGamma alone, a warmed corner head
(zoo.warm_corner_head), training steps of the two models interleaved (the order inside a pair alternates), host clock around every
synchronised step, median over the steps of a model. Learning rate 0: every step sees the same detector. Reported per mode: ms per
step, and the two cost calls measured ALONE (device events around the ops call on the last step's own log-probabilities, logits and
targets, median of 20 after 3 unmeasured calls; a call is the cost kernel plus its one or two single-workgroup finishing sums).
No ratio is promised, the mode stays opt-in. bench.py never turns it on. Not measured here: whether a detector trained with the
focal cost is more accurate, and multi-GPU steps.

    python tools/bench_focal.py [--batch 32] [--steps 20] [--warmup 3] [--image 512] [--bias 7.5] [--gamma 2]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402
from denet_amd.model import zoo  # noqa: E402

MODES = ("plain", "focal")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alone(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = [event_ms(fn) for _ in range(reps)]
    return {"median_us": round(1e3 * statistics.median(t), 1), "min_us": round(1e3 * min(t), 1)}


def build(mode, B, image, bias, gamma):
    desc = zoo.DENET34_SKIP_DESC
    if mode == "focal":
        desc = desc.replace("DNC[96,100]", "DNC[96,100,0,%g]" % gamma).replace("DND[0.5,1,1]", "DND[0.5,1,1,0,%g]" % gamma)
    model = zoo.denet34(B, "skip", image, class_num=80, seed=1, head_desc=desc)
    zoo.warm_corner_head(model, bias, 0.3)
    model.build_train_func("nesterov")
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    dnc, dnd = by_type("denet-corner"), by_type("denet-detect")
    assert dnc.focal_gamma == dnd.focal_gamma == (gamma if mode == "focal" else 0.0)
    return model, by_type("denet-sparse"), dnc, dnd


def kernels_alone(dnc, dnd):
    """the two cost calls of the layers, as loss_backward makes them, on the last step's tensors, each alone on the compute stream"""
    cost = torch.zeros(2, device="cuda")
    ctx = type("Ctx", (), {"has_sparse": True})()
    out = {"corner_cost": alone(lambda: dnc.loss_backward(ctx, cost)), "detect_cost": alone(lambda: dnd.loss_backward(ctx, cost))}
    B, _, cn, H, W = dnc.corner_pr.shape
    out["corner_cells"] = B * cn * H * W
    out["rois"], out["classes"] = dnd.batch_size * dnd.sample_num ** 2, dnd.s0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--bias", type=float, default=7.5, help="corner head bias of zoo.warm_corner_head")
    ap.add_argument("--gamma", type=float, default=2.0)
    args = ap.parse_args()
    B = args.batch
    x, metas = zoo.synthetic_batch(B, args.image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    models = {m: build(m, B, args.image, args.bias, args.gamma) for m in MODES}
    ms = {m: [] for m in MODES}
    costs = {m: None for m in MODES}
    it = {m: 0 for m in MODES}
    states = {m: None for m in MODES}
    random.seed(5)
    first = random.getstate()

    def step(mode, record):
        # each model draws its RoI editing from a generator stream of its own, so the two see the same lists step for step
        random.setstate(states[mode] or first)
        model, dns = models[mode][:2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        costs[mode] = model.train_step(xd, metas, 0, it[mode], 0.0, [0.0], 0.0)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        dns.sample_bbox_list                             # (resolves the step's lazy host share before the state is taken)
        states[mode] = random.getstate()
        it[mode] += 1
        if record:
            ms[mode].append(dt)

    for _ in range(args.warmup):
        for m in MODES:
            step(m, False)
    for i in range(args.steps):
        for m in (MODES if i % 2 == 0 else MODES[::-1]):
            step(m, True)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "image": args.image, "steps_per_mode": args.steps,
           "corner_head_bias": args.bias, "gamma": args.gamma}
    for m in MODES:
        med = statistics.median(ms[m])
        total, layer_costs = costs[m]
        res[m] = {"median_ms_per_step": round(med, 2), "min_ms_per_step": round(min(ms[m]), 2), "max_ms_per_step": round(max(ms[m]), 2),
                  "images_per_s": round(1e3 * B / med, 1), "cost": float(total), "layer_costs": [float(c) for c in layer_costs],
                  "alone": kernels_alone(*models[m][2:])}
    res["focal_over_plain_time"] = round(res["focal"]["median_ms_per_step"] / res["plain"]["median_ms_per_step"], 4)
    for m in MODES:
        a = res[m]["alone"]
        print("%-6s %.2f ms / step (min %.2f, max %.2f); alone: corner cost %.1f us (%d cells), detect cost %.1f us (%d RoIs x %d "
              "classes); cost %.4f"
              % (m, res[m]["median_ms_per_step"], res[m]["min_ms_per_step"], res[m]["max_ms_per_step"], a["corner_cost"]["median_us"],
                 a["corner_cells"], a["detect_cost"]["median_us"], a["rois"], a["classes"], res[m]["cost"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
