#!/usr/bin/env python
"""Nearest (tapRule 0) against bilinear (tapRule 2, `DNS.I`; csrc/sparse_bilinear.hip) RoI sampling, in ONE process.

DeNet-34 skip 512x512, two models from the same seed that differ in the DNS layer's rule alone, a warmed corner head
(zoo.warm_corner_head), training steps of the two models interleaved (the order inside a pair alternates), host clock around every
synchronised step, median over the steps of a model. Learning rate 0: every step sees the same detector. Reported per rule: ms per
step, and the gather, the grouping (sort) and the gather gradient measured ALONE (device events around the ops call on the last
step's own map and RoI list, median of 20 after 3 unmeasured calls), with the slot statistics of the gradient's lists (the longest
list decides the gradient's time: one wave per cell). No ratio is promised, the mode stays opt-in. bench.py never turns it on.

    python tools/bench_sparse_bilinear.py [--batch 32] [--steps 20] [--warmup 3] [--image 512] [--bias 7.5]"""
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

RULES = ("nearest", "bilinear")


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


def build(rule, B, image, bias):
    tag = "DNS.I" if rule == "bilinear" else "DNS"
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "%s[7,24,0.01,0.1]" % tag)
    model = zoo.denet34(B, "skip", image, class_num=80, seed=1, head_desc=desc)
    zoo.warm_corner_head(model, bias, 0.3)
    model.build_train_func("nesterov")
    return model, [l for l in model.layers if l.type_name == "denet-sparse"][0]


def kernels_alone(rule, dns):
    """the three launches of the rule on the last step's map and RoI list, each alone on the compute stream"""
    dnc = dns.corner_layer
    fmap, coff, F = dnc.sample_map()
    B, H, W, CP = fmap.shape
    S, gs, kp = dns.sample_count, dns.grid_size, dns.output.cp
    L = ops._L()
    dy = torch.rand(B * S, kp, device="cuda") - 0.5
    dfmap = torch.zeros_like(fmap)
    ev = torch.cuda.Event()
    ev.record()
    out = {}
    if rule == "bilinear":
        _, taps4, wts4 = ops.sparse_bilinear_fwd(fmap, dns.sample_bbox, coff, F, S, gs, kp)
        ws = ops._sparse_bilinear_ws(B, H, W, S, gs)
        out["gather"] = alone(lambda: ops.sparse_bilinear_fwd(fmap, dns.sample_bbox, coff, F, S, gs, kp))
        out["sort"] = alone(lambda: ops.check(L.denet_sparse_bilinear_sort(ops.ptr(taps4), ops.ptr(ws), ws.numel(), B, H, W, S, gs,
                                                                            ops.stream_ptr()), "sparse_bilinear_sort"))
        out["gather_gradient"] = alone(lambda: ops.sparse_bilinear_bwd(dy, taps4, wts4, dfmap, coff, F, S, gs, coff + F, presorted=ev))
        cells, single = taps4.view(B, -1), L.denet_sparse_sort_is_single(B, H, W, S * 4, gs)
    else:
        _, taps = ops.sparse_fwd(fmap, dns.sample_bbox, coff, F, S, gs, kp, dns.tap_rule)
        ws = ops.WS.get("sparse_sort", L.denet_sparse_sort_workspace_bytes(B, H, W, S, gs))
        out["gather"] = alone(lambda: ops.sparse_fwd(fmap, dns.sample_bbox, coff, F, S, gs, kp, dns.tap_rule))
        out["sort"] = alone(lambda: ops.check(L.denet_sparse_sort(ops.ptr(taps), ops.ptr(ws), ws.numel(), B, H, W, S, gs,
                                                                   ops.stream_ptr()), "sparse_sort"))
        out["gather_gradient"] = alone(lambda: ops.sparse_bwd(dy, taps, dfmap, coff, F, S, gs, coff + F, presorted=ev))
        cells, single = taps.view(B, -1), L.denet_sparse_sort_is_single(B, H, W, S, gs)
    counts = torch.stack([torch.bincount(c.long(), minlength=H * W) for c in cells]).cpu().numpy()
    out["slots_per_image"] = int(cells.shape[1])
    out["sort_kernels"] = 1 if single else 3
    out["slots_per_cell"] = {"median": float(statistics.median(counts.reshape(-1).tolist())), "max": int(counts.max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--bias", type=float, default=7.5, help="corner head bias of zoo.warm_corner_head")
    args = ap.parse_args()
    B = args.batch
    x, metas = zoo.synthetic_batch(B, args.image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    models = {r: build(r, B, args.image, args.bias) for r in RULES}
    ms = {r: [] for r in RULES}
    it = {r: 0 for r in RULES}
    states = {r: None for r in RULES}
    random.seed(5)
    first = random.getstate()

    def step(rule, record):
        # each model draws its RoI editing from a generator stream of its own, so the two see the same lists step for step
        random.setstate(states[rule] or first)
        model, _ = models[rule]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.train_step(xd, metas, 0, it[rule], 0.0, [0.0], 0.0)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        models[rule][1].sample_bbox_list                 # (resolves the step's lazy host share before the state is taken)
        states[rule] = random.getstate()
        it[rule] += 1
        if record:
            ms[rule].append(dt)

    for _ in range(args.warmup):
        for r in RULES:
            step(r, False)
    for i in range(args.steps):
        for r in (RULES if i % 2 == 0 else RULES[::-1]):
            step(r, True)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "image": args.image, "steps_per_rule": args.steps,
           "corner_head_bias": args.bias}
    for r in RULES:
        med = statistics.median(ms[r])
        res[r] = {"median_ms_per_step": round(med, 2), "min_ms_per_step": round(min(ms[r]), 2), "max_ms_per_step": round(max(ms[r]), 2),
                  "images_per_s": round(1e3 * B / med, 1), "alone": kernels_alone(r, models[r][1])}
    res["bilinear_over_nearest_time"] = round(res["bilinear"]["median_ms_per_step"] / res["nearest"]["median_ms_per_step"], 4)
    for r in RULES:
        a = res[r]["alone"]
        print("%-8s %.2f ms / step (min %.2f, max %.2f); alone: gather %.1f us, sort %.1f us (%d kernel%s, %d slots per image), gather "
              "gradient %.1f us (slots per cell: median %.0f, max %d)"
              % (r, res[r]["median_ms_per_step"], res[r]["min_ms_per_step"], res[r]["max_ms_per_step"], a["gather"]["median_us"],
                 a["sort"]["median_us"], a["sort_kernels"], "s" * (a["sort_kernels"] > 1), a["slots_per_image"],
                 a["gather_gradient"]["median_us"], a["slots_per_cell"]["median"], a["slots_per_cell"]["max"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
