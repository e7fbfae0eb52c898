#!/usr/bin/env python
"""Group normalisation (`BN.G`, normGroups, csrc/gn.hip) against the plain batch norm, in ONE process.

  passes  ops.gn_fwd / ops.gn_bwd against the plain layer's SEPARATE passes on the same tensors - ops.bn_fwd_train without `pre`
          and ops.bn_bwd, three launches each like the group norm's - at DeNet-34's four stage geometries (512 x 512 input: 128^2 x
          64, 64^2 x 128, 32^2 x 256, 16^2 x 512) at batch 32 and batch 2, G = 32, ReLU on. The compulsory traffic is the same
          (forward: x twice + y; backward: x and dy twice + dx), so the yardstick is the batch-norm pass itself. Blocks of the two
          interleaved (the order inside a pair alternates), event pairs around a block; median, minimum and maximum us per call,
          the ratio of the medians, whether the group norm's median lies inside the batch norm's own range, and the fraction of
          the copy rate on record (6.29 TB/s) the compulsory bytes reach.
  step    zoo.denet34(B, "skip", 512) plain against norm_groups = 32 (same weights), blocks of training steps interleaved, host
          clock around a synchronised block; median, minimum and maximum ms per step. A group-mode layer gives up the linked,
          pool-fused, producer-finished and inference-folded forms of the batch norm, so the model is expected to be slower; the
          tool reports by how much and promises nothing. bench.py never builds such a model.

    python tools/bench_group_norm.py passes [--rounds 9] [--reps 20]
    python tools/bench_group_norm.py step [--batch 32] [--image 512] [--pairs 5] [--steps 4] [--warmup 3]"""
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
from denet_amd.layer.batch_norm import group_norm_layers  # noqa: E402
from denet_amd.model import zoo  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, the device-to-device copy rate on record
STAGES = [(128, 64), (64, 128), (32, 256), (16, 512)]      # (map side, channels) of DeNet-34's four stages at 512 x 512
G = 32


def _stat(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def passes(args):
    out = {"device": torch.cuda.get_device_name(0), "groups": G, "rounds": args.rounds, "reps": args.reps, "cases": []}
    for B in (32, 2):
        for side, C in STAGES:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(B, side, side, C, device="cuda", generator=g)
            dy = torch.randn(B, side, side, C, device="cuda", generator=g)
            gamma = torch.rand(C, device="cuda", generator=g) + 0.5
            beta = torch.randn(C, device="cuda", generator=g)
            y, dx = torch.empty_like(x), torch.empty_like(x)
            rm, rs = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            _, bm, bi = ops.bn_fwd_train(x, gamma, beta, rm, rs, 0.9, 1e-5, relu=True, out=y)
            _, gm, gi = ops.gn_fwd(x, gamma, beta, G, 1e-5, relu=True, out=y)
            calls = {
                "bn_fwd": lambda: ops.bn_fwd_train(x, gamma, beta, rm, rs, 0.9, 1e-5, relu=True, out=y),
                "gn_fwd": lambda: ops.gn_fwd(x, gamma, beta, G, 1e-5, relu=True, out=y),
                "bn_bwd": lambda: ops.bn_bwd(x, None, dy, gamma, bm, bi, relu=True, dgamma=dg, dbeta=db, dx=dx, beta=beta),
                "gn_bwd": lambda: ops.gn_bwd(x, None, dy, gamma, gm, gi, G, relu=True, dgamma=dg, dbeta=db, dx=dx, beta=beta),
            }
            us = {k: [] for k in calls}
            for f in calls.values():
                f()
            torch.cuda.synchronize()
            for r in range(args.rounds):
                for pair in (("bn_fwd", "gn_fwd"), ("bn_bwd", "gn_bwd")):
                    for k in (pair if r % 2 == 0 else pair[::-1]):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.reps):
                            calls[k]()
                        e1.record()
                        e1.synchronize()
                        us[k].append(1e3 * e0.elapsed_time(e1) / args.reps)
            nbytes = x.numel() * 4
            case = {"batch": B, "map": side, "channels": C, "tensor_MB": round(nbytes / 1e6, 2)}
            for k in calls:
                case[k] = _stat(us[k])
            for d, mult in (("fwd", 3), ("bwd", 5)):
                b, gq = case["bn_" + d], case["gn_" + d]
                case[d + "_gn_over_bn"] = round(gq["median_us"] / b["median_us"], 3)
                case[d + "_gn_inside_bn_range"] = b["min_us"] <= gq["median_us"] <= b["max_us"]
                for k in ("bn_", "gn_"):
                    case[k + d + "_of_copy_rate"] = round(mult * nbytes / (case[k + d]["median_us"] * 1e-6) / COPY_RATE, 3)
            out["cases"].append(case)
            print("B=%2d %3dx%-3d C=%3d (%6.2f MB): fwd bn %7.2f us [%7.2f, %7.2f] gn %7.2f us [%7.2f, %7.2f] ratio %.3f %s, of copy "
                  "rate bn %.2f gn %.2f | bwd bn %7.2f us [%7.2f, %7.2f] gn %7.2f us [%7.2f, %7.2f] ratio %.3f %s, of copy rate bn %.2f "
                  "gn %.2f" % (B, side, side, C, nbytes / 1e6,
                               case["bn_fwd"]["median_us"], case["bn_fwd"]["min_us"], case["bn_fwd"]["max_us"],
                               case["gn_fwd"]["median_us"], case["gn_fwd"]["min_us"], case["gn_fwd"]["max_us"], case["fwd_gn_over_bn"],
                               "inside" if case["fwd_gn_inside_bn_range"] else "OUTSIDE", case["bn_fwd_of_copy_rate"],
                               case["gn_fwd_of_copy_rate"],
                               case["bn_bwd"]["median_us"], case["bn_bwd"]["min_us"], case["bn_bwd"]["max_us"],
                               case["gn_bwd"]["median_us"], case["gn_bwd"]["min_us"], case["gn_bwd"]["max_us"], case["bwd_gn_over_bn"],
                               "inside" if case["bwd_gn_inside_bn_range"] else "OUTSIDE", case["bn_bwd_of_copy_rate"],
                               case["gn_bwd_of_copy_rate"]), flush=True)
    print(json.dumps(out))


def step(args):
    B, image = args.batch, args.image
    kinds = ("plain", "group")
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    lr, mom, decay = 0.1, [0.9], 1e-4
    models = {"plain": zoo.denet34(B, "skip", image, class_num=80, seed=1),
              "group": zoo.denet34(B, "skip", image, class_num=80, seed=1, norm_groups=G)}
    n_group = len(group_norm_layers(models["group"]))
    assert n_group > 0 and not group_norm_layers(models["plain"])
    it = {k: 0 for k in kinds}

    def run(k, n):
        for _ in range(n):
            cost, _ = models[k].train_step(xd, metas, 0, it[k], lr, mom, decay)
            it[k] += 1
        return cost

    for k in kinds:
        models[k].build_train_func("nesterov")
        run(k, max(args.warmup, 2))
    torch.cuda.synchronize()
    ms, costs = {k: [] for k in kinds}, {k: [] for k in kinds}
    for i in range(args.pairs):
        for k in (kinds if i % 2 == 0 else kinds[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cost = run(k, args.steps)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            costs[k].append(round(float(cost), 4))
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "image": image, "pairs": args.pairs, "steps_per_block": args.steps,
           "group_mode_layers": n_group, "groups": G}
    for k in kinds:
        med = statistics.median(ms[k])
        out[k] = {"median_ms_per_step": round(med, 3), "min_ms_per_step": round(min(ms[k]), 3), "max_ms_per_step": round(max(ms[k]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "cost_after_each_block": costs[k]}
    out["group_over_plain_time"] = round(out["group"]["median_ms_per_step"] / out["plain"]["median_ms_per_step"], 3)
    print("train_step B=%d %dx%d, %d group-mode layers (G = %d): plain %.3f ms (min %.3f, max %.3f) = %.1f img/s | group %.3f ms (min "
          "%.3f, max %.3f) = %.1f img/s | group / plain time %.3f" % (
              B, image, image, n_group, G, out["plain"]["median_ms_per_step"], out["plain"]["min_ms_per_step"],
              out["plain"]["max_ms_per_step"], out["plain"]["images_per_s"], out["group"]["median_ms_per_step"],
              out["group"]["min_ms_per_step"], out["group"]["max_ms_per_step"], out["group"]["images_per_s"],
              out["group_over_plain_time"]), flush=True)
    print("  costs after each timed block: plain %s | group %s" % (costs["plain"], costs["group"]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    p = sub.add_parser("passes")
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=20)
    s = sub.add_parser("step")
    s.add_argument("--batch", type=int, default=32)
    s.add_argument("--image", type=int, default=512)
    s.add_argument("--pairs", type=int, default=5)
    s.add_argument("--steps", type=int, default=4)
    s.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    {"passes": passes, "step": step}[args.what](args)


if __name__ == "__main__":
    main()
