#!/usr/bin/env python
"""A plain training step against a step that keeps an exponential moving average of the weights (`model-train --ema`,
csrc/ema.hip), in ONE process.

  1. DeNet-34 skip 512x512 training steps at batch 32 (the model and batch of bench.py): one plain model and one with ema_decay =
     0.999 (the average only observes: both train alike; their RoI draws come from one shared random stream, so their parameters
     are not compared bit for bit here - tests/test_ema_gpu.py does that on seeded twins), blocks of steps of the two interleaved
     (the order inside a pair alternates), host clock around a synchronised block; median, minimum and maximum ms per step, images/s.
  2. the two new launches alone (ema_update_kernel over P into E and over S into ES, nothing beside them): event pairs around
     blocks of calls, the bytes moved, 3 x 4 x (|P| + |S|) (two reads and one write per float), and the GB/s that amounts to:
     once on one pair of buffers over and over (partly served by the 256 MiB Infinity Cache), once rotating over four sets of
     copies (1 GB per cycle: from HBM, as inside a step).
  3. the exchange of ema_weights() alone (swap_kernel over both buffer pairs): 4 x 4 x (|P| + |S|) bytes.

The cost is one extra read of P and S and a read and a write of their shadows, behind the solver; the tool reports it against the
plain model of the same process and promises nothing. bench.py never turns the mode on.

    python tools/bench_ema.py [--pairs 6] [--steps 3] [--warmup 3] [--batch 32] [--image 512]"""
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

KINDS = ("plain", "ema")


def _alone(fn, calls, rounds=5):
    """median / min / max ms per call of fn() over `rounds` event pairs around `calls` calls"""
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--alone-calls", type=int, default=20)
    args = ap.parse_args()
    B, image = args.batch, args.image
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    lr, mom, decay = 0.1, [0.9], 1e-4
    models = {k: zoo.denet34(B, "skip", image, class_num=80, seed=1) for k in KINDS}
    models["ema"].ema_decay = args.decay
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
    m = models["ema"]
    floats = m.P.numel() + m.S.numel()
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "image": image, "pairs": args.pairs, "steps_per_block": args.steps,
           "ema_decay": args.decay, "ema_updates": m.ema_updates, "steps_taken": it["ema"], "floats_P": m.P.numel(),
           "floats_S": m.S.numel(), "average_is_finite": bool(torch.isfinite(m.E).all() and torch.isfinite(m.ES).all()),
           "plain_model_has_no_average": models["plain"].E is None}
    for k in KINDS:
        med = statistics.median(ms[k])
        out[k] = {"median_ms_per_step": round(med, 3), "min_ms_per_step": round(min(ms[k]), 3), "max_ms_per_step": round(max(ms[k]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "cost_after_each_block": costs[k]}
    out["ema_over_plain_time"] = round(out["ema"]["median_ms_per_step"] / out["plain"]["median_ms_per_step"], 4)
    # the two new launches alone, on scratch copies (the model's average is left as the steps made it)
    E, ES = m.E.clone(), m.ES.clone()
    om = 1.0 - args.decay

    def update():
        ops.ema_update(E, m.P, om)
        ops.ema_update(ES, m.S, om)

    def exchange():
        ops.swap(E, m.P)
        ops.swap(ES, m.S)

    med, lo, hi = _alone(update, args.alone_calls)
    moved = 3 * 4 * floats
    out["update_alone"] = {"bytes_moved": moved, "alone_ms": round(med, 4), "alone_ms_min": round(lo, 4), "alone_ms_max": round(hi, 4),
                           "gb_per_s": round(moved / (med * 1e-3) / 1e9, 1)}
    # the same pass over four rotating sets of copies: P and E together (263 MB at DeNet-34) nearly fit the 256 MiB Infinity Cache,
    # so repeated calls on one pair are served partly from it; four sets (1 GB per cycle) are not, which is what a step sees
    sets = [(E.clone(), m.P.clone(), ES.clone(), m.S.clone()) for _ in range(4)]
    turn = [0]

    def update_rotating():
        e, p, es, s = sets[turn[0] % len(sets)]
        turn[0] += 1
        ops.ema_update(e, p, om)
        ops.ema_update(es, s, om)

    cmed, clo, chi = _alone(update_rotating, args.alone_calls)
    out["update_alone_rotating"] = {"sets": len(sets), "bytes_moved": moved, "alone_ms": round(cmed, 4), "alone_ms_min": round(clo, 4),
                                    "alone_ms_max": round(chi, 4), "gb_per_s": round(moved / (cmed * 1e-3) / 1e9, 1)}
    del sets
    calls = args.alone_calls + args.alone_calls % 2          # an even count per block: P and S end where they began
    smed, slo, shi = _alone(exchange, calls)
    swapped = 4 * 4 * floats
    out["swap_alone"] = {"bytes_moved": swapped, "alone_ms": round(smed, 4), "alone_ms_min": round(slo, 4), "alone_ms_max": round(shi, 4),
                         "gb_per_s": round(swapped / (smed * 1e-3) / 1e9, 1)}
    print("train_step B=%d %dx%d: plain %.3f ms (min %.3f, max %.3f) = %.1f img/s | ema %.3f ms (min %.3f, max %.3f) = %.1f img/s | "
          "ema / plain time %.4f | %d updates in %d steps" % (
              B, image, image, out["plain"]["median_ms_per_step"], out["plain"]["min_ms_per_step"], out["plain"]["max_ms_per_step"],
              out["plain"]["images_per_s"], out["ema"]["median_ms_per_step"], out["ema"]["min_ms_per_step"],
              out["ema"]["max_ms_per_step"], out["ema"]["images_per_s"], out["ema_over_plain_time"], m.ema_updates, it["ema"]),
          flush=True)
    print("  update alone: %d + %d floats, %.1f MB moved in %.4f ms (min %.4f, max %.4f) = %.1f GB/s" % (
        m.P.numel(), m.S.numel(), moved / 1e6, med, lo, hi, out["update_alone"]["gb_per_s"]))
    print("  update alone over %d rotating sets of copies (outside the Infinity Cache): %.4f ms (min %.4f, max %.4f) = %.1f GB/s" % (
        out["update_alone_rotating"]["sets"], cmed, clo, chi, out["update_alone_rotating"]["gb_per_s"]))
    print("  exchange alone: %.1f MB moved in %.4f ms (min %.4f, max %.4f) = %.1f GB/s" % (
        swapped / 1e6, smed, slo, shi, out["swap_alone"]["gb_per_s"]))
    print("  costs after each timed block: plain %s | ema %s" % (costs["plain"], costs["ema"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
