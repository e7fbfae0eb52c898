#!/usr/bin/env python
"""fp32 against the opt-in bf16 training mode (ops.TRAIN_PRECISION, csrc/conv_bf16.hip + csrc/conv_bf16_train.hip), in ONE process.

  1. DeNet-34 skip 512x512 training steps at batch 32 (the model and batch of bench.py): one model per mode (a layer's caches and
     prepared filters belong to one mode), blocks of steps of the two modes interleaved (the order inside a pair alternates), host
     clock around a synchronised block; median and minimum ms per step, images/s.
  2. one audited step per mode: which kernels every convolution layer launched (model/audit.py).
  3. every convolution geometry bf16 mode moves: each of the three passes alone in both modes (ops.conv_fwd / conv_dgrad /
     conv_wgrad as ConvLayer calls them, device events around one call, interleaved, median of the repeats; the kernels by the
     launch trace). An fp32 Winograd pass transforms its filter inside the timed call here (the step prepares those on a side
     stream); the bf16 filter copies are made once per weights version and are not in the bf16 figure. Neither figure holds the
     batch-norm statistics passes that bf16 mode adds to the step (fp32 mode fuses them into the convolution epilogues).

The comparison is against fp32 mode in the same run; no ratio is promised. bench.py never turns the mode on.

    python tools/bench_train_precision.py [--pairs 6] [--steps 3] [--warmup 3] [--reps 10] [--batch 32] [--image 512]"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from denet_amd import ops  # noqa: E402
from denet_amd.model import audit, zoo  # noqa: E402

MODES = ("fp32", "bf16")
PASSES = ("fwd", "dgrad", "wgrad")


def step_times(B, image, pairs, steps, warmup):
    models, it = {}, {m: 0 for m in MODES}
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    lr, mom, decay = 0.1, [0.9], 1e-4

    def run(m, n):
        with ops.train_precision(m):
            for _ in range(n):
                cost, _ = models[m].train_step(xd, metas, 0, it[m], lr, mom, decay)
                it[m] += 1
        return cost

    costs = {m: [] for m in MODES}
    for m in MODES:
        models[m] = zoo.denet34(B, "skip", image, class_num=80, seed=1)
        with ops.train_precision(m):
            models[m].build_train_func("nesterov")
        run(m, max(warmup, 2))
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    for i in range(pairs):
        for m in (MODES if i % 2 == 0 else MODES[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cost = run(m, steps)
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / steps)
            costs[m].append(round(float(cost), 4))
    out = {"batch": B, "image": image, "pairs": pairs, "steps_per_block": steps}
    for m in MODES:
        med = statistics.median(ms[m])
        out[m] = {"median_ms_per_step": round(med, 3), "min_ms_per_step": round(min(ms[m]), 3), "max_ms_per_step": round(max(ms[m]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "cost_after_each_block": costs[m]}
    out["bf16_over_fp32_time"] = round(out["bf16"]["median_ms_per_step"] / out["fp32"]["median_ms_per_step"], 3)
    tables = {}
    for m in MODES:
        with ops.train_precision(m), audit.KernelAudit(models[m]) as ka:
            models[m].train_step(xd, metas, 0, it[m], lr, mom, decay)
        torch.cuda.synchronize()
        tables[m] = ka.summary()
    return out, models, tables


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pass_times(model, reps, warmup):
    """alone-times per geometry of the layers bf16 mode moves: [{geometry, layers, pass: {mode: {kernels, median_ms}}}]"""
    geoms = collections.OrderedDict()
    for name, l in audit.conv_layers(model):
        if not l._bf16_train_eligible():
            continue
        g, txt = audit.layer_geometry(l)
        ent = geoms.setdefault(g, [txt, 0, False])
        ent[1] += 1
        ent[2] = ent[2] or bool(getattr(l.input, "requires_grad", True))
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for g, (txt, count, need_dx) in geoms.items():
        N, H, W, C, K, R, S, s_real, stride, pad, OH, OW = g
        x = torch.rand(N, H, W, C, generator=gen).cuda()
        w = (torch.randn(K, R, S, C, generator=gen) / (R * S * C) ** 0.5).cuda()
        dy = (torch.randn(N, OH, OW, K, generator=gen) * 1e-3).cuda()
        y, dx, dw = ops.empty(N, OH, OW, K), ops.empty(N, H, W, C), ops.empty(K, R, S, C)
        caches = {"fp32": {"train": True}, "bf16": {"train": True, "bf16_train": True}}
        row = {"geometry": "B%d %s" % (N, txt), "layers": count}
        for p in PASSES:
            if p == "dgrad" and not need_dx:
                continue
            fns = {}
            for m in MODES:
                c = caches[m]
                if p == "fwd":
                    fns[m] = lambda c=c: ops.conv_fwd(x, w, stride=stride, pad=pad, out=y, cache=c)
                elif p == "dgrad":
                    fns[m] = lambda c=c: ops.conv_dgrad(dy, w, tuple(x.shape), stride=stride, pad=pad, out=dx, cache=c)
                else:
                    fns[m] = lambda c=c: ops.conv_wgrad(x, dy, tuple(w.shape), stride=stride, pad=pad, out=dw, cache=c)
            names = {}
            for m in MODES:
                for _ in range(warmup):
                    fns[m]()
                with ops.LaunchTrace() as tr:
                    fns[m]()
                names[m] = tr.symbols
            ms = {m: [] for m in MODES}
            for i in range(reps):
                for m in (MODES if i % 2 == 0 else MODES[::-1]):
                    ms[m].append(event_ms(fns[m]))
            row[p] = {m: {"kernels": names[m], "median_ms": round(statistics.median(ms[m]), 4), "min_ms": round(min(ms[m]), 4)}
                      for m in MODES}
            row[p]["bf16_over_fp32_time"] = round(row[p]["bf16"]["median_ms"] / row[p]["fp32"]["median_ms"], 3)
        rows.append(row)
        del x, w, dy, y, dx, dw
    total = {p: {m: round(sum(r[p][m]["median_ms"] * r["layers"] for r in rows if p in r), 3) for m in MODES} for p in PASSES}
    return rows, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image", type=int, default=512)
    args = ap.parse_args()
    assert ops.TRAIN_PRECISION == "fp32", "run without DENET_TRAIN_BF16: the tool switches the mode itself"
    out = {"device": torch.cuda.get_device_name(0)}
    res, models, tables = step_times(args.batch, args.image, args.pairs, args.steps, args.warmup)
    out["steps"] = res
    print("train_step B=%d %dx%d: fp32 %.3f ms (min %.3f) = %.1f img/s | bf16 %.3f ms (min %.3f) = %.1f img/s | bf16 / fp32 time %.3f"
          % (args.batch, args.image, args.image, res["fp32"]["median_ms_per_step"], res["fp32"]["min_ms_per_step"],
             res["fp32"]["images_per_s"], res["bf16"]["median_ms_per_step"], res["bf16"]["min_ms_per_step"], res["bf16"]["images_per_s"],
             res["bf16_over_fp32_time"]), flush=True)
    print("  costs after each timed block: fp32 %s | bf16 %s" % (res["fp32"]["cost_after_each_block"], res["bf16"]["cost_after_each_block"]))
    out["kernels_per_geometry"] = tables
    for geom in tables["fp32"]:
        a, b = tables["fp32"][geom], tables["bf16"].get(geom, {"fwd": [], "bwd": []})
        if a["fwd"] != b["fwd"] or a["bwd"] != b["bwd"]:
            print("  %-28s x%-2d fwd %s -> %s\n%35s bwd %s -> %s" % (geom, a["layers"], ", ".join(a["fwd"]), ", ".join(b["fwd"]), "",
                                                                  ", ".join(a["bwd"]), ", ".join(b["bwd"])), flush=True)
    model = models["fp32"]
    del models
    rows, total = pass_times(model, args.reps, args.warmup)
    out["passes"] = {"rows": rows, "sum_over_layers_ms": total}
    print("%-34s %3s  %s" % ("geometry", "n", "  ".join("%-26s" % (p + " fp32 / bf16 ms (ratio)") for p in PASSES)))
    for r in rows:
        cells = []
        for p in PASSES:
            cells.append("%-26s" % ("%.4f / %.4f (%.2f)" % (r[p]["fp32"]["median_ms"], r[p]["bf16"]["median_ms"], r[p]["bf16_over_fp32_time"])
                                    if p in r else "-"))
        print("%-34s %3d  %s" % (r["geometry"], r["layers"], "  ".join(cells)))
    for r in rows:
        for p in PASSES:
            if p in r:
                print("    %s %s: %s -> %s" % (r["geometry"], p, ", ".join(r[p]["fp32"]["kernels"]), ", ".join(r[p]["bf16"]["kernels"])))
    print("sum over the layers: " + "; ".join("%s fp32 %.3f ms, bf16 %.3f ms" % (p, total[p]["fp32"], total[p]["bf16"]) for p in PASSES),
          flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
