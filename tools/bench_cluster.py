#!/usr/bin/env python
"""Host against device RoI clustering (ops.CLUSTER_DEVICE, csrc/cluster.hip) of a clustering DNS layer, in ONE process.

DeNet-34 skip 512x512 with `DNS[7,sn,0.01,0.1,0,0.7]`, a warmed corner head (the warmest at which every image proposes more than
sn^2 candidates, found by lowering the bias from --bias), one
model per sn; training steps of the two modes interleaved on the same model (the order inside a pair alternates), host clock around
every synchronised step, median over the steps of a mode. Reported per mode: step time, the hand-off's phase_ms entries (medians),
handoff_modes, candidates per image; for the device mode also the summed duration of the four cluster_* launches, measured alone
(device events around ops.cluster_samples_device on the last step's staged proposal). The baseline is the host form of the same
model in the same process; no ratio is promised, the mode stays opt-in. bench.py never turns the mode on.

    python tools/bench_cluster.py [--sn 24 48] [--batch 32 16] [--steps 20] [--warmup 2] [--image 512] [--bias 7.5]"""
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

MODES = ("host", "device")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(sn, B, image, steps, warmup, bias):
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "DNS[7,%d,0.01,0.1,0,0.7]" % sn)
    model = zoo.denet34(B, "skip", image, class_num=80, seed=1, head_desc=desc)
    dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
    dnc = dns.corner_layer
    assert dns.cluster and dns.proposal_count == 10 * sn * sn
    x, metas = zoo.synthetic_batch(B, image, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    model.build_train_func("nesterov")
    random.seed(5)
    P, S = dns.proposal_count, dns.sample_count
    # the warmest head (highest bias, quarter steps down from --bias) at which EVERY image proposes more than sn^2 candidates
    while True:
        zoo.warm_corner_head(model, bias, 0.3)
        with ops.cluster_device(True):
            model.train_step(xd, metas, 0, 0, 0.0, [0.0], 0.0)
        if int(dns._stage_dev[B * P * 5:].min()) > S:
            break
        bias -= 0.25
        assert bias > 0, "no corner head bias makes every image propose more than %d candidates" % S
    it = [0]
    ms = {m: [] for m in MODES}
    phases = {m: {} for m in MODES}

    def step(mode, record):
        before = dict(dns.handoff_modes)
        with ops.cluster_device(mode == "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.train_step(xd, metas, 0, it[0], 0.0, [0.0], 0.0)          # learning rate 0: every step sees the same detector
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
        it[0] += 1
        if record:
            ms[mode].append(dt)
            for k, v in dns.phase_ms.items():
                phases[mode].setdefault(k, []).append(v)
            for k in dns.handoff_modes:
                forms[mode][k] += dns.handoff_modes[k] - before[k]

    forms = {m: {k: 0 for k in dns.handoff_modes} for m in MODES}
    for _ in range(warmup):
        for m in MODES:
            step(m, False)
    for i in range(steps):
        for m in (MODES if i % 2 == 0 else MODES[::-1]):
            step(m, True)
    # the proposal of the last device-mode step lies in the staging buffer: candidates per image, the cluster_* launches alone
    with ops.cluster_device(True):
        step("device", False)
    st = dns._stage_dev
    staged = (st[:B * P * 4].view(B, P, 4), st[B * P * 4:B * P * 5].view(torch.float32).view(B, P), st[B * P * 5:])
    counts = staged[2].cpu().numpy()
    call = lambda: ops.cluster_samples_device(*staged, float(dns.nms_threshold), S, dnc.height, dnc.width)
    for _ in range(3):
        call()
    alone = [event_ms(call) for _ in range(20)]
    out = {"sn": sn, "batch": B, "image": image, "steps_per_mode": steps, "corner_head_bias": bias, "candidates_per_image": {"min": int(counts.min()), "mean": float(counts.mean()), "max": int(counts.max())},
           "rois_per_image": S, "cluster_launches_alone_ms": {"median": round(statistics.median(alone), 3), "min": round(min(alone), 3)}}
    for m in MODES:
        med = statistics.median(ms[m])
        out[m] = {"median_ms_per_step": round(med, 2), "min_ms_per_step": round(min(ms[m]), 2), "max_ms_per_step": round(max(ms[m]), 2),
                  "images_per_s": round(1e3 * B / med, 1), "handoff_modes": forms[m],
                  "phase_ms_median": {k: round(statistics.median(v), 3) for k, v in sorted(phases[m].items())}}
    out["device_over_host_time"] = round(out["device"]["median_ms_per_step"] / out["host"]["median_ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sn", type=int, nargs="+", default=[24, 48])
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 16], help="one per --sn (the last one repeats)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--bias", type=float, default=7.5, help="corner head bias of zoo.warm_corner_head to start from; lowered in quarter steps until every image proposes more than sn^2 candidates")
    args = ap.parse_args()
    assert not ops.CLUSTER_DEVICE, "run without DENET_CLUSTER_DEVICE: the tool switches the mode itself"
    res = {"device": torch.cuda.get_device_name(0), "runs": []}
    for i, sn in enumerate(args.sn):
        B = args.batch[min(i, len(args.batch) - 1)]
        r = run(sn, B, args.image, args.steps, args.warmup, args.bias)
        res["runs"].append(r)
        print("sn = %d, B = %d, corner head bias %.2f, %.0f candidates per image (min %d, max %d): host %.2f ms / step (%s), device %.2f ms / step (%s), device / host time %.3f; "
              "cluster_* launches alone %.3f ms" % (sn, B, r["corner_head_bias"], r["candidates_per_image"]["mean"], r["candidates_per_image"]["min"],
                                                   r["candidates_per_image"]["max"], r["host"]["median_ms_per_step"],
                                                   r["host"]["handoff_modes"], r["device"]["median_ms_per_step"],
                                                   r["device"]["handoff_modes"], r["device_over_host_time"],
                                                   r["cluster_launches_alone_ms"]["median"]), flush=True)
        for m in MODES:
            print("    %-6s phase_ms (median): %s" % (m, r[m]["phase_ms_median"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
