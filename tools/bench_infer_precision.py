#!/usr/bin/env python
"""fp32 against the opt-in bf16 inference mode (ops.INFER_PRECISION, csrc/conv_bf16.hip), in ONE process.

  1. DeNet-34 skip 512x512 `get_detections` (the model of bench.py's inference leg) at batch 32 and batch 1: fp32 and bf16 calls in
     interleaved pairs (the order inside a pair alternates), host clock around a synchronised call; median and minimum per mode.
  2. every convolution geometry of that pass that bf16 mode moves to conv_bf16_kernel: the bf16 kernel alone beside what fp32
     inference runs there (Winograd transforms included), device events around one call, interleaved, median of the repeats.
  3. how many detections of the two modes coincide on the test views of the pipeline test's VOC tree (tests/golden/
     dataset_scenarios.py), DeNet-34 skip 128x128 with calibrated (not trained) heads.

The comparison is against fp32 mode in the same run; no ratio is promised. bench.py never turns the mode on.

    python tools/bench_infer_precision.py [--pairs 12] [--warmup 3] [--reps 20] [--batches 32,1] [--no-agreement]"""
import argparse
import collections
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy  # noqa: E402
import torch  # noqa: E402

from denet_amd import ops  # noqa: E402
from denet_amd.model import audit, zoo  # noqa: E402

MODES = ("fp32", "bf16")


def by_type(model, t):
    return [l for l in model.layers if l.type_name == t][0]


def bench_model(B):
    """the model and batch of bench.py's inference leg"""
    model = zoo.denet34(B, "skip", 512, class_num=80, seed=1)
    zoo.warm_corner_head(model, 4.0, 0.3)
    dnd = by_type(model, "denet-detect")
    dnd.layers[0].omega.set_value(numpy.random.RandomState(3).normal(0, 0.02, dnd.layers[0].omega.value.shape))
    x, metas = zoo.synthetic_batch(B, 512, 80, seed=1)
    return model, dnd, torch.from_numpy(x).cuda(), metas


def pass_times(B, pairs, warmup):
    model, dnd, xd, metas = bench_model(B)
    params = {"prThreshold": 0.05, "nmsThreshold": 0.5, "useSoftNMS": 0}
    last = {}
    for m in MODES:
        with ops.infer_precision(m):
            for _ in range(warmup):
                last[m] = dnd.get_detections(model, xd, metas, params)
    ms = {m: [] for m in MODES}
    for i in range(pairs):
        for m in (MODES if i % 2 == 0 else MODES[::-1]):
            with ops.infer_precision(m):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[m] = dnd.get_detections(model, xd, metas, params)
                torch.cuda.synchronize()
                ms[m].append(1e3 * (time.perf_counter() - t0))
    out = {"batch": B, "pairs": pairs}
    for m in MODES:
        med = statistics.median(ms[m])
        out[m] = {"median_ms": round(med, 3), "min_ms": round(min(ms[m]), 3), "max_ms": round(max(ms[m]), 3),
                  "images_per_s": round(1e3 * B / med, 1), "detections": sum(len(r["detections"]) for r in last[m])}
    out["bf16_over_fp32_time"] = round(out["bf16"]["median_ms"] / out["fp32"]["median_ms"], 3)
    return out, model


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_times(model, reps, warmup):
    """alone-times per geometry of the layers bf16 mode moves: [{geometry, layers, fp32 kernels + ms, bf16 kernel + ms}]"""
    geoms = collections.OrderedDict()
    for name, l in audit.conv_layers(model):
        if getattr(l, "direct", False) or getattr(l, "fp32_only", False) or l.cp % 32:
            continue
        g, txt = audit.layer_geometry(l)
        geoms.setdefault(g, [txt, 0])[1] += 1
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for g, (txt, count) in geoms.items():
        N, H, W, C, K, R, S, s_real, stride, pad, OH, OW = g
        x = torch.rand(N, H, W, C, generator=gen).cuda()
        w = (torch.randn(K, R, S, C, generator=gen) / (R * S * C) ** 0.5).cuda()
        b = torch.randn(K, generator=gen).cuda()
        y = ops.empty(N, OH, OW, K)
        w16 = ops.filter_to_bf16(w)
        cache = {"train": False}
        fns = {"fp32": lambda: ops.conv_fwd(x, w, bias=b, stride=stride, pad=pad, out=y, cache=cache, relu=True, ohw=(OH, OW)),
               "bf16": lambda: ops.conv_fwd_bf16(x, w16, bias=b, stride=stride, pad=pad, out=y, relu=True, ohw=(OH, OW))}
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
        flops = 2.0 * N * OH * OW * K * R * S * C
        row = {"geometry": "B%d %s" % (N, txt), "layers": count}
        for m in MODES:
            med = statistics.median(ms[m])
            row[m] = {"kernels": names[m], "median_ms": round(med, 4), "min_ms": round(min(ms[m]), 4),
                      "tflops": round(flops / med * 1e-9, 1)}
        row["bf16_over_fp32_time"] = round(row["bf16"]["median_ms"] / row["fp32"]["median_ms"], 3)
        rows.append(row)
        del x, w, y, w16
    total = {m: round(sum(r[m]["median_ms"] * r["layers"] for r in rows), 3) for m in MODES}
    return rows, total


def _iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def compare(d32, d16):
    """per-image detection lists [(score, class, box)] of the two modes. `exactly`: same class and the same box bit for bit;
    `iou_0.9`: same class and IoU >= 0.9 (greedy, in fp32 score order)"""
    exact = matched = 0
    dscore = 0.0
    for a, c in zip(d32, d16):
        exact += len({(cls, tuple(box)) for _, cls, box in a} & {(cls, tuple(box)) for _, cls, box in c})
        left = list(c)
        for pr, cls, box in a:
            best = max(((_iou(box, o[2]), k) for k, o in enumerate(left) if o[1] == cls), default=(0.0, -1))
            if best[0] >= 0.9:
                dscore = max(dscore, abs(pr - left[best[1]][0]))
                left.pop(best[1])
                matched += 1
    return {"images": len(d32), "detections_fp32": sum(len(d) for d in d32), "detections_bf16": sum(len(d) for d in d16),
            "same_class_same_box_exactly": exact, "same_class_iou_0.9": matched,
            "largest_score_difference_of_a_matched_pair": round(dscore, 5)}


def agreement():
    """detections of the two modes on the VOC test views of the pipeline test (128x128, batch 2). `exact`: same class and the
    same box bit for bit; `matched`: same class and IoU >= 0.9 (greedy, in score order)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import dataset_scenarios as S
    from denet_amd import dataset
    import random
    random.seed(5)
    numpy.random.seed(5)
    root = tempfile.mkdtemp(prefix="denet_bf16_")
    S.build_dataset(root)
    src = os.path.join(root, "voc")
    train = dataset.load(src, "voc,2007-trainval,2012-trainval,crop=128,crop_mode=denet,check_center", True, 1)
    test = dataset.load(src, "voc,2007-test,2012-test,crop=128,scale=128", False, 1, train.class_labels)
    B = 2
    model = zoo.denet34(B, "skip", 128, class_num=train.get_class_num(), seed=1)
    zoo.warm_corner_head(model, 4.0, 0.3)
    dnd = by_type(model, "denet-detect")
    dconv = dnd.layers[0]
    dconv.omega.set_value(numpy.random.RandomState(5).normal(0, 0.3, dconv.omega.value.shape))
    params = {"prThreshold": 0.08, "nmsThreshold": 0.5, "cornerThreshold": 0.02}
    batches = []
    for subset in range(test.subset_num):
        test.load_from_subset(subset)
        data_x, data_m, size = test.export(B)
        for n in range(data_x.shape[0] // B):
            batches.append((data_x[n * B:(n + 1) * B], data_m[n * B:(n + 1) * B], max(0, min(B, size - n * B))))
    # class logits of order one, box regressions of order 0.1, like a trained head (tests/test_inference_gpu.py)
    raw = []
    for x, m, _ in batches:
        dnd.get_detections(model, x, m, params)
        raw.append(dnd.conv.output.data.float().cpu().numpy().reshape(-1, dnd.conv.kp))
    raw = numpy.concatenate(raw)
    w = dconv.omega.get_value().copy()
    w[:dnd.s0] *= 2.0 / raw[:, :dnd.s0].std()
    w[dnd.s0:dnd.s0 + 4] *= 0.2 / raw[:, dnd.s0:dnd.s0 + 4].std()
    dconv.omega.set_value(w)
    dets = {m: [] for m in MODES}
    rois_equal = rois = 0
    for x, meta, n_real in batches:
        lists = {}
        for m in MODES:
            with ops.infer_precision(m):
                r = dnd.get_detections(model, x, meta, params)
            dets[m] += [d["detections"] for d in r[:n_real]]
            lists[m] = [[tuple(bx) for _, bx in l] for l in by_type(model, "denet-sparse").sample_bbox_list[:n_real]]
        for a, c in zip(lists["fp32"], lists["bf16"]):
            rois += len(a)
            rois_equal += len(set(a) & set(c))
    for data in (train, test):
        loader = getattr(data, "image_loader", None)
        if loader is not None:
            loader.close()
    out = compare(dets["fp32"], dets["bf16"])
    out.update({"rois_fp32": rois, "rois_also_proposed_in_bf16": rois_equal})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--no-agreement", action="store_true")
    args = ap.parse_args()
    assert ops.INFER_PRECISION == "fp32", "run without DENET_INFER_BF16: the tool switches the mode itself"
    out = {"device": torch.cuda.get_device_name(0), "passes": [], "kernels": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        res, model = pass_times(B, args.pairs, args.warmup)
        out["passes"].append(res)
        print("get_detections B=%d: fp32 %.3f ms (min %.3f) = %.1f img/s | bf16 %.3f ms (min %.3f) = %.1f img/s | bf16 / fp32 time %.3f"
              % (B, res["fp32"]["median_ms"], res["fp32"]["min_ms"], res["fp32"]["images_per_s"], res["bf16"]["median_ms"],
                 res["bf16"]["min_ms"], res["bf16"]["images_per_s"], res["bf16_over_fp32_time"]), flush=True)
        print("  detections of the timed batch (random heads, nothing to compare): fp32 %d, bf16 %d"
              % (res["fp32"]["detections"], res["bf16"]["detections"]), flush=True)
        rows, total = kernel_times(model, args.reps, args.warmup)
        out["kernels"]["b%d" % B] = {"rows": rows, "sum_over_layers_ms": total}
        print("%-34s %3s %10s %10s %7s  %s" % ("geometry", "n", "fp32 ms", "bf16 ms", "ratio", "fp32 kernels -> bf16 kernel"))
        for r in rows:
            print("%-34s %3d %10.4f %10.4f %7.3f  %s -> %s" % (r["geometry"], r["layers"], r["fp32"]["median_ms"], r["bf16"]["median_ms"],
                                                              r["bf16_over_fp32_time"], ", ".join(r["fp32"]["kernels"]),
                                                              ", ".join(r["bf16"]["kernels"])))
        print("sum over the layers: fp32 %.3f ms, bf16 %.3f ms" % (total["fp32"], total["bf16"]), flush=True)
        del model
        torch.cuda.empty_cache()
    if not args.no_agreement:
        out["agreement"] = agreement()
        print("agreement on the pipeline test's VOC views:", out["agreement"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
