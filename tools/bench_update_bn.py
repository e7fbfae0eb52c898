"""Wall time of update_bn (model-update-bn) on DeNet-34 skip: one untimed warm-up sweep of the first layer, then the whole
update over --batches synthetic batches, ended by a device synchronise. Prints one JSON line. Kernel times come from a run of
its own under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    import torch
    from denet_amd import ops
    from denet_amd.model import update_bn, zoo
    B = args.batch_size
    model = zoo.warm_corner_head(zoo.denet34(B, "skip", args.image, seed=1))
    batches = [torch.from_numpy(zoo.synthetic_batch(B, args.image, seed=s)[0]).cuda() for s in range(args.batches)]
    # warm-up: code objects, algorithm choices and workspaces of every shape of the sweeps (one batch, all layers)
    update_bn.update_bn(model, batches[:1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = update_bn.update_bn(model, batches)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the accumulate kernels alone at the stem batch norm's input (the largest: B x H/2 x W/2 rows x 64 channels)
    stem = update_bn.select_bn_layers(model)[0]
    shape = stem.input_shape
    x = torch.empty(shape[0] * shape[2] * shape[3], shape[1], device="cuda").uniform_()
    acc = torch.zeros(2, shape[1], dtype=torch.float64, device="cuda")
    ws = ops.bn_moments_workspace(x.shape[0], x.shape[1])
    for _ in range(3):
        ops.bn_moments_accumulate(x, acc, ws)
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.bn_moments_accumulate(x, acc, ws)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    print(json.dumps({"model": "denet34_skip", "batch_size": B, "image": args.image, "batches": args.batches, "layers": len(res),
                      "update_bn_s": round(wall, 3), "stem_rows": x.shape[0], "stem_channels": x.shape[1],
                      "accumulate_ms_back_to_back": round(ms, 4),
                      "accumulate_tb_s": round(x.numel() * 4 / (ms * 1e-3) / 1e12, 3)}))


if __name__ == "__main__":
    main()
