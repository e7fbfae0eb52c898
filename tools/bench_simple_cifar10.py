"""Training step of the getting-started recipe (zoo.simple_cifar10, examples/simple-cifar10.sh): --warmup untimed steps, then
--steps steps on random 32x32 batches, ended by a device synchronise. Prints one JSON line (ms per step, images per second).
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`."""
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
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import numpy
    import torch
    from denet_amd.model import zoo
    B = args.batch_size
    model = zoo.simple_cifar10(B, args.classes, seed=1)
    model.build_train_func("sgd")
    rng = numpy.random.RandomState(2)
    batches = []
    for _ in range(4):
        x = torch.from_numpy(rng.uniform(0.0, 1.0, (B, 3, 32, 32)).astype(numpy.float32)).cuda()
        batches.append((x, [{"image_class": int(c)} for c in rng.randint(0, args.classes, B)]))

    def step(it):
        x, metas = batches[it % len(batches)]
        return model.train_step(x, metas, 0, it, 0.1, [0.9], 0.0005, fetch_cost=False)

    for it in range(args.warmup):
        step(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.warmup, args.warmup + args.steps):
        step(it)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    cost, _ = model.train_step(*batches[0], 0, args.warmup + args.steps, 0.1, [0.9], 0.0005)
    print(json.dumps({"model": "simple_cifar10", "batch_size": B, "image": 32, "classes": args.classes, "steps": args.steps,
                      "ms_per_step": round(ms, 3), "images_per_s": round(B * 1e3 / ms, 1), "last_cost": round(float(cost), 4)}))


if __name__ == "__main__":
    main()
