"""The getting-started recipe (examples/simple-cifar10.sh) on the device, against float64.

- `same` convolutions with even filters on the direct kernels: forward (bias, batch-norm statistics epilogue), data and filter
  gradient. The float64 side is the reference's formulation (denet/layer/convolution.py:66-69,76-80): the full TRUE convolution,
  cropped at (k - 1) // 2 to H x W.
- csrc/regression.hip: cost, gradient and view-averaged probabilities (denet/layer/regression.py:23-47,97-98).
- One training step of zoo.simple_cifar10 restated in torch float64, test-mode probabilities, and the command line."""
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.model import zoo
from fp64_model import dropout_masks_of, param_layers, png_dataset as _png_dataset, reference, rel as _rel, relu_masks_of, sgd_step_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _true_conv_same(x, w):
    """reference formulation of `same`: full true convolution, cropped at (k - 1) // 2"""
    k = w.shape[2]
    y0 = (k - 1) // 2
    full = Fn.conv2d(x, w.flip(2, 3), padding=k - 1)
    return full[:, :, y0:y0 + x.shape[2], y0:y0 + x.shape[3]]


# ------------------------------------------------------------------------------------------------- even-filter `same` convolution
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("N,H,C,K", [(2, 38, 128, 96), (2, 19, 256, 192), (2, 9, 512, 384), (3, 13, 32, 32)])
def test_same_even_conv_vs_fp64(hip, k, N, H, C, K):
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + H * 10 + k + C)
    x = torch.randn(N, C, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, k, k, generator=g, dtype=torch.float64) / math.sqrt(C * k * k)
    bias = torch.randn(K, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y_ref = _true_conv_same(xr, wr)
    assert y_ref.shape == (N, K, H, H)
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)

    xn = x.permute(0, 2, 3, 1).float().contiguous().cuda()
    wn = w.flip(2, 3).permute(0, 2, 3, 1).float().contiguous().cuda()      # the device's correlation taps, KRSC
    dyn = dy.permute(0, 2, 3, 1).float().contiguous().cuda()
    bn = bias.float().cuda()
    geom = ops.conv_geom(tuple(xn.shape), tuple(wn.shape), 1, k // 2, None, (H, H))
    assert geom[10:] == (H, H) and not ops._full(geom)
    for mode in (0, 1, 2):
        assert ops._decided(mode, geom) == 0                 # no Winograd / fused path takes the cut geometry
    assert not ops.conv_wino2f_ok(0, geom) and not ops.conv_wino4t_ok(0, geom) and not ops.conv_wino_ok(geom, 2)

    cache = {"train": True}
    y = ops.conv_fwd(xn, wn, bias=bn, stride=1, pad=k // 2, cache=cache, ohw=(H, H))
    assert cache["fwd_tile"] == 0
    yr = (y_ref.detach() + bias[None, :, None, None]).permute(0, 2, 3, 1)
    assert y.shape == yr.shape and _rel(y, yr) <= 1e-5
    # the fused batch-norm statistics epilogue
    cache = {"train": True}
    y2 = ops.conv_fwd(xn, wn, bias=bn, stride=1, pad=k // 2, cache=cache, bn_stats=True, ohw=(H, H))
    assert torch.equal(y2, y)
    buf, rows = cache["bn_stats"]
    part = buf[:rows * 2 * K].view(rows, 2, K).sum(0).cpu()
    yd = yr.reshape(-1, K)
    assert float((part[0] - yd.sum(0)).abs().max() / yd.abs().sum(0).max()) <= 1e-5
    assert float((part[1] - (yd * yd).sum(0)).abs().max() / (yd * yd).sum(0).max()) <= 1e-5
    # data gradient (the transposed-filter and the plain implicit-GEMM kernels)
    for dgrad_t in (True, False):
        with ops.switches(DGRAD_T=dgrad_t):
            cache = {}
            dx = ops.conv_dgrad(dyn, wn, tuple(xn.shape), stride=1, pad=k // 2, cache=cache, ohw=(H, H))
        assert cache["dgrad_tile"] == 0
        assert _rel(dx, xr.grad.permute(0, 2, 3, 1)) <= 1e-5
    # filter gradient (the device's taps are flipped)
    dw = ops.conv_wgrad(xn, dyn, tuple(wn.shape), stride=1, pad=k // 2, ohw=(H, H))
    assert _rel(dw, wr.grad.flip(2, 3).permute(0, 2, 3, 1)) <= 1e-5


# ------------------------------------------------------------------------------------------------- regression kernels
def _logits(B, H, W, C, cp, seed):
    rng = np.random.RandomState(seed)
    z = rng.normal(0.0, 3.0, (B, H, W, cp)).astype(np.float32)
    z[..., C:] = 1e30                      # padding channels: must never be read
    return z


def _softmax64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("C", [6, 10, 1000])
@pytest.mark.parametrize("view", ["centre", "explicit"])
def test_regression_loss_vs_fp64(hip, C, view):
    B, H, W = 7, 4, 5
    cp = ((C + 31) // 32) * 32
    y, x = (H // 2, W // 2) if view == "centre" else (3, 1)
    z = _logits(B, H, W, C, cp, C + H)
    cls = np.random.RandomState(C).randint(0, C, B)
    pr = _softmax64(z[:, y, x, :C])
    cost_ref = -np.mean(np.log(pr[np.arange(B), cls]))
    g_ref = np.zeros((B, H, W, cp))
    g_ref[:, y, x, :C] = (pr - np.eye(C)[cls]) / B

    zd = torch.from_numpy(z).cuda()
    views = torch.tensor([y * W + x], dtype=torch.int32, device="cuda")
    cd = torch.from_numpy(cls.astype(np.int32)).cuda()

    def run():
        dl = torch.full((B, H, W, cp), float("nan"), device="cuda")
        costs = torch.full((2,), float("nan"), device="cuda")
        ops.regression_loss(zd, views, cd, dl, costs, C)
        return dl.cpu(), costs.cpu()

    dl, costs = run()
    assert abs(float(costs[0]) - cost_ref) <= 1e-5 * abs(cost_ref) and float(costs[1]) == 0.0
    off = torch.ones(B, H, W, cp, dtype=torch.bool)
    off[:, y, x, :C] = False
    assert torch.all(dl[off] == 0)                       # padding channels and every other pixel: exact zeros
    assert float((dl.double() - torch.from_numpy(g_ref)).abs().max()) <= 1e-6 / B
    dl2, costs2 = run()
    assert torch.equal(dl2.view(torch.int32), dl.view(torch.int32)) and torch.equal(costs2.view(torch.int32), costs.view(torch.int32))
    # without a gradient: the same cost bits
    costs3 = torch.full((2,), float("nan"), device="cuda")
    ops.regression_loss(zd, views, cd, None, costs3, C)
    assert torch.equal(costs3.cpu().view(torch.int32), costs.view(torch.int32))


@pytest.mark.parametrize("C", [6, 10, 1000])
@pytest.mark.parametrize("views", [[(2, 2)], [(0, 4), (3, 1)], [(0, 0), (1, 2), (3, 4), (2, 0), (1, 1)], "all"])
def test_regression_probabilities_vs_fp64(hip, C, views):
    B, H, W = 9, 4, 5
    cp = ((C + 31) // 32) * 32
    if views == "all":
        views = [(yy, xx) for yy in range(H) for xx in range(W)]
    z = _logits(B, H, W, C, cp, 3 * C + len(views))
    ref = np.mean([_softmax64(z[:, yy, xx, :C]) for yy, xx in views], axis=0)
    vd = torch.tensor([yy * W + xx for yy, xx in views], dtype=torch.int32, device="cuda")
    zd = torch.from_numpy(z).cuda()
    p = ops.regression_probs(zd, vd, C).cpu()
    assert p.shape == (B, C)
    assert float((p.double() - torch.from_numpy(ref)).abs().max()) <= 2e-6
    assert torch.equal(ops.regression_probs(zd, vd, C).cpu().view(torch.int32), p.view(torch.int32))


# ------------------------------------------------------------------------------------------------- one training step vs float64
def _policy(name):
    """`direct`: every convolution pass on the direct kernels (exact fp32 FMA chains); `default`: what a training run uses
    (static_policy: Winograd on the 3x3 layers that take it)"""
    return ops.algorithms(table={}, POLICY=ops.direct_policy) if name == "direct" else ops.algorithms()


@pytest.mark.parametrize("policy", ["direct", "default"])
def test_training_step_vs_fp64(hip, policy):
    """cost, every gradient, the SGD update, the running statistics and the test-mode probabilities against float64, 1e-3 (max
    norm), over twelve dropout seeds (ModelCNN.rng_seed, which selects the masks).

    The float64 restatement takes the device's ReLU decisions, as it takes its dropout masks. A batch-norm output within a few
    float32 ulps of zero (beta = 0, gamma = 1 at initialisation: xhat ~ 0) can fall on the other side of the ReLU in float32 than in
    float64. Such an element passes or stops one value of the gradient: the beta gradient of that batch norm (a sum over the pixels
    that largely cancels) and the filter gradient of the convolution in front move by 1e-3 - 1e-2, gamma's (weighted by xhat ~ 0)
    does not. The number of such elements is printed."""
    with _policy(policy):
        for seed in DROPOUT_SEEDS:
            _training_step_check(policy, seed)


DROPOUT_SEEDS = list(range(1, 13))


def _training_step_check(policy, seed):
    B, CLS, LR, MOM, DECAY = 4, 10, 0.1, 0.9, 0.0005
    model = zoo.simple_cifar10(B, CLS, seed=5)
    model.rng_seed = seed
    model.build_train_func("sgd")
    rng = np.random.RandomState(11)
    x = rng.uniform(0.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    metas = [{"image_class": int(c)} for c in cls]
    weights = set(id(p) for l in model.layers for p in l.weights())
    before = param_layers(model)
    values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}

    cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
    torch.cuda.synchronize()
    tiles = [(l.layer_index, l._cache().get("fwd_tile"), l._cache().get("dgrad_tile")) for l in model.layers if l.type_name == "conv"]
    print(policy, "seed", seed, "algorithms (layer, forward, data gradient):", tiles)
    if policy == "direct":
        assert all(t[1] == 0 and t[2] in (0, None) for t in tiles), tiles

    masks = dropout_masks_of(model)
    assert len(masks) == 3
    for m in masks.values():
        assert 0.6 < float((m != 0).double().mean()) < 0.95
    relu_masks = relu_masks_of(model)
    params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
    flips = {}
    cost_ref, _, stats = reference(model, x, params, cls, True, masks=masks, relu_masks=relu_masks, flips=flips)
    cost_ref.backward()
    print(policy, "seed", seed, "ReLU decisions that differ from float64 (layer: count):",
          {l.layer_index: flips[id(l)] for l in model.layers if flips.get(id(l))})
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach())), (cost, float(cost_ref.detach()))
    bound = 1e-3
    report, bad = [], []
    for l, p, e_g, e_p, _, _ in sgd_step_errors(before, values, params, weights, LR, DECAY):
        report.append("seed %d L%d %s: grad %.2e, update %.2e" % (seed, l.layer_index, p.name, e_g, e_p))
        if e_g > bound or e_p > bound:
            bad.append(report[-1])
    print("%s seed %d: worst gradient %.2e, worst update %.2e" % (
        policy, seed, max(float(r.split("grad ")[1].split(",")[0]) for r in report),
        max(float(r.split("update ")[1]) for r in report)))
    assert not bad, bad
    # running statistics: momentum over (mean = 0, stdinv = 1) (batch_norm.py:75-76)
    running = {}
    for l in model.layers:
        if l.type_name == "batchnorm":
            rm, rs = torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double()
            m_ref = (1.0 - l.momentum) * stats[id(l)]["mean"]
            s_ref = l.momentum + (1.0 - l.momentum) * stats[id(l)]["stdinv"]
            assert _rel(rm, m_ref) <= 1e-3 and _rel(rs, s_ref) <= 1e-3, l.layer_index
            running[id(l)] = (rm, rs)

    # test mode: the probabilities of the centre pixel with the updated parameters and statistics
    pr = model.predict_output_step(x)
    now = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in before}
    with torch.no_grad():
        _, logits, _ = reference(model, x, now, cls, False, running=running)
    pr_ref = torch.softmax(logits, dim=1)
    assert pr.shape == (B, CLS)
    assert float((torch.from_numpy(pr).double() - pr_ref).abs().max()) <= 1e-3 * float(pr_ref.max())


# ------------------------------------------------------------------------------------------------- command line
def test_recipe_cli_train_then_predict(hip, tmp_path):
    train_dir, test_dir, out = str(tmp_path / "train"), str(tmp_path / "test"), tmp_path / "out"
    _png_dataset(train_dir, seed=1)
    _png_dataset(test_dir, per_class=2, seed=2)
    out.mkdir()
    desc = zoo.SIMPLE_CIFAR10_DESC.split()
    cmd = [os.path.join(ROOT, "bin", "model-train"), "--seed", "0", "--distort-mode", "o4", "--solver", "sgd", "--border-mode",
           "same", "--augment-mirror", "--activation", "relu", "--epochs", "1", "--batch-size", "4", "--train", train_dir,
           "--test", test_dir, "--extension", "png", "--learn-rate", "0.1", "--learn-momentum", "0.9", "--learn-anneal", "0.5",
           "--learn-anneal-epochs", "15", "30", "--learn-decay", "0.0005", "--output-prefix", str(out / "model"),
           "--model-desc"] + desc
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    costs = [float(c) for c in re.findall(r"cost: (\S+) \(lr", log)]
    assert costs and all(math.isfinite(c) for c in costs), log[-3000:]
    assert os.path.exists(str(out / "model_epoch000.test"))
    final = glob.glob(str(out / "model_epoch000_final.mdl.gz"))
    assert final, os.listdir(str(out))
    r = subprocess.run([os.path.join(ROOT, "bin", "model-predict"), "--model", final[0], "--input", test_dir, "--extension", "png",
                        "--batch-size", "4", "--predict-mode", "single"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Top1 - Error Rate" in r.stdout + r.stderr
    # --skip-train: no step, but the epoch still tests and saves; the model written is the one read
    r = subprocess.run([os.path.join(ROOT, "bin", "model-train"), "--skip-train", "--model", final[0], "--epochs", "1", "--batch-size",
                        "4", "--train", train_dir, "--test", test_dir, "--extension", "png", "--border-mode", "same",
                        "--output-prefix", str(out / "skip")], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert not re.findall(r"cost: (\S+) \(lr", log), log[-3000:]
    assert os.path.exists(str(out / "skip_epoch000.test")) and os.path.exists(str(out / "skip_epoch000_final.mdl.gz"))
    from denet_amd.model import model_cnn
    a, b = model_cnn.load_from_file(final[0], 4), model_cnn.load_from_file(str(out / "skip_epoch000_final.mdl.gz"), 4)
    for la, lb in zip(a.layers, b.layers):
        for pa, pb in zip(la.all_params() if hasattr(la, "all_params") else [], lb.all_params() if hasattr(lb, "all_params") else []):
            np.testing.assert_array_equal(pa.get_value(), pb.get_value())
