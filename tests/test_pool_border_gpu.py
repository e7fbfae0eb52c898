"""Border-keeping pooling (`P.B` / `P.AB`, csrc/pool_border.hip) on the device, against float64.

The arbiter is the numpy restatement below of the rules of pool_2d(..., ignore_border=False) without padding:
window (oy, ox) covers rows oy*sh .. min(oy*sh + kh, H) - 1 and columns ox*sw .. min(ox*sw + kw, W) - 1; max is the maximum of
the clipped window and its gradient goes to EVERY tap equal to it; the average divides by the clipped window's own tap count
and every tap receives dy / count. The restatement itself is cross-checked on the CPU against torch's float64
max_pool2d / avg_pool2d(padding=0, ceil_mode=True), forward values and shapes, and on tie-free inputs their autograd.

Bounds: the max forward selects, it does not round: exact. Everything else: 1e-3 max-norm relative, the project's standing
budget for fp32 activations (README)."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.model import model_cnn
from fp64_model import build_model, png_dataset as _png_dataset, reference, rel as _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-3


# ------------------------------------------------------------------------------------------------- the float64 reference (NHWC)
def ref_out(r, k, s):
    return (r - 1) // s + 1 if s >= k else max(0, (r - 1 - k + s) // s) + 1


def _windows(H, W, size, stride):
    OH, OW = ref_out(H, size[0], stride[0]), ref_out(W, size[1], stride[1])
    for oy in range(OH):
        for ox in range(OW):
            y0, x0 = oy * stride[0], ox * stride[1]
            yield oy, ox, slice(y0, min(y0 + size[0], H)), slice(x0, min(x0 + size[1], W))


def ref_fwd(x, size, stride, mode):
    """x [N, H, W, C] float64 -> y [N, OH, OW, C]"""
    N, H, W, C = x.shape
    y = np.zeros((N, ref_out(H, size[0], stride[0]), ref_out(W, size[1], stride[1]), C), np.float64)
    for oy, ox, ys, xs in _windows(H, W, size, stride):
        win = x[:, ys, xs, :]
        assert win.shape[1] > 0 and win.shape[2] > 0
        y[:, oy, ox, :] = win.max(axis=(1, 2)) if mode == "max" else win.sum(axis=(1, 2)) / (win.shape[1] * win.shape[2])
    return y


def ref_bwd(x, dy, size, stride, mode):
    """gradient under the rules above; also the largest number of taps at a window's maximum (max mode)"""
    N, H, W, C = x.shape
    dx = np.zeros_like(x)
    most = 0
    for oy, ox, ys, xs in _windows(H, W, size, stride):
        win = x[:, ys, xs, :]
        g = dy[:, oy, ox, :][:, None, None, :]
        if mode == "max":
            hit = win == win.max(axis=(1, 2), keepdims=True)
            most = max(most, int(hit.sum(axis=(1, 2)).max()))
            dx[:, ys, xs, :] += hit * g
        else:
            dx[:, ys, xs, :] += g / (win.shape[1] * win.shape[2])
    return dx, most


def _clips(H, W, size, stride):
    OH, OW = ref_out(H, size[0], stride[0]), ref_out(W, size[1], stride[1])
    return (OH - 1) * stride[0] + size[0] > H, (OW - 1) * stride[1] + size[1] > W


# name: (N, H, W, C, (kh, kw), (sh, sw))
CASES = {
    "stem k3 s2, even map": (2, 32, 32, 64, (3, 3), (2, 2)),
    "k = s = 2, odd map": (2, 15, 15, 32, (2, 2), (2, 2)),
    "s > k": (2, 10, 10, 32, (2, 2), (3, 3)),
    "non-square map": (2, 14, 20, 32, (3, 3), (2, 2)),
    "kh != kw": (2, 16, 15, 64, (3, 2), (2, 2)),
    "sh != sw": (3, 13, 16, 32, (2, 3), (3, 2)),
    "stem of the 224 x 224 classifier": (2, 112, 112, 64, (3, 3), (2, 2)),
}


def _case(name):
    N, H, W, C, size, stride = CASES[name]
    ch, cw = _clips(H, W, size, stride)
    assert ch or cw, "no window of this case is clipped: it shows nothing"
    return N, H, W, C, size, stride


def _inputs(name, ties):
    N, H, W, C, size, stride = _case(name)
    rng = np.random.RandomState(sum(map(ord, name)))
    if ties:
        x = np.maximum(rng.randint(-3, 4, (N, H, W, C)), 0).astype(np.float32)        # a ReLU of small integers
    else:
        x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    OH, OW = ref_out(H, size[0], stride[0]), ref_out(W, size[1], stride[1])
    dy = rng.standard_normal((N, OH, OW, C)).astype(np.float32)
    return x, dy, size, stride


# ------------------------------------------------------------------------------------------------- the reference itself, on the CPU
@pytest.mark.parametrize("name", [n for n in CASES if "224" not in n])
@pytest.mark.parametrize("mode", ["max", "average_inc_pad"])
def test_reference_agrees_with_torch_ceil_mode_fp64(name, mode):
    """forward values and shapes of the numpy restatement against torch float64 (every case has H >= kh and W >= kw), and on the
    tie-free input the gradient against torch's autograd"""
    x, dy, size, stride = _inputs(name, ties=False)
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    assert x.shape[1] >= size[0] and x.shape[2] >= size[1]
    y = ref_fwd(x, size, stride, mode)
    t = torch.from_numpy(x).requires_grad_(True)
    f = Fn.max_pool2d if mode == "max" else Fn.avg_pool2d
    yt = f(t.permute(0, 3, 1, 2), size, stride, padding=0, ceil_mode=True)
    assert tuple(yt.shape) == (y.shape[0], y.shape[3], y.shape[1], y.shape[2])
    got = yt.detach().permute(0, 2, 3, 1).numpy()
    if mode == "max":
        assert np.array_equal(got, y)
    else:
        assert np.abs(got - y).max() <= 1e-14 * np.abs(y).max()
    dx, most = ref_bwd(x, dy, size, stride, mode)
    assert mode != "max" or most == 1, "the continuous input must be tie-free"
    yt.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.abs(t.grad.numpy() - dx).max() <= 1e-14 * np.abs(dx).max()


# ------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_max_forward_is_exact(hip, name):
    for ties in (False, True):
        x, _, size, stride = _inputs(name, ties)
        y = ops.maxpool_border_fwd(torch.from_numpy(x).cuda(), size, stride).cpu().numpy()
        ref = ref_fwd(x.astype(np.float64), size, stride, "max").astype(np.float32)
        assert y.shape == ref.shape
        assert np.array_equal(y, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_average_forward_vs_fp64(hip, name):
    x, _, size, stride = _inputs(name, ties=False)
    y = ops.avgpool_border_fwd(torch.from_numpy(x).cuda(), size, stride).cpu().numpy()
    ref = ref_fwd(x.astype(np.float64), size, stride, "average_inc_pad")
    assert y.shape == ref.shape
    err = _rel(y, ref)
    print("%s: average forward %.2e" % (name, err))
    assert err <= BOUND
    # a constant map stays that constant, in the clipped windows as well: the divisor is the window's own tap count
    one = torch.full(x.shape, 3.0, device="cuda")
    assert torch.all((ops.avgpool_border_fwd(one, size, stride) - 3.0).abs() <= 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_max_gradient_sends_to_every_tie(hip, name):
    """an input quantised so that ties occur (a ReLU of small integers): some window has two or more taps at its maximum, and dx
    follows the all-ties rule"""
    x, dy, size, stride = _inputs(name, ties=True)
    ref, most = ref_bwd(x.astype(np.float64), dy.astype(np.float64), size, stride, "max")
    assert most >= 2, "no window of this input has a tie"
    xd = torch.from_numpy(x).cuda()
    y = ops.maxpool_border_fwd(xd, size, stride)
    dx = ops.maxpool_border_bwd(xd, y, torch.from_numpy(dy).cuda(), size, stride)
    assert tuple(dx.shape) == x.shape
    err = _rel(dx.cpu().numpy(), ref)
    print("%s: max gradient with ties (up to %d taps at a maximum) %.2e" % (name, most, err))
    assert err <= BOUND
    # the first-tap rule of the cuDNN path is a different gradient on this input
    first, _ = ref_bwd(x.astype(np.float64) + 1e-9 * np.arange(x.size)[::-1].reshape(x.shape), dy.astype(np.float64), size, stride,
                       "max")
    assert _rel(first, ref) > BOUND
    # run to run: bitwise (a gather, no atomics)
    assert torch.equal(ops.maxpool_border_bwd(xd, y, torch.from_numpy(dy).cuda(), size, stride), dx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_max_gradient_tie_free_vs_torch_autograd_fp64(hip, name):
    x, dy, size, stride = _inputs(name, ties=False)
    ref, most = ref_bwd(x.astype(np.float64), dy.astype(np.float64), size, stride, "max")
    assert most == 1, "the continuous input must be tie-free"
    t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    Fn.max_pool2d(t.permute(0, 3, 1, 2), size, stride, padding=0, ceil_mode=True).backward(
        torch.from_numpy(dy.astype(np.float64)).permute(0, 3, 1, 2))
    xd = torch.from_numpy(x).cuda()
    y = ops.maxpool_border_fwd(xd, size, stride)
    dx = ops.maxpool_border_bwd(xd, y, torch.from_numpy(dy).cuda(), size, stride).cpu().numpy()
    errs = _rel(dx, ref), _rel(dx, t.grad.numpy())
    print("%s: max gradient, tie-free: %.2e (reference) %.2e (torch autograd)" % ((name,) + errs))
    assert max(errs) <= BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_average_gradient_vs_fp64(hip, name):
    x, dy, size, stride = _inputs(name, ties=False)
    ref, _ = ref_bwd(x.astype(np.float64), dy.astype(np.float64), size, stride, "average_inc_pad")
    dyd = torch.from_numpy(dy).cuda()
    dx = ops.avgpool_border_bwd(dyd, x.shape, size, stride)
    err = _rel(dx.cpu().numpy(), ref)
    print("%s: average gradient %.2e" % (name, err))
    assert err <= BOUND
    assert torch.equal(ops.avgpool_border_bwd(dyd, x.shape, size, stride), dx)


# ------------------------------------------------------------------------------------------------- through the layer
def _model(desc, data_shape, B, CLS, seed):
    m = build_model(desc, data_shape, B, CLS, seed=seed)
    m.class_labels = {"class%i" % i: i for i in range(CLS)}
    return m


@pytest.mark.gpu
def test_training_step_gradients_vs_fp64_autograd(hip):
    """`C.B[32,7,2] P.B[3,2] R` (the pool behind a convolution with no ReLU between: a tie-free map) trains one step; cost and both
    convolutions' weight gradients against a float64 torch-autograd restatement of the same net"""
    B, CLS = 4, 6
    m = _model("C.B[32,7,2] P.B[3,2] R", (3, 32, 32), B, CLS, seed=3)
    conv, pool, head = m.layers[1], m.layers[2], m.layers[3]
    assert pool.type_name == "pool" and not pool.ignore_border and pool.output_shape == (B, 32, 8, 8)
    assert all(_clips(16, 16, pool.size, pool.stride))
    assert head.filter_shape == (CLS, 32, 8, 8)
    m.build_train_func("sgd")
    rng = np.random.RandomState(5)
    x = rng.uniform(0.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    w0, w1 = [torch.from_numpy(l.omega.get_value().copy()).double().requires_grad_(True) for l in (conv, head)]
    b0 = torch.from_numpy(conv.beta.get_value().copy()).double()
    cost, _ = m.train_step(x, [{"image_class": int(c)} for c in cls], 0, 0, 0.1, [0.9], 0.0)
    # the map the pool saw is tie-free
    seen = conv.output.data[..., :32].double().cpu().numpy()
    _, most = ref_bwd(seen, np.zeros((B, 8, 8, 32)), pool.size, pool.stride, "max")
    assert most == 1
    cost_ref, _, _ = reference(m, x, {id(conv): [w0, b0], id(head): [w1]}, cls, True)      # (asserts the pool's output shape)
    cost_ref.backward()
    print("cost", cost, float(cost_ref.detach()))
    assert abs(cost - float(cost_ref.detach())) <= BOUND * abs(float(cost_ref.detach()))
    for name, l, t in (("stem", conv, w0), ("head", head, w1)):
        err = _rel(l.omega.get_grad().copy(), t.grad.numpy())
        print("%s convolution weight gradient %.2e" % (name, err))
        assert err <= BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("pool_desc,fused", [("P.B[3,2]", False), ("P[3,2,1]", True)])
def test_fused_stem_pass_runs_for_the_cudnn_mode_only(hip, monkeypatch, pool_desc, fused):
    """`C.B[32,7,2] BN A <pool> C[32,3] BN A R`: the fused BN + ReLU + max-pool pass does not run for `P.B[3,2]` (BN + ReLU, then
    the border-keeping kernels) and does run for the same net written with `P[3,2,1]`"""
    assert ops.BN_POOL_FUSE
    calls = {"fused": 0, "border_fwd": 0, "border_bwd": 0}

    def counted(key, fn):
        def wrapper(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(ops, "bn_relu_pool_fwd_train", counted("fused", ops.bn_relu_pool_fwd_train))
    monkeypatch.setattr(ops, "maxpool_border_fwd", counted("border_fwd", ops.maxpool_border_fwd))
    monkeypatch.setattr(ops, "maxpool_border_bwd", counted("border_bwd", ops.maxpool_border_bwd))
    B, CLS = 4, 6
    m = _model("C.B[32,7,2] BN A %s C[32,3] BN A R" % pool_desc, (3, 32, 32), B, CLS, seed=7)
    pool = [l for l in m.layers if l.type_name == "pool"][0]
    assert pool.output_shape == (B, 32, 8, 8)
    m.build_train_func("sgd")
    rng = np.random.RandomState(8)
    x = rng.uniform(0.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    metas = [{"image_class": int(c)} for c in rng.randint(0, CLS, B)]
    before = m.layers[1].omega.get_value().copy()
    cost, _ = m.train_step(x, metas, 0, 0, 0.1, [0.9], 0.0)
    assert np.isfinite(cost)
    assert not np.array_equal(m.layers[1].omega.get_value(), before), "the stem's weights did not move"
    if fused:
        assert calls == {"fused": 1, "border_fwd": 0, "border_bwd": 0}, calls
    else:
        assert calls == {"fused": 0, "border_fwd": 1, "border_bwd": 1}, calls
        # behind the ReLU the pool's input has windows of zeros: the output is their maximum, the stem still received a gradient
        xin, y = pool.input.data, pool.output.data
        ref = ref_fwd(xin.double().cpu().numpy(), pool.size, pool.stride, "max").astype(np.float32)
        assert np.array_equal(y.cpu().numpy(), ref)
    pr = m.predict_output_step(x)
    assert pr.shape == (B, CLS) and np.isfinite(pr).all() and np.allclose(pr.sum(axis=1), 1.0, atol=1e-4)


@pytest.mark.gpu
def test_average_border_layer_trains_and_predicts(hip):
    """`P.AB[2]` on an odd map inside a net: one step, then test-mode probabilities against float64"""
    B, CLS = 4, 5
    m = _model("C.B[32,3] P.AB[2] R", (3, 15, 15), B, CLS, seed=9)
    conv, pool, head = m.layers[1], m.layers[2], m.layers[3]
    assert pool.mode == "average_inc_pad" and not pool.ignore_border and pool.output_shape == (B, 32, 8, 8)
    m.build_train_func("sgd")
    rng = np.random.RandomState(10)
    x = rng.uniform(0.0, 1.0, (B, 3, 15, 15)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    w0, w1 = [torch.from_numpy(l.omega.get_value().copy()).double().requires_grad_(True) for l in (conv, head)]
    b0 = torch.from_numpy(conv.beta.get_value().copy()).double()
    cost, _ = m.train_step(x, [{"image_class": int(c)} for c in cls], 0, 0, 0.1, [0.9], 0.0)

    cost_ref, _, _ = reference(m, x, {id(conv): [w0, b0], id(head): [w1]}, cls, True)
    cost_ref.backward()
    assert abs(cost - float(cost_ref.detach())) <= BOUND * abs(float(cost_ref.detach()))
    for l, t in ((conv, w0), (head, w1)):
        assert _rel(l.omega.get_grad().copy(), t.grad.numpy()) <= BOUND
    pr = m.predict_output_step(x)
    with torch.no_grad():
        now = [torch.from_numpy(l.omega.get_value().copy()).double() for l in (conv, head)]
        _, logits, _ = reference(m, x, {id(conv): [now[0], torch.from_numpy(conv.beta.get_value().copy()).double()],
                                        id(head): [now[1]]}, cls, False)
        pr_ref = torch.softmax(logits, dim=1).numpy()
    assert np.abs(pr - pr_ref).max() <= BOUND * pr_ref.max()


# ------------------------------------------------------------------------------------------------- command line
@pytest.mark.gpu
def test_cli_predict_and_update_bn_on_a_border_keeping_model(hip, tmp_path):
    """model-predict (single mode), model-update-bn and model-modify --use-cudnn-pool on a saved `P.B` model and a folder of
    generated PNGs: each finishes; the updated model keeps its border-keeping pool, the converted one predicts as well"""
    B, CLS = 4, 3
    m = _model("C.B[32,7,2] BN A P.B[3,2] C[32,3] BN A R", (3, 32, 32), B, CLS, seed=11)
    data = str(tmp_path / "data")
    _png_dataset(data, classes=CLS, per_class=4, seed=3)
    src, upd, conv = str(tmp_path / "border.mdl.gz"), str(tmp_path / "updated.mdl.gz"), str(tmp_path / "cudnn.mdl.gz")
    model_cnn.save_to_file(m, src)

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        log = r.stdout + r.stderr
        assert r.returncode == 0, (cmd[0], log[-3000:])
        return log

    predict = [os.path.join(ROOT, "bin", "model-predict"), "--input", data, "--extension", "png", "--batch-size", str(B),
               "--predict-mode", "single", "--model"]
    assert "Top1 - Error Rate" in run(predict + [src])
    log = run([os.path.join(ROOT, "bin", "model-update-bn"), "--model", src, "--output", upd, "--input", data, "--extension", "png",
               "--batch-size", str(B), "--seed", "1", "--thread-num", "1"])
    assert "Found 2 batch norm layers" in log
    got = model_cnn.load_from_file(upd, B)
    pool = [l for l in got.layers if l.type_name == "pool"][0]
    assert pool.ignore_border is False and pool.pad == (0, 0) and pool.output_shape == (B, 32, 8, 8)
    bns = [(a, b) for a, b in zip(m.layers, got.layers) if a.type_name == "batchnorm"]
    assert len(bns) == 2
    for a, b in bns:
        assert not np.array_equal(a.mean.get_value(), b.mean.get_value())
    assert "Top1 - Error Rate" in run(predict + [upd])
    run([os.path.join(ROOT, "bin", "model-modify"), "--input", upd, "--output", conv, "--use-cudnn-pool"])
    pool = [l for l in model_cnn.load_from_file(conv, B).layers if l.type_name == "pool"][0]
    assert pool.ignore_border is True and pool.pad == (1, 1) and pool.output_shape == (B, 32, 8, 8)
    assert "Top1 - Error Rate" in run(predict + [conv])
