"""The sigmoid / tanh / elu / softplus activations on the device (csrc/activation.hip), against float64 torch on the host.

- the three kernels for every kind: values, finiteness, exact zeros in the padding channels;
- one training step and the test-mode pass of a small network built from desc tokens, for every kind and for relu (control);
- relu models launch none of the new kernels and stay bit-identical;
- the padding channels behind a consumer (max pool) and in the gradient that reaches the convolution;
- the command lines: model-train --activation, model-predict, model-modify --activation."""
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
from denet_amd.model import model_cnn, zoo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["sigmoid", "tanh", "elu", "softplus"]


@pytest.fixture(autouse=True)
def _algorithm_tables_restored():
    """ops memoises per geometry which implementation a convolution pass takes (ops._WINO); the small geometries of this file
    are those of other files' tests, which must find the tables as a fresh process has them"""
    ops._load_tuned_once()
    saved = (ops.POLICY, dict(ops._WINO), set(ops._TUNED))
    yield
    ops.POLICY = saved[0]
    ops._WINO.clear()
    ops._WINO.update(saved[1])
    ops._TUNED.clear()
    ops._TUNED.update(saved[2])


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _act64(name, x):
    """the table of the issue, in the dtype of x (float64 here): denet/layer/activation.py:25-44"""
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "elu":
        return torch.where(x > 0, x, torch.expm1(x))
    if name == "softplus":
        return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    if name in ("relu", "relu-safe"):
        return torch.relu(x)
    assert name == "none", name
    return x


def _dact64(name, x):
    """d act / dx from the INPUT, in float64 (the kernels write it from the output)"""
    if name == "sigmoid":
        s = torch.sigmoid(x)
        return s * (1 - s)
    if name == "tanh":
        return 1 - torch.tanh(x) ** 2
    if name == "elu":
        return torch.where(x > 0, torch.ones_like(x), torch.exp(x))
    assert name == "softplus", name
    return torch.sigmoid(x)


# ------------------------------------------------------------------------------------------------- kernels against float64
def _inputs(M, C, CP, seed):
    """a ramp over [-100, 100] plus N(0, 3^2) plus +-0 and denormals in the logical channels; non-zero garbage in the padding"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = M * C
    x = torch.randn(n, generator=g) * 3.0
    ramp = torch.linspace(-100.0, 100.0, n // 2)
    x[: n // 2] = ramp[torch.randperm(n // 2, generator=g)]
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 100.0, -100.0, 88.8, -88.8, 103.0, -103.0, 17.0, -17.0])
    x[n // 2: n // 2 + len(special)] = special
    x = x[torch.randperm(n, generator=g)].view(M, C)
    full = torch.empty(M, CP)
    full[:, :C] = x
    junk = torch.randn(M, CP - C, generator=g) * 50.0 + 7.0
    junk[junk == 0] = 1.0
    full[:, C:] = junk
    if CP > C:
        full[0, C] = float("inf")              # whatever those lanes hold
        full[1 % M, C] = float("nan")
    return full


def _padding_is_plus_zero(t, C):
    pad = t[..., C:].contiguous().cpu().view(torch.int32)
    return bool((pad == 0).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [3, 100, 128])
def test_kernels_vs_fp64(hip, kind, C):
    """act_fwd, act_bwd and add_act: finite, +0.0 bit patterns in channels C..CP-1, max-norm relative error <= 2e-4 (the per-op
    bound of this project; fp32 torch on the host measured 9e-8 forward and 3e-7 backward on these inputs)."""
    CP = 4 if C == 3 else ((C + 31) // 32) * 32
    shapes = [(1237, CP)]
    if C != 3:
        shapes.append((3, 7, 59, CP))                       # NHWC, and more vectors than one sweep of a small grid
    for shape in shapes:
        M = int(np.prod(shape[:-1]))                        # not a multiple of the 256 x 4 elements a workgroup covers per sweep
        assert (M * CP // 4) % 256 != 0
        x = _inputs(M, C, CP, seed=C * 10 + len(shape))
        dy = _inputs(M, C, CP, seed=C * 10 + len(shape) + 5) * 0.01
        b = _inputs(M, C, CP, seed=C * 10 + len(shape) + 7)
        xd, dyd, bd = x.view(shape).cuda(), dy.view(shape).cuda(), b.view(shape).cuda()
        x64, dy64, b64 = x[:, :C].double(), dy[:, :C].double(), b[:, :C].double()

        y = ops.act_fwd(xd, C, kind)
        assert y.shape == xd.shape
        yl = y.view(M, CP)[:, :C].cpu()
        assert bool(torch.isfinite(yl).all()) and _padding_is_plus_zero(y, C)
        e_f = _rel(yl, _act64(kind, x64))

        dx = ops.act_bwd(y, dyd, C, kind)
        dxl = dx.view(M, CP)[:, :C].cpu()
        assert bool(torch.isfinite(dxl).all()) and _padding_is_plus_zero(dx, C)
        e_b = _rel(dxl, dy64 * _dact64(kind, x64))
        # the padding of y may hold anything as well (a caller's tensor): the gradient's padding is still +0
        yg = y.clone()
        yg.view(M, CP)[:, C:] = xd.view(M, CP)[:, C:]
        dx2 = ops.act_bwd(yg, dyd, C, kind)
        assert _padding_is_plus_zero(dx2, C) and torch.equal(dx2.view(M, CP)[:, :C], dx.view(M, CP)[:, :C])

        ya = ops.add_act(xd, bd, C, kind)
        yal = ya.view(M, CP)[:, :C].cpu()
        assert bool(torch.isfinite(yal).all()) and _padding_is_plus_zero(ya, C)
        s32 = (x[:, :C] + b[:, :C])                           # the sum as the kernel forms it, in fp32
        e_a = _rel(yal, _act64(kind, s32.double()))
        e_a64 = _rel(yal, _act64(kind, x64 + b64))
        print("%s C=%d CP=%d M=%d: forward %.2e, backward %.2e, add_act %.2e (against the fp64 sum %.2e)" % (
            kind, C, CP, M, e_f, e_b, e_a, e_a64))
        assert e_f <= 2e-4 and e_b <= 2e-4 and e_a <= 2e-4 and e_a64 <= 2e-4

        # the saturated ends, exactly
        ends = torch.zeros(1, CP)
        ends[0, 0], ends[0, 1] = -100.0, 100.0
        ye = ops.act_fwd(ends.cuda(), 2, kind).cpu()[0]
        want = {"sigmoid": (0.0, 1.0), "tanh": (-1.0, 1.0), "elu": (-1.0, 100.0), "softplus": (0.0, 100.0)}[kind]
        assert abs(float(ye[0]) - want[0]) <= 1e-37 and float(ye[1]) == want[1], (kind, ye[:2])


# ------------------------------------------------------------------------------------------------- a network against float64
NET_DESC = "C.B[32,3] A C[32,3] BN A P[2] nRSN.O[2,64,3,2] nRSN[2,64,3,2,32] R.C"


def _build(desc, activation, B, size, class_num=10, seed=5, border="half"):
    np.random.seed(seed)
    m = model_cnn.ModelCNN()
    m.batch_size = B
    m.class_num = class_num
    m.build(desc, (3, size, size), activation, border, ["he-backward"])
    # batch norms away from (gamma, beta) = (1, 0): both gradients carry weight
    rng = np.random.RandomState(seed + 1)
    for l in model_cnn.walk_layers(m.layers):
        if l.type_name == "batchnorm" and l.enabled:
            l.omega.set_value(rng.uniform(0.7, 1.3, l.omega.value.shape))
            l.beta.set_value(rng.normal(0.0, 0.3, l.beta.value.shape))
    if m.layers[-1].type_name == "regression":
        # logits of order one: with the initialisation as it is they reach the hundreds on these nets, the soft-max saturates (the
        # test-mode probabilities come out as exact zeros and ones) and the comparison of the probabilities says nothing
        head = m.layers[-2]
        head.omega.set_value(head.omega.get_value() * 0.05)
    return m


def _param_layers(model):
    out = []
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name == "conv":
            out.append((l, [l.omega] + ([l.beta] if l.use_bias else [])))
        elif l.type_name == "batchnorm" and l.enabled:
            out.append((l, [l.omega, l.beta]))
    return out


def _reference(model, x, params, cls, train, running=None):
    """the layer list in float64 on the host, wired like the layers themselves: every layer reads the tensor of its `input` handle
    and writes the one of its `output` handle. Returns (cost, logits, {id(batch norm): (mean, stdinv) of the batch})."""
    val = {id(model.layers[0].output): torch.from_numpy(x).double()}
    stats = {}

    def run(l):
        t = l.type_name
        if t == "initial":
            return
        h = val[id(l.input)]
        if t == "conv":
            ps = params[id(l)]
            h = Fn.conv2d(h, ps[0].flip(2, 3), stride=l.stride[0], padding=l.pad)      # (true convolution: convolution.py:80-83)
            if l.use_bias:
                h = h + ps[1][None, :, None, None]
        elif t == "batchnorm":
            if not l.enabled:
                return
            gamma, beta = params[id(l)]
            if train:
                mean = h.mean(dim=(0, 2, 3))
                var = h.var(dim=(0, 2, 3), unbiased=False)
                stats[id(l)] = (mean.detach(), 1.0 / torch.sqrt(var.detach() + l.eps))
                h = (h - mean[None, :, None, None]) / torch.sqrt(var + l.eps)[None, :, None, None]
            else:
                rm, rs = running[id(l)]
                inv = 1.0 / torch.sqrt((1.0 / rs) ** 2 + l.eps)                         # batch_norm.py:50-52: eps twice
                h = (h - rm[None, :, None, None]) * inv[None, :, None, None]
            h = h * gamma[None, :, None, None] + beta[None, :, None, None]
        elif t == "activation":
            h = _act64(l.activation, h)
        elif t == "pool":
            assert l.mode == "max"
            h = Fn.max_pool2d(h, l.size[0], l.stride[0], l.pad[0])
        elif t == "resnet":
            for s in l.layers:
                run(s)
            y = val[id(l.layers[l.n_main - 1].output)]
            sc = l.layers[l.n_main:]
            xs = val[id(sc[-1].output)] if sc else h
            h = xs + y if "pre-activation" in l.version else _act64(l.activation, xs + y)      # resnet.py:109-113
        elif t == "regression":
            yc, xc = l.valid[0][1], l.valid[0][2]
            logits = h[:, :, yc, xc]
            lp = torch.log_softmax(logits, dim=1)
            val["cost"] = -lp[torch.arange(len(cls)), torch.from_numpy(cls)].mean()
            val["logits"] = logits
            return
        else:
            raise AssertionError("unexpected layer " + t)
        val[id(l.output)] = h

    for l in model.layers:
        run(l)
    return val["cost"], val["logits"], stats


class _direct_policy:
    """every convolution pass on the direct kernels (exact fp32 FMA chains)"""

    def __enter__(self):
        self.saved = (ops.POLICY, dict(ops._WINO))
        ops._WINO.clear()
        ops.POLICY = lambda mode, g: 0

    def __exit__(self, *a):
        ops.POLICY = self.saved[0]
        ops._WINO.clear()
        ops._WINO.update(self.saved[1])


@pytest.mark.parametrize("activation", KINDS + ["relu"])
def test_training_step_vs_fp64(hip, activation):
    """one SGD step at B = 4 on the direct kernels: cost, every parameter gradient, the update and the batch-norm running
    statistics against float64 autograd, <= 1e-3 max-norm (the bound of test_simple_cifar10_gpu.test_training_step_vs_fp64);
    then the test-mode probabilities with the updated parameters, with the inference fold at its default and switched off,
    <= 1e-3 against float64. The two device results against each other: <= 1e-4 of the largest probability - both are fp32
    evaluations of the same function, the fold only moves gamma / sqrt(var + eps) from the output into the filters (one more
    rounding per weight, ~6e-8 relative, over reductions of at most 1 152 terms and a dozen layers).
    relu is the control: the same harness on ground that worked before."""
    B, CLS, LR, MOM, DECAY = 4, 10, 0.1, 0.9, 0.0005
    with _direct_policy():
        model = _build(NET_DESC, activation, B, 32, CLS)
        blocks = [l for l in model.layers if l.type_name == "resnet"]
        assert [b.version for b in blocks] == ["original"] * 2 + ["pre-activation"] * 2
        assert len(blocks[0].layers) > blocks[0].n_main and len(blocks[2].layers) > blocks[2].n_main      # strided projections
        model.build_train_func("sgd")
        rng = np.random.RandomState(11)
        x = rng.uniform(-1.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
        cls = rng.randint(0, CLS, B)
        metas = [{"image_class": int(c)} for c in cls]
        weights = set(id(p) for l in model.layers for p in l.weights())
        before = _param_layers(model)
        values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}

        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
        torch.cuda.synchronize()
        tiles = [(l._cache().get("fwd_tile"), l._cache().get("dgrad_tile")) for l, _ in before if l.type_name == "conv"]
        assert all(t[0] == 0 and t[1] in (0, None) for t in tiles), tiles

        params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
        cost_ref, _, stats = _reference(model, x, params, cls, train=True)
        cost_ref.backward()
        e_cost = abs(cost - float(cost_ref.detach())) / abs(float(cost_ref.detach()))
        report, bad = [], []
        for n, (l, ps) in enumerate(before):
            for p, v, t in zip(ps, values[id(l)], params[id(l)]):
                g_dev = torch.from_numpy(p.get_grad().copy()).double()
                g_ref = t.grad
                assert float(g_ref.abs().max()) > 0, (n, p.name)
                dec = DECAY if id(p) in weights else 0.0
                v64 = torch.from_numpy(v).double()
                p_ref = v64 - LR * (g_ref + dec * v64)                  # SGD at iteration 0 (no momentum yet), L2 decay on the weights
                p_dev = torch.from_numpy(p.get_value().copy()).double()
                e_g, e_p = _rel(g_dev, g_ref), _rel(p_dev - v64, p_ref - v64)
                report.append((e_g, e_p, "%s #%d %s %s: grad %.2e, update %.2e" % (activation, n, l.type_name, p.name, e_g, e_p)))
                if not (e_g <= 1e-3 and e_p <= 1e-3):
                    bad.append(report[-1][2])
        print("%s: cost %.6f (float64 %.6f, %.2e), worst gradient %.2e, worst update %.2e over %d arrays" % (
            activation, cost, float(cost_ref.detach()), e_cost, max(r[0] for r in report), max(r[1] for r in report), len(report)))
        assert e_cost <= 1e-3, (cost, float(cost_ref.detach()))
        assert not bad, bad
        running, e_run = {}, 0.0
        for l, _ in before:
            if l.type_name == "batchnorm":
                rm, rs = torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double()
                m_ref, s_ref = (1.0 - l.momentum) * stats[id(l)][0], l.momentum + (1.0 - l.momentum) * stats[id(l)][1]
                e_run = max(e_run, _rel(rm, m_ref), _rel(rs, s_ref))
                running[id(l)] = (rm, rs)
        print("%s: running statistics %.2e" % (activation, e_run))
        assert e_run <= 1e-3

        # test mode, with the updated parameters and statistics
        now = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in before}
        with torch.no_grad():
            _, logits, _ = _reference(model, x, now, cls, train=False, running=running)
        pr_ref = torch.softmax(logits, dim=1)
        assert ops.INFER_FOLD == (os.environ.get("DENET_INFER_FOLD", "1") != "0")
        head = model.layers[-1].input                                   # the logit map in front of the soft-max, [B, 1, 1, cp]
        pr_fold = torch.from_numpy(model.predict_output_step(x)).double()
        z_fold = head.data.view(B, -1)[:, :CLS].double().cpu()
        with ops.infer_fold(False):
            pr_plain = torch.from_numpy(model.predict_output_step(x)).double()
            z_plain = head.data.view(B, -1)[:, :CLS].double().cpu()
        print("%s: test-mode logits up to %.2f, fold %.2e, no fold %.2e; largest probability %.3f" % (
            activation, float(logits.abs().max()), _rel(z_fold, logits), _rel(z_plain, logits), float(pr_ref.max())))
        assert _rel(z_fold, logits) <= 1e-3 and _rel(z_plain, logits) <= 1e-3
        assert pr_fold.shape == (B, CLS) and pr_plain.shape == (B, CLS)
        e1 = float((pr_fold - pr_ref).abs().max() / pr_ref.max())
        e2 = float((pr_plain - pr_ref).abs().max() / pr_ref.max())
        e3 = float((pr_fold - pr_plain).abs().max() / pr_ref.max())
        print("%s: test-mode probabilities, fold %.2e, no fold %.2e, one against the other %.2e" % (activation, e1, e2, e3))
        assert bool(torch.isfinite(pr_fold).all()) and bool(torch.isfinite(pr_plain).all())
        assert e1 <= 1e-3 and e2 <= 1e-3 and e3 <= 1e-4


# ------------------------------------------------------------------------------------------------- relu is untouched
RELU_DESC = "C[32,3] BN A nRSN.O[2,32,3,1] nRSN.O[2,64,3,2] R.C"


def _relu_step(monkeypatch, wrap):
    calls = {"act_fwd": 0, "act_bwd": 0, "add_act": 0}
    for name in calls:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name), calls))
    model = _build(RELU_DESC, "relu", 4, 16)
    model.build_train_func("sgd")
    rng = np.random.RandomState(3)
    x = rng.uniform(-1.0, 1.0, (4, 3, 16, 16)).astype(np.float32)
    metas = [{"image_class": int(c)} for c in rng.randint(0, 10, 4)]
    cost, _ = model.train_step(x, metas, 0, 0, 0.1, [0.9], 0.0005)
    torch.cuda.synchronize()
    grads = [p.get_grad().copy() for _, ps in _param_layers(model) for p in ps]
    pr = model.predict_output_step(x)
    with ops.infer_fold(False):
        pr2 = model.predict_output_step(x)
    return calls, cost, grads, pr, pr2


def test_relu_launches_none_of_the_new_kernels(hip, monkeypatch):
    def counting(name, fn, calls):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    def raising(name, fn, calls):
        def f(*a, **k):
            raise AssertionError("ops.%s called by a relu model" % name)
        return f

    calls, cost, grads, pr, pr2 = _relu_step(monkeypatch, counting)
    assert calls == {"act_fwd": 0, "act_bwd": 0, "add_act": 0}, calls
    calls_b, cost_b, grads_b, pr_b, pr2_b = _relu_step(monkeypatch, raising)
    assert math.isfinite(cost) and np.float32(cost).tobytes() == np.float32(cost_b).tobytes()
    assert len(grads) == len(grads_b) > 10
    for a, b in zip(grads, grads_b):
        assert a.tobytes() == b.tobytes()
    assert pr.tobytes() == pr_b.tobytes() and pr2.tobytes() == pr2_b.tobytes()


def test_smooth_model_launches_the_new_kernels(hip, monkeypatch):
    """the counterpart: the same wrappers do count when the activation is not a ReLU (the counting itself works)"""
    calls = {"act_fwd": 0, "act_bwd": 0, "add_act": 0}
    for name in calls:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda n, f: lambda *a, **k: (calls.__setitem__(n, calls[n] + 1), f(*a, **k))[1])(name, fn))
    model = _build(RELU_DESC, "elu", 4, 16)
    model.build_train_func("sgd")
    rng = np.random.RandomState(3)
    x = rng.uniform(-1.0, 1.0, (4, 3, 16, 16)).astype(np.float32)
    metas = [{"image_class": int(c)} for c in rng.randint(0, 10, 4)]
    cost, _ = model.train_step(x, metas, 0, 0, 0.1, [0.9], 0.0005)
    assert math.isfinite(cost)
    # one `A` layer + one inner `BN A` per block forward, one block exit each; the backward pass mirrors them
    assert calls == {"act_fwd": 5, "act_bwd": 9, "add_act": 4}, calls
    for fold in (True, False):
        for k in calls:
            calls[k] = 0
        with ops.infer_fold(fold):
            assert np.isfinite(model.predict_output_step(x)).all()
        assert calls == {"act_fwd": 5, "act_bwd": 0, "add_act": 4}, (fold, calls)


# ------------------------------------------------------------------------------------------------- padding through a consumer
def test_padding_channels_through_a_pool(hip):
    """100 logical channels in 128 physical ones, sigmoid (0.5 at 0), a max pool behind it: the pooled tensor holds +0 in
    channels 100..127, and so does the gradient that reaches the convolution.

    (The issue's recipe for this test reads `C[100,3] BN A P[2]`. A batch norm of this build takes multiples of 32 channels only
    (BatchNormLayer asserts an unpadded channel count), so that model cannot be built; the bias of `C.B` stands in for the batch
    norm's shift, the activation, the padding and the consumer are as asked.)"""
    with pytest.raises(AssertionError, match="unpadded channel count"):
        _build("C[100,3] BN A P[2]", "sigmoid", 2, 16)
    model = _build("C.B[100,3] A P[2] R.C", "sigmoid", 4, 16)
    conv, act, pool = model.layers[1], model.layers[2], model.layers[3]
    assert (conv.type_name, act.type_name, pool.type_name) == ("conv", "activation", "pool")
    assert act.output.cp == 128 and act.output_shape[1] == 100
    model.build_train_func("sgd")
    rng = np.random.RandomState(4)
    x = rng.uniform(-1.0, 1.0, (4, 3, 16, 16)).astype(np.float32)
    metas = [{"image_class": int(c)} for c in rng.randint(0, 10, 4)]
    cost, _ = model.train_step(x, metas, 0, 0, 0.1, [0.9], 0.0005)
    torch.cuda.synchronize()
    assert math.isfinite(cost)
    for t in (act.output.data, pool.output.data, conv.output.grad):
        assert t is not None and t.shape[-1] == 128
        assert _padding_is_plus_zero(t, 100)
        assert float(t[..., :100].abs().max()) > 0
    # sigmoid really ran on the logical channels: strictly inside (0, 1), 0.5 nowhere exactly by construction of the bias-free lanes
    yl = act.output.data[..., :100]
    assert float(yl.min()) > 0.0 and float(yl.max()) < 1.0
    model.predict_output_step(x)
    assert _padding_is_plus_zero(act.output.data, 100) and _padding_is_plus_zero(pool.output.data, 100)


# ------------------------------------------------------------------------------------------------- command line
def _png_dataset(root, classes=3, per_class=4, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    for c in range(classes):
        d = os.path.join(root, "class%i" % c)
        os.makedirs(d)
        for j in range(per_class):
            img = rng.randint(0, 256, (32, 32, 3)).astype(np.uint8)
            img[..., c] = 200 + 10 * (j % 5)
            Image.fromarray(img).save(os.path.join(d, "img%i.png" % j))


def _names(layers):
    out = []
    for l in layers:
        if l["type"] in ("activation", "resnet"):
            out.append(l["activation"])
        out += _names(l.get("layers", []))
    return out


def _finite_predictions(fname):
    m = model_cnn.load_from_file(fname, 4)
    x = np.random.RandomState(9).uniform(0.0, 1.0, (4,) + tuple(m.data_shape)).astype(np.float32)
    pr = m.predict_output_step(x)
    assert pr.shape[0] == 4 and np.isfinite(pr).all() and np.allclose(pr.sum(axis=1), 1.0, atol=1e-4)
    return m


def test_cli_train_predict_modify(hip, tmp_path):
    """model-train --activation tanh (two epochs of the getting-started recipe), model-predict, model-modify --activation elu,
    model-predict: each must exit 0 before the next one starts"""
    train_dir, test_dir, out = str(tmp_path / "train"), str(tmp_path / "test"), tmp_path / "out"
    _png_dataset(train_dir, seed=1)
    _png_dataset(test_dir, per_class=2, seed=2)
    out.mkdir()

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        log = r.stdout + r.stderr
        assert r.returncode == 0, (cmd[0], log[-3000:])
        return log

    desc = zoo.SIMPLE_CIFAR10_DESC.split()
    log = run([os.path.join(ROOT, "bin", "model-train"), "--seed", "0", "--distort-mode", "o4", "--solver", "sgd", "--border-mode",
               "same", "--augment-mirror", "--activation", "tanh", "--epochs", "2", "--batch-size", "4", "--train", train_dir,
               "--test", test_dir, "--extension", "png", "--learn-rate", "0.1", "--learn-momentum", "0.9", "--learn-anneal", "0.5",
               "--learn-anneal-epochs", "15", "30", "--learn-decay", "0.0005", "--output-prefix", str(out / "model"),
               "--model-desc"] + desc)
    costs = [float(c) for c in re.findall(r"cost: (\S+) \(lr", log)]
    assert len(costs) >= 2 and all(math.isfinite(c) for c in costs), log[-3000:]
    final = sorted(glob.glob(str(out / "model_epoch*_final.mdl.gz")))[-1:]
    assert final and "epoch001" in final[0], os.listdir(str(out))
    predict = [os.path.join(ROOT, "bin", "model-predict"), "--input", test_dir, "--extension", "png", "--batch-size", "4",
               "--predict-mode", "single", "--model"]
    assert "Top1 - Error Rate" in run(predict + [final[0]])
    m = _finite_predictions(final[0])
    names = _names(m.export_json()["layers"])
    assert names and set(names) == {"tanh"}

    elu = str(out / "elu.mdl.gz")
    run([os.path.join(ROOT, "bin", "model-modify"), "--input", final[0], "--output", elu, "--activation", "elu"])
    assert "Top1 - Error Rate" in run(predict + [elu])
    m2 = _finite_predictions(elu)
    names2 = _names(m2.export_json()["layers"])
    assert len(names2) == len(names) and set(names2) == {"elu"}
    # nothing but the names moved
    for la, lb in zip(model_cnn.walk_layers(m.layers), model_cnn.walk_layers(m2.layers)):
        for pa, pb in zip(la.all_params() if hasattr(la, "all_params") else [], lb.all_params() if hasattr(lb, "all_params") else []):
            np.testing.assert_array_equal(pa.get_value(), pb.get_value())
