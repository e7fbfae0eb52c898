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

from denet_amd import ops
from denet_amd.model import model_cnn, zoo
from fp64_model import act64 as _act64, build_model, param_layers as _param_layers, png_dataset as _png_dataset, reference as _reference
from fp64_model import rel as _rel, sgd_step_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["sigmoid", "tanh", "elu", "softplus"]


@pytest.fixture(autouse=True)
def _algorithm_tables_restored():
    """ops memoises per geometry which implementation a convolution pass takes (ops._WINO); the small geometries of this file
    are those of other files' tests, which must find the tables as a fresh process has them"""
    with ops.algorithms():
        yield


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


def _build(desc, activation, B, size, class_num=10):
    """batch norms away from (gamma, beta) = (1, 0), logits of order one"""
    return build_model(desc, (3, size, size), B, class_num, activation, spread_bn=True, head_scale=0.05)


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
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
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
        for l, p, e_g, e_p, _, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
            assert float(g_ref.abs().max()) > 0, (l.layer_index, p.name)
            report.append((e_g, e_p, "%s L%d %s %s: grad %.2e, update %.2e" % (activation, l.layer_index, l.type_name, p.name, e_g, e_p)))
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
                m_ref = (1.0 - l.momentum) * stats[id(l)]["mean"]
                s_ref = l.momentum + (1.0 - l.momentum) * stats[id(l)]["stdinv"]
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
