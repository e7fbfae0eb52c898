"""Rectangular filters and per-axis strides (`C.X` / `DC.X`, csrc/conv_rect.hip) on the device, against float64.

The arbiter is PyTorch's CPU conv2d in float64 with the filters flipped (the reference's conv2d is a true convolution,
denet/layer/convolution.py:80-83; the device stores correlation taps), gradients by autograd. Padding per axis: `valid` (0, 0),
`half` (R // 2, S // 2), `full` (R - 1, S - 1), `same` (R // 2, S // 2) with the output cut to H x W - the reference crops the full
convolution at ((R - 1) // 2, (S - 1) // 2), convolution.py:76-80, which is the same thing. `same` exists for stride 1 only
(ConvLayer asserts it), so the grid pairs it with stride (1, 1).

Bound of the kernel checks: max|a - b| / max|b| <= 1e-5, the figure every direct fp32 kernel of this project is held to
(tests/test_simple_cifar10_gpu.py). Whole steps: 1e-3 max-norm, the project's whole-step budget."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.lib import DenetHipError
from denet_amd.model import model_cnn
from denet_amd.model.audit import KernelAudit
from fp64_model import build_model, param_layers, reference, rel as _rel, relu_masks_of, sgd_step_errors

pytestmark = pytest.mark.gpu

FILTERS = [(1, 7), (7, 1), (1, 3), (3, 1), (3, 5), (2, 3), (3, 3)]
STRIDES = [(1, 1), (2, 1), (1, 2), (2, 2), (4, 1)]
BORDERS = ["valid", "half", "full", "same"]
BOUND = 1e-5


def _padding(border, R, S):
    return {"valid": (0, 0), "half": (R // 2, S // 2), "full": (R - 1, S - 1), "same": (R // 2, S // 2)}[border]


def _nhwc(t, cp):
    """[N, C, H, W] float64 -> the device's [N, H, W, cp] float32, padding channels zero"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cp, dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 1).float()
    return out.cuda()


def _krsc(w, kp, cp, s_pad=None):
    """reference filters [K, C, R, S] -> the device's correlation taps [kp][R][s_pad][cp], zero padded"""
    k, c, r, s = w.shape
    out = torch.zeros(kp, r, s_pad or s, cp, dtype=torch.float32)
    out[:k, :, :s, :c] = w.flip(2, 3).permute(0, 2, 3, 1).float()
    return out.cuda()


def _up32(v):
    return (v + 31) // 32 * 32


def _check_passes(N, H, W, C, K, R, S, stride, border, seed, first_layer=False):
    """all three passes of one geometry against float64; returns the measured errors"""
    ph, pw = _padding(border, R, S)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, R, S, generator=g, dtype=torch.float64) / math.sqrt(C * R * S)
    bias = torch.randn(K, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = Fn.conv2d(xr, wr.flip(2, 3), stride=stride, padding=(ph, pw))
    ohw = None
    if border == "same":
        assert stride == (1, 1)
        y_ref = y_ref[:, :, :H, :W]
        ohw = (H, W)
    OH, OW = y_ref.shape[2:]
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)

    cp = 4 if first_layer else _up32(C)
    kp = _up32(K)
    s_pad = _up32(S * cp) // cp if first_layer else S
    xn, wn, dyn = _nhwc(x, cp), _krsc(w, kp, cp, s_pad), _nhwc(dy, kp)
    bn = torch.zeros(kp)
    bn[:K] = bias.float()
    bn = bn.cuda()
    kw = dict(stride=stride, pad=(ph, pw), s_real=S, ohw=ohw)
    geom = ops.conv_rect_geom(tuple(xn.shape), tuple(wn.shape), stride, (ph, pw), S, ohw)
    assert geom[12:] == (OH, OW), (geom, OH, OW)
    errs = {}

    def ref_nhwc(t, cpad):
        out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cpad, dtype=torch.float64)
        out[..., :t.shape[1]] = t.detach().permute(0, 2, 3, 1)
        return out

    # forward: plain, bias, bias + add, bias + add + ReLU
    yr = ref_nhwc(y_ref, kp)
    br = torch.zeros(kp, dtype=torch.float64)
    br[:K] = bias
    addn = torch.randn(N, OH, OW, kp, generator=g, dtype=torch.float64).float()
    y = ops.conv_rect_fwd(xn, wn, **kw)
    assert tuple(y.shape) == (N, OH, OW, kp)
    errs["fwd"] = _rel(y, yr)
    assert torch.all(y[..., K:] == 0)
    errs["fwd_bias"] = _rel(ops.conv_rect_fwd(xn, wn, bias=bn, **kw), yr + br)
    errs["fwd_add"] = _rel(ops.conv_rect_fwd(xn, wn, bias=bn, add=addn.cuda(), **kw), yr + br + addn.double())
    y4 = ops.conv_rect_fwd(xn, wn, bias=bn, add=addn.cuda(), relu=True, **kw)
    errs["fwd_relu"] = _rel(y4, torch.relu(yr + br + addn.double()))
    assert float(y4.min()) >= 0.0
    assert torch.equal(ops.conv_rect_fwd(xn, wn, bias=bn, add=addn.cuda(), relu=True, **kw), y4)

    # filter gradient (padding taps and channels: exact zeros)
    dwr = torch.zeros(kp, R, s_pad, cp, dtype=torch.float64)
    dwr[:K, :, :S, :C] = wr.grad.flip(2, 3).permute(0, 2, 3, 1)
    dw = ops.conv_rect_wgrad(xn, dyn, tuple(wn.shape), **kw)
    errs["wgrad"] = _rel(dw, dwr)
    assert torch.all(dw[:, :, S:, :] == 0) and torch.all(dw[K:] == 0) and torch.all(dw[..., C:] == 0)
    assert torch.equal(ops.conv_rect_wgrad(xn, dyn, tuple(wn.shape), **kw), dw)

    # data gradient, without and with `add` (the network input has none)
    if not first_layer:
        dxr = ref_nhwc(xr.grad, cp)
        dx = ops.conv_rect_dgrad(dyn, wn, tuple(xn.shape), **kw)
        errs["dgrad"] = _rel(dx, dxr)
        addx = torch.randn(N, H, W, cp, generator=g, dtype=torch.float64).float()
        dx2 = ops.conv_rect_dgrad(dyn, wn, tuple(xn.shape), add=addx.cuda(), **kw)
        errs["dgrad_add"] = _rel(dx2, dxr + addx.double())
        assert torch.equal(ops.conv_rect_dgrad(dyn, wn, tuple(xn.shape), add=addx.cuda(), **kw), dx2)
    print("N%d %dx%d C%d K%d %dx%d/%dx%d %s:" % (N, H, W, C, K, R, S, stride[0], stride[1], border),
          " ".join("%s %.2e" % kv for kv in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= BOUND}
    assert not bad, bad
    return errs


def _grid():
    cases = []
    for fi, (R, S) in enumerate(FILTERS):
        for si, stride in enumerate(STRIDES):
            for border in BORDERS:
                if border == "same" and stride != (1, 1):
                    continue
                cases.append((R, S, stride, border, (fi + si) % 2))
    return cases


@pytest.mark.parametrize("R,S,stride,border,which", _grid())
def test_rect_passes_vs_fp64(hip, R, S, stride, border, which):
    """maps that are no multiple of any tile (19 x 38, 9 x 13), logical 48 channels in physical 64"""
    N, H, W = (2, 19, 38) if which == 0 else (3, 9, 13)
    C, K = (48, 40) if which == 0 else (32, 48)
    _check_passes(N, H, W, C, K, R, S, stride, border, seed=1000 * R + 100 * S + 10 * stride[0] + stride[1])


@pytest.mark.parametrize("R,S,stride,border", [(3, 3, (1, 1), "half"), (1, 7, (1, 1), "half"), (7, 1, (2, 1), "half"),
                                               (3, 5, (1, 2), "full")])
def test_rect_realistic_size_vs_fp64(hip, R, S, stride, border):
    """N = 8, 64 x 64, C = 128, K = 96: reductions of 896 - 1920 terms (forward, data gradient) and 32768 pixels (filter gradient)"""
    _check_passes(8, 64, 64, 128, 96, R, S, stride, border, seed=7 * R + S)


@pytest.mark.parametrize("R,S", [(1, 7), (7, 1), (3, 5), (2, 3), (3, 3), (1, 3)])
@pytest.mark.parametrize("stride", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("border", ["half", "valid", "full"])
def test_rect_network_input_vs_fp64(hip, R, S, stride, border):
    """the 4-channel network input: 3 logical channels, the filter's S padded to a multiple of 8 taps, S_real = S"""
    _check_passes(2, 19, 38, 3, 40, R, S, stride, border, seed=31 * R + S + stride[0], first_layer=True)


def test_rect_network_input_same(hip):
    _check_passes(2, 13, 9, 3, 32, 2, 3, (1, 1), "same", seed=5, first_layer=True)


# ------------------------------------------------------------------------------------------------- two independent kernels, one answer
@pytest.mark.parametrize("k,stride,pad,ohw", [(3, 1, 1, None), (3, 2, 1, None), (1, 1, 0, None), (5, 1, 2, None), (2, 1, 1, "cut"),
                                              (4, 4, 0, None)])
def test_rect_agrees_with_square_direct_kernels(hip, k, stride, pad, ohw):
    N, H, W, C, K = 3, 20, 28, 64, 96
    g = torch.Generator(device="cpu").manual_seed(k * 10 + stride)
    ohw = (H, W) if ohw == "cut" else None
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, k, k, C, generator=g) / math.sqrt(C * k * k)).cuda()
    geom = ops.conv_geom(tuple(x.shape), tuple(w.shape), stride, pad, None, ohw)
    dy = torch.randn(N, geom[10], geom[11], K, generator=g).cuda()
    bias = torch.randn(K, generator=g).cuda()
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        y0 = ops.conv_fwd(x, w, bias=bias, stride=stride, pad=pad, ohw=ohw)
        dx0 = ops.conv_dgrad(dy, w, tuple(x.shape), stride=stride, pad=pad, ohw=ohw)
        dw0 = ops.conv_wgrad(x, dy, tuple(w.shape), stride=stride, pad=pad, ohw=ohw)
    kw = dict(stride=(stride, stride), pad=(pad, pad), ohw=ohw)
    y1 = ops.conv_rect_fwd(x, w, bias=bias, **kw)
    dx1 = ops.conv_rect_dgrad(dy, w, tuple(x.shape), **kw)
    dw1 = ops.conv_rect_wgrad(x, dy, tuple(w.shape), **kw)
    errs = (_rel(y1, y0), _rel(dx1, dx0), _rel(dw1, dw0))
    print("k%d/%d pad %d: fwd %.2e dgrad %.2e wgrad %.2e" % ((k, stride, pad) + errs))
    assert max(errs) <= BOUND


# ------------------------------------------------------------------------------------------------- refusals
def test_rect_refuses_other_strides(hip):
    """a stride that is no power of two is refused with a message naming it, and nothing is launched"""
    x = torch.zeros(2, 12, 12, 32, device="cuda")
    w = torch.zeros(32, 3, 1, 32, device="cuda")
    with ops.LaunchTrace() as trace:
        for stride, name in (((3, 1), "sh"), ((1, 3), "sw"), ((6, 2), "sh")):
            oh, ow = (12 + 2 - 3) // stride[0] + 1, (12 - 1) // stride[1] + 1
            dy = torch.zeros(2, oh, ow, 32, device="cuda")
            with pytest.raises(DenetHipError, match="stride %s must be a power of two" % name):
                ops.conv_rect_fwd(x, w, stride=stride, pad=(1, 0))
            with pytest.raises(DenetHipError, match="stride %s must be a power of two" % name):
                ops.conv_rect_dgrad(dy, w, tuple(x.shape), stride=stride, pad=(1, 0))
            with pytest.raises(DenetHipError, match="stride %s must be a power of two" % name):
                ops.conv_rect_wgrad(x, dy, tuple(w.shape), stride=stride, pad=(1, 0))
        # the data gradient of the 4-channel network input does not exist
        x4, w4 = torch.zeros(2, 12, 12, 4, device="cuda"), torch.zeros(32, 3, 8, 4, device="cuda")
        with pytest.raises(DenetHipError, match="physical C"):
            ops.conv_rect_dgrad(torch.zeros(2, 12, 12, 32, device="cuda"), w4, tuple(x4.shape), stride=(1, 1), pad=(1, 1), s_real=3)
        # an output larger than the padding gives
        with pytest.raises(DenetHipError, match="OH"):
            ops.check(ops._L().denet_conv_rect_fwd(x.data_ptr(), w.data_ptr(), None, None, x.data_ptr(), 0, 2, 12, 12, 32, 32, 3, 1, 1,
                                                   1, 1, 0, 0, 11, 12, ops.stream_ptr()), "conv_rect_fwd")
    assert trace.symbols == []


def test_rect_data_gradient_of_indivisible_map(hip):
    """the data gradient does not need H % sh == 0 or W % sw == 0 (the class grid is masked): 19 x 13 under (2, 4)"""
    _check_passes(2, 19, 13, 32, 32, 3, 5, (2, 4), "half", seed=77)


# ------------------------------------------------------------------------------------------------- a whole step of a mixed model
MIXED_DESC = "C.B[32,3] BN A C.X[64,1,7] BN A C.X[64,7,1,2,1] BN A DC.X[32,3,1,2,1] C.X[32,3,3,1,2] BN A R"
MIXED_MAPS = [(16, 24), (16, 24), (8, 24), (16, 24), (16, 12), (1, 1)]      # C.B, C.X 1x7, C.X 7x1/2x1, DC.X, C.X 3x3/1x2, the head


def _mixed_model(B, CLS, seed):
    m = build_model(MIXED_DESC, (3, 16, 24), B, CLS, seed=seed)
    m.class_labels = {"c%i" % i: i for i in range(CLS)}
    return m


def test_mixed_model_training_step_and_inference_vs_fp64(hip, tmp_path):
    """one sgd step of a model that mixes square, rectangular, per-axis strided and transposed convolutions: cost, every parameter
    gradient and every updated parameter against float64 (1e-3 max-norm), which kernels ran, then test-mode probabilities (batch
    norms folded into the rectangular forward kernel with bias and ReLU), and the save / reload / predict round trip"""
    B, CLS, LR, MOM, DECAY = 4, 10, 0.1, 0.9, 0.0005
    model = _mixed_model(B, CLS, seed=3)
    convs = [l for l in model.layers if l.type_name in ("conv", "deconv")]
    assert [l.output_shape[2:] for l in convs] == MIXED_MAPS
    assert [l.anisotropic for l in convs] == [False, True, True, True, True, True]
    assert convs[-1].filter_shape[2:] == (16, 12)
    model.build_train_func("sgd")
    rng = np.random.RandomState(11)
    x = rng.uniform(0.0, 1.0, (B, 3, 16, 24)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    metas = [{"image_class": int(c)} for c in cls]
    weights = set(id(p) for l in model.layers for p in l.weights())
    before = param_layers(model)
    values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}

    with KernelAudit(model) as audit:
        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
        torch.cuda.synchronize()
    for row in audit.table:
        print(row)
    rows = {r["layer"]: r for r in audit.table}
    conv_rows = [r for r in audit.table]
    assert len(conv_rows) == 5                        # the ConvLayers (the transposed layer is no ConvLayer)
    square, rect = conv_rows[0], conv_rows[1:]
    assert square["fwd"] and all(not s.startswith("conv_rect_kernel") for s in square["fwd"] + square["bwd"]), square
    for r in rect:
        assert len(r["fwd"]) == 1 and r["fwd"][0].startswith("conv_rect_kernel<0, "), r
        assert sorted(s[:19] for s in r["bwd"]) == ["conv_rect_kernel<1,", "conv_rect_kernel<2,"], r
    # the transposed layer's three launches are attributed to no ConvLayer
    assert sorted(s[:19] for s in audit.other if s.startswith("conv_rect")) == ["conv_rect_kernel<0,", "conv_rect_kernel<1,",
                                                                                  "conv_rect_kernel<2,"], audit.other

    relu_masks = relu_masks_of(model)
    params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
    flips, outs = {}, {}
    cost_ref, _, stats = reference(model, x, params, cls, True, relu_masks=relu_masks, flips=flips, outs=outs)
    cost_ref.backward()
    print("ReLU decisions that differ from float64 (layer: count):", {l.layer_index: flips[id(l)] for l in model.layers if flips.get(id(l))})
    print("cost", cost, float(cost_ref.detach()))
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach())), (cost, float(cost_ref.detach()))
    report, bad = [], []
    for l, p, e_g, e_p, g_dev, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
        i = l.layer_index
        if p is getattr(l, "beta", None) and l.type_name == "conv" and model.layers[i + 1].type_name == "batchnorm":
            # a bias in front of a batch norm: the normalisation removes it, its exact gradient is 0 (float64 leaves 1e-17)
            # and max|b| is no scale. The gradient is the column sum of dy: the error is taken against the largest
            # sum of |dy| over a channel, the magnitude those sums are formed from (an fp32 sum errs by eps times that)
            scale = float(outs[id(l)].grad.abs().sum(dim=(0, 2, 3)).max())
            v64 = torch.from_numpy(values[id(l)][1]).double()
            p_dev = torch.from_numpy(p.get_value().copy()).double()
            p_ref = v64 - LR * (g_ref + (DECAY if id(p) in weights else 0.0) * v64)
            e_g = float((g_dev - g_ref).abs().max()) / scale
            e_p = float(((p_dev - v64) - (p_ref - v64)).abs().max()) / (LR * scale)
            print("L%d bias in front of a batch norm: |grad| device %.2e float64 %.2e, sum|dy| %.2e" % (
                i, float(g_dev.abs().max()), float(g_ref.abs().max()), scale))
        report.append("L%d %s %s: grad %.2e, update %.2e" % (i, l.type_name, p.name, e_g, e_p))
        if not (e_g <= 1e-3 and e_p <= 1e-3):
            bad.append(report[-1])
    print("\n".join(report))
    assert not bad, bad

    running = {}
    for l in model.layers:
        if l.type_name == "batchnorm":
            rm, rs = torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double()
            m_ref = (1.0 - l.momentum) * stats[id(l)]["mean"]
            s_ref = l.momentum + (1.0 - l.momentum) * stats[id(l)]["stdinv"]
            assert _rel(rm, m_ref) <= 1e-3 and _rel(rs, s_ref) <= 1e-3, l.layer_index
            running[id(l)] = (rm, rs)

    # inference: the batch norms behind the rectangular layers are folded into conv_rect_fwd's epilogue
    assert ops.INFER_FOLD
    with KernelAudit(model) as audit:
        pr = model.predict_output_step(x)
        torch.cuda.synchronize()
    for r in audit.table[1:]:
        assert len(r["fwd"]) == 1 and r["fwd"][0].startswith("conv_rect_kernel<0, "), r
    now = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in before}
    with torch.no_grad():
        _, logits, _ = reference(model, x, now, cls, False, running=running)
    pr_ref = torch.softmax(logits, dim=1)
    assert pr.shape == (B, CLS)
    e_pr = float((torch.from_numpy(pr).double() - pr_ref).abs().max()) / float(pr_ref.max())
    print("test-mode probabilities: %.2e" % e_pr)
    assert e_pr <= 1e-3
    # unfolded inference agrees as well (separate batch-norm passes behind the rectangular kernel)
    with ops.infer_fold(False):
        pr_unfolded = model.predict_output_step(x)
    assert float((torch.from_numpy(pr_unfolded).double() - pr_ref).abs().max()) / float(pr_ref.max()) <= 1e-3

    path = str(tmp_path / "mixed.mdl.gz")
    model_cnn.save_to_file(model, path)
    again = model_cnn.load_from_file(path, B)
    assert [l.output_shape for l in again.layers] == [l.output_shape for l in model.layers]
    pr2 = again.predict_output_step(x)
    assert np.array_equal(pr2.view(np.int32), pr.view(np.int32))


def test_classifier_head_behind_non_square_map_trains(hip):
    """`C[32,3] R` on a 3 x 16 x 20 input: the head's whole-map `valid` convolution (16 x 20) runs the rectangular kernels"""
    B, CLS = 4, 6
    m = build_model("C[32,3] R", (3, 16, 20), B, CLS, seed=1)
    head = m.layers[2]
    assert head.filter_shape == (CLS, 32, 16, 20) and head.anisotropic and head.output_shape == (B, CLS, 1, 1)
    m.build_train_func("sgd")
    rng = np.random.RandomState(2)
    x = rng.uniform(0.0, 1.0, (B, 3, 16, 20)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    w0, w1 = [torch.from_numpy(l.omega.get_value().copy()).double().requires_grad_(True) for l in m.layers[1:3]]
    cost, _ = m.train_step(x, [{"image_class": int(c)} for c in cls], 0, 0, 0.1, [0.9], 0.0)
    cost_ref, _, _ = reference(m, x, {id(m.layers[1]): [w0], id(m.layers[2]): [w1]}, cls, True)
    cost_ref.backward()
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach()))
    for l, t in zip(m.layers[1:3], (w0, w1)):
        assert _rel(torch.from_numpy(l.omega.get_grad().copy()), t.grad) <= 1e-3
    pr = m.predict_output_step(x)
    assert pr.shape == (B, CLS) and np.allclose(pr.sum(axis=1), 1.0, atol=1e-5)
