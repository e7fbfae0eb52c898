"""Dilated convolutions (`C.D` / `C.DX`, dilated residual blocks; csrc/conv_rect.hip, conv_dil_kernel) on the device, against float64.

The contract is this build's own ("Dilated convolutions"; the reference has no such parameter): on the stored
correlation taps, y[n, oy, ox, k] = sum x[n, oy*sh - ph + r*dh, ox*sw - pw + s*dw, c] * w[k, r, s, c], zero outside the map. The
arbiter is PyTorch's CPU conv2d(..., dilation=) in float64 on the flipped reference filter, gradients by autograd. The border modes
act on the effective extent ke = (k - 1) * d + 1: `valid` 0, `half` ke // 2, `full` ke - 1, `same` ke // 2 with the output cut to
H x W (stride 1).

Bound of the kernel checks: max|a - b| / max|b| <= 1e-5, the figure tests/test_conv_rect_gpu.py holds the same kernel text to: the
dilated passes form the same sums over the same reduction lengths in the same FMA chain. Whole steps: 1e-3 max-norm, the project's
whole-step budget.

Shapes, chosen where the kernel can go wrong:
  A  2 x 7 x 9,   32 -> 32           126 output pixels at stride 1: one partial row tile (the rows that are none must stay outside
                                     the image whatever r * dh is added), tile <128, 32>, one filter-gradient slice
  B  3 x 11 x 13, 96 -> 64 physical  logical 80 -> 40: three chunks per tap, tiles <128, 64> and <64, 128>, three slices
  C  2 x 10 x 6,  64 -> 128          tile <128, 128>"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.lib import DenetHipError
from denet_amd.model import model_cnn
from denet_amd.model.audit import KernelAudit, conv_layers
from dilated_reference import block_exit_masks, build_model, param_layers, reference, rel as _rel, relu_masks_of, sgd_step_errors

pytestmark = pytest.mark.gpu

SHAPES = {"A": (2, 7, 9, 32, 32), "B": (3, 11, 13, 80, 40), "C": (2, 10, 6, 64, 128)}        # N, H, W, logical C, logical K
FILTERS = [(3, 3), (2, 3), (1, 5)]
DILATIONS = [(2, 2), (1, 2), (3, 1), (2, 3), (4, 4)]
BORDERS = ["valid", "half", "full", "same"]
BOUND = 1e-5


def _padding(border, keh, kew):
    return {"valid": (0, 0), "half": (keh // 2, kew // 2), "full": (keh - 1, kew - 1), "same": (keh // 2, kew // 2)}[border]


def _up32(v):
    return (v + 31) // 32 * 32


def _nhwc(t, cp):
    """[N, C, H, W] float64 -> the device's [N, H, W, cp] float32, padding channels zero"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cp, dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 1).float()
    return out.cuda()


def _krsc(w, kp, cp):
    """reference filters [K, C, R, S] -> the device's correlation taps [kp][R][S][cp], zero padded"""
    k, c, r, s = w.shape
    out = torch.zeros(kp, r, s, cp, dtype=torch.float32)
    out[:k, :, :, :c] = w.flip(2, 3).permute(0, 2, 3, 1).float()
    return out.cuda()


def _fits(H, W, R, S, dilation, border):
    keh, kew = (R - 1) * dilation[0] + 1, (S - 1) * dilation[1] + 1
    ph, pw = _padding(border, keh, kew)
    return keh <= H + 2 * ph and kew <= W + 2 * pw


def _check_passes(shape, R, S, stride, dilation, border, seed):
    """all three passes of one geometry against float64 (forward plain / bias / add / ReLU, filter gradient with exact zeros in
    the padding channels, data gradient without and with `add`), each repeated once for bit-equal reruns; returns the errors"""
    N, H, W, C, K = SHAPES[shape]
    keh, kew = (R - 1) * dilation[0] + 1, (S - 1) * dilation[1] + 1
    ph, pw = _padding(border, keh, kew)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, R, S, generator=g, dtype=torch.float64) / math.sqrt(C * R * S)
    bias = torch.randn(K, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = Fn.conv2d(xr, wr.flip(2, 3), stride=stride, padding=(ph, pw), dilation=dilation)
    ohw = None
    if border == "same":
        assert stride == (1, 1)
        y_ref = y_ref[:, :, :H, :W]
        ohw = (H, W)
    OH, OW = y_ref.shape[2:]
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)

    cp, kp = _up32(C), _up32(K)
    xn, wn, dyn = _nhwc(x, cp), _krsc(w, kp, cp), _nhwc(dy, kp)
    bn = torch.zeros(kp)
    bn[:K] = bias.float()
    bn = bn.cuda()
    kw = dict(stride=stride, pad=(ph, pw), dilation=dilation, ohw=ohw)
    geom = ops.conv_dil_geom(tuple(xn.shape), tuple(wn.shape), stride, (ph, pw), dilation, S, ohw)
    assert geom[14:] == (OH, OW), (geom, OH, OW)
    errs = {}

    def ref_nhwc(t, cpad):
        out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cpad, dtype=torch.float64)
        out[..., :t.shape[1]] = t.detach().permute(0, 2, 3, 1)
        return out

    yr = ref_nhwc(y_ref, kp)
    br = torch.zeros(kp, dtype=torch.float64)
    br[:K] = bias
    addn = torch.randn(N, OH, OW, kp, generator=g, dtype=torch.float64).float()
    y = ops.conv_dil_fwd(xn, wn, **kw)
    assert tuple(y.shape) == (N, OH, OW, kp)
    errs["fwd"] = _rel(y, yr)
    assert torch.all(y[..., K:] == 0)
    assert torch.equal(ops.conv_dil_fwd(xn, wn, **kw), y)
    errs["fwd_bias"] = _rel(ops.conv_dil_fwd(xn, wn, bias=bn, **kw), yr + br)
    errs["fwd_add"] = _rel(ops.conv_dil_fwd(xn, wn, bias=bn, add=addn.cuda(), **kw), yr + br + addn.double())
    y4 = ops.conv_dil_fwd(xn, wn, bias=bn, add=addn.cuda(), relu=True, **kw)
    errs["fwd_relu"] = _rel(y4, torch.relu(yr + br + addn.double()))
    assert float(y4.min()) >= 0.0
    assert torch.equal(ops.conv_dil_fwd(xn, wn, bias=bn, add=addn.cuda(), relu=True, **kw), y4)

    dwr = torch.zeros(kp, R, S, cp, dtype=torch.float64)
    dwr[:K, :, :, :C] = wr.grad.flip(2, 3).permute(0, 2, 3, 1)
    dw = ops.conv_dil_wgrad(xn, dyn, tuple(wn.shape), **kw)
    errs["wgrad"] = _rel(dw, dwr)
    assert torch.all(dw[K:] == 0) and torch.all(dw[..., C:] == 0)
    assert torch.equal(ops.conv_dil_wgrad(xn, dyn, tuple(wn.shape), **kw), dw)

    dxr = ref_nhwc(xr.grad, cp)
    dx = ops.conv_dil_dgrad(dyn, wn, tuple(xn.shape), **kw)
    errs["dgrad"] = _rel(dx, dxr)
    assert torch.equal(ops.conv_dil_dgrad(dyn, wn, tuple(xn.shape), **kw), dx)
    addx = torch.randn(N, H, W, cp, generator=g, dtype=torch.float64).float()
    dx2 = ops.conv_dil_dgrad(dyn, wn, tuple(xn.shape), add=addx.cuda(), **kw)
    errs["dgrad_add"] = _rel(dx2, dxr + addx.double())
    assert torch.equal(ops.conv_dil_dgrad(dyn, wn, tuple(xn.shape), add=addx.cuda(), **kw), dx2)
    print("%s %dx%d/%dx%d d%dx%d %s:" % ((shape, R, S) + tuple(stride) + tuple(dilation) + (border,)),
          " ".join("%s %.2e" % kv for kv in errs.items()))
    bad = {k: v for k, v in errs.items() if not v <= BOUND}
    assert not bad, bad
    return errs


def _refused(shape, R, S, stride, dilation, border):
    """ke larger than the padded map: refused with the cause named, nothing launched"""
    N, H, W, C, K = SHAPES[shape]
    ph, pw = _padding(border, (R - 1) * dilation[0] + 1, (S - 1) * dilation[1] + 1)
    x = torch.zeros(N, H, W, _up32(C), device="cuda")
    w = torch.zeros(_up32(K), R, S, _up32(C), device="cuda")
    with ops.LaunchTrace() as trace:
        with pytest.raises(ValueError, match="larger than the padded map"):
            ops.conv_dil_fwd(x, w, stride=stride, pad=(ph, pw), dilation=dilation)
    assert trace.symbols == []


def _grid():
    """every filter x dilation x border at stride 1, the shapes taking turns so that each shape meets each dilation and each
    border; then shape A (the partial row tile) with every dilation under `half` and `valid` - (4, 4) puts whole taps into the
    padding under `half` (ke = 9 > 7) and is refused under `valid`; then the strided axes a dilated layer may have"""
    cases = []
    names = sorted(SHAPES)
    for fi, (R, S) in enumerate(FILTERS):
        for di, dil in enumerate(DILATIONS):
            for bi, border in enumerate(BORDERS):
                cases.append((names[(fi + di + bi) % 3], R, S, (1, 1), dil, border))
    for dil in DILATIONS:
        for border in ("half", "valid"):
            case = ("A", 3, 3, (1, 1), dil, border)
            if case not in cases:
                cases.append(case)
    for name in names:
        for (R, S) in FILTERS:
            for border in ("valid", "half", "full"):
                cases.append((name, R, S, (2, 1), (1, 2), border))
                cases.append((name, R, S, (1, 2), (3, 1), border))
    return cases


@pytest.mark.parametrize("shape,R,S,stride,dilation,border", _grid())
def test_dilated_passes_vs_fp64(hip, shape, R, S, stride, dilation, border):
    N, H, W, C, K = SHAPES[shape]
    if not _fits(H, W, R, S, dilation, border):
        assert border == "valid"                      # every other mode pads by the extent
        _refused(shape, R, S, stride, dilation, border)
        return
    _check_passes(shape, R, S, stride, dilation, border,
                  seed=10000 * R + 1000 * S + 100 * dilation[0] + 10 * dilation[1] + stride[0] + BORDERS.index(border))


def test_grid_holds_the_named_cases():
    """the cases the kernel's hazards live in are in the grid: whole taps in the padding on the partial row tile, its refusal
    under `valid`, and both strided forms on every shape"""
    grid = _grid()
    assert ("A", 3, 3, (1, 1), (4, 4), "half") in grid and ("A", 3, 3, (1, 1), (4, 4), "valid") in grid
    assert _fits(7, 9, 3, 3, (4, 4), "half") and not _fits(7, 9, 3, 3, (4, 4), "valid")
    for name in SHAPES:
        assert {d for s, _, _, _, d, _ in grid if s == name} == set(DILATIONS)
        assert {b for s, _, _, _, _, b in grid if s == name} == set(BORDERS)
        assert {st for s, _, _, st, _, _ in grid if s == name} == {(1, 1), (2, 1), (1, 2)}


# ------------------------------------------------------------------------------------------------- dilation (1, 1) is the rectangular kernel
@pytest.mark.parametrize("stride", [(2, 1), (1, 1)])
def test_dilation_one_equals_the_rectangular_kernel_bit_for_bit(hip, stride):
    N, H, W, C, K = 3, 11, 13, 96, 64
    g = torch.Generator(device="cpu").manual_seed(7 + stride[0])
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, 3, 3, C, generator=g) / math.sqrt(9 * C)).cuda()
    bias = torch.randn(K, generator=g).cuda()
    geom = ops.conv_rect_geom(tuple(x.shape), tuple(w.shape), stride, (1, 1))
    dy = torch.randn(N, geom[12], geom[13], K, generator=g).cuda()
    addy = torch.randn(N, geom[12], geom[13], K, generator=g).cuda()
    addx = torch.randn(N, H, W, C, generator=g).cuda()
    kw = dict(stride=stride, pad=(1, 1))
    assert ops.conv_dil_geom(tuple(x.shape), tuple(w.shape), stride, (1, 1), (1, 1))[14:] == geom[12:]
    with ops.LaunchTrace() as trace:
        y1 = ops.conv_dil_fwd(x, w, bias=bias, add=addy, relu=True, dilation=(1, 1), **kw)
        dx1 = ops.conv_dil_dgrad(dy, w, tuple(x.shape), add=addx, dilation=(1, 1), **kw)
        dw1 = ops.conv_dil_wgrad(x, dy, tuple(w.shape), dilation=(1, 1), **kw)
    assert [s[:18] for s in trace.symbols] == ["conv_dil_kernel<0,", "conv_dil_kernel<1,", "conv_dil_kernel<2,"], trace.symbols
    y0 = ops.conv_rect_fwd(x, w, bias=bias, add=addy, relu=True, **kw)
    dx0 = ops.conv_rect_dgrad(dy, w, tuple(x.shape), add=addx, **kw)
    dw0 = ops.conv_rect_wgrad(x, dy, tuple(w.shape), **kw)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and torch.equal(dw1, dw0)


# ------------------------------------------------------------------------------------------------- two kernels, one answer
def test_dilated_kernel_agrees_with_the_rectangular_kernel_on_the_stuffed_filter(hip):
    """dilation (2, 3): a 3x3 filter on the dilated kernel against conv_rect_* on the zero-stuffed 5x7 filter, same padding"""
    N, H, W, C, K = 3, 11, 13, 96, 64
    dh, dw_ = 2, 3
    g = torch.Generator(device="cpu").manual_seed(23)
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, 3, 3, C, generator=g) / math.sqrt(9 * C)).cuda()
    stuffed = torch.zeros(K, 5, 7, C, device="cuda")
    stuffed[:, ::dh, ::dw_, :] = w
    pad = (2, 3)
    geom = ops.conv_dil_geom(tuple(x.shape), tuple(w.shape), (1, 1), pad, (dh, dw_))
    assert geom[14:] == (H, W) == ops.conv_rect_geom(tuple(x.shape), tuple(stuffed.shape), (1, 1), pad)[12:]
    dy = torch.randn(N, H, W, K, generator=g).cuda()
    y1 = ops.conv_dil_fwd(x, w, stride=(1, 1), pad=pad, dilation=(dh, dw_))
    dx1 = ops.conv_dil_dgrad(dy, w, tuple(x.shape), stride=(1, 1), pad=pad, dilation=(dh, dw_))
    dw1 = ops.conv_dil_wgrad(x, dy, tuple(w.shape), stride=(1, 1), pad=pad, dilation=(dh, dw_))
    y0 = ops.conv_rect_fwd(x, stuffed, stride=(1, 1), pad=pad)
    dx0 = ops.conv_rect_dgrad(dy, stuffed, tuple(x.shape), stride=(1, 1), pad=pad)
    dw0 = ops.conv_rect_wgrad(x, dy, tuple(stuffed.shape), stride=(1, 1), pad=pad)[:, ::dh, ::dw_, :]      # the real taps
    errs = (_rel(y1, y0), _rel(dx1, dx0), _rel(dw1, dw0))
    print("fwd %.2e dgrad %.2e wgrad %.2e" % errs)
    assert max(errs) <= BOUND


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(hip):
    x = torch.zeros(2, 12, 12, 32, device="cuda")
    w = torch.zeros(32, 3, 3, 32, device="cuda")
    x4, w4 = torch.zeros(2, 12, 12, 4, device="cuda"), torch.zeros(32, 3, 8, 4, device="cuda")
    with ops.LaunchTrace() as trace:
        for dil, stride, name in (((0, 1), (1, 1), "dh"), ((1, -1), (1, 1), "dw"), ((2, 1), (2, 1), "sh"), ((1, 2), (1, 2), "sw")):
            keh, kew = 2 * dil[0] + 1, 2 * dil[1] + 1
            oh, ow = (12 + 4 - keh) // stride[0] + 1, (12 + 4 - kew) // stride[1] + 1
            dy = torch.zeros(2, oh, ow, 32, device="cuda")
            kw = dict(stride=stride, pad=(2, 2), dilation=dil)
            with pytest.raises(DenetHipError, match=name):
                ops.conv_dil_fwd(x, w, **kw)
            with pytest.raises(DenetHipError, match=name):
                ops.conv_dil_dgrad(dy, w, tuple(x.shape), **kw)
            with pytest.raises(DenetHipError, match=name):
                ops.conv_dil_wgrad(x, dy, tuple(w.shape), **kw)
        # a dilated filter on the 4-channel network input
        with pytest.raises(DenetHipError, match="physical C"):
            ops.conv_dil_fwd(x4, w4, stride=(1, 1), pad=(2, 2), dilation=(2, 2), s_real=3)
        with pytest.raises(DenetHipError, match="physical C"):
            ops.conv_dil_wgrad(x4, torch.zeros(2, 12, 12, 32, device="cuda"), tuple(w4.shape), stride=(1, 1), pad=(2, 2), dilation=(2, 2),
                               s_real=3)
        # the effective extent beyond the padded map
        with pytest.raises(ValueError, match="larger than the padded map"):
            ops.conv_dil_fwd(x, w, stride=(1, 1), pad=(0, 0), dilation=(6, 6))
        # an output larger than the extent allows: ke = 5, 12 + 2 - 5 + 1 = 10 rows
        with pytest.raises(DenetHipError, match="OH"):
            ops.check(ops._L().denet_conv_dil_fwd(x.data_ptr(), w.data_ptr(), None, None, x.data_ptr(), 0, 2, 12, 12, 32, 32, 3, 3, 3,
                                                  1, 1, 1, 1, 2, 2, 11, 10, ops.stream_ptr()), "conv_dil_fwd")
    assert trace.symbols == []


# ------------------------------------------------------------------------------------------------- a whole step of a dilated model
DESC = "C.B[32,3] BN A C.D[32,3,1,2] BN A nRSN.O[1,32,3,1,0,2] C.DX[64,3,3,1,1,1,2] BN A R"
DILATED_ROWS = ["4.conv", "7.resnet.0", "7.resnet.1", "8.conv"]


def _model(B, CLS, seed):
    m = build_model(DESC, (3, 12, 16), B, CLS, seed=seed, head_scale=0.05)
    m.class_labels = {"c%i" % i: i for i in range(CLS)}
    return m


def _assert_dilated_rows(audit, training):
    rows = {r["layer"]: r for r in audit.table}
    assert set(DILATED_ROWS) <= set(rows), sorted(rows)
    for name in DILATED_ROWS:
        r = rows[name]
        assert r["geometry"].split()[-1] in ("d2x2", "d1x2"), r
        assert len(r["fwd"]) == 1 and r["fwd"][0].startswith("conv_dil_kernel<0, "), r
        if training:
            assert sorted(s[:18] for s in r["bwd"]) == ["conv_dil_kernel<1,", "conv_dil_kernel<2,"], r
    stem = audit.table[0]
    assert stem["layer"] == "1.conv" and stem["fwd"]
    assert all(not s.startswith(("conv_dil", "conv_rect")) for s in stem["fwd"] + stem["bwd"]), stem
    return rows


def test_dilated_model_training_step_and_inference_vs_fp64(hip, tmp_path):
    """one sgd step of a model with a `C.D` layer, a dilated residual block and a `C.DX` layer dilated along one axis: cost, every
    parameter gradient and every updated parameter against float64 (1e-3 max-norm, the ReLU decisions taken from the device),
    which kernels ran, then test-mode probabilities folded and unfolded, the save / reload / predict round trip, and the same step
    under bf16 training, where the dilated layers stay on the fp32 kernel"""
    B, CLS, LR, MOM, DECAY = 4, 10, 0.1, 0.9, 0.0005
    model = _model(B, CLS, seed=3)
    assert [name for name, l in conv_layers(model) if l.dilated] == DILATED_ROWS
    assert [l.dilation for _, l in conv_layers(model)] == [(1, 1), (2, 2), (2, 2), (2, 2), (1, 2), (1, 1)]
    assert all(l.output_shape[2:] == (12, 16) for _, l in conv_layers(model)[:-1])
    model.build_train_func("sgd")
    rng = np.random.RandomState(11)
    x = rng.uniform(0.0, 1.0, (B, 3, 12, 16)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    metas = [{"image_class": int(c)} for c in cls]
    weights = set(id(p) for l in model_cnn.walk_layers(model.layers) for p in l.weights())
    before = param_layers(model)
    values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}

    with KernelAudit(model) as audit:
        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
        torch.cuda.synchronize()
    for row in audit.table:
        print(row)
    _assert_dilated_rows(audit, True)

    relu_masks = relu_masks_of(model)
    relu_masks.update(block_exit_masks(model))
    params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
    flips, outs = {}, {}
    cost_ref, _, stats = reference(model, x, params, cls, True, relu_masks=relu_masks, flips=flips, outs=outs)
    cost_ref.backward()
    print("ReLU decisions that differ from float64:", {k: v for k, v in flips.items() if v})
    print("cost", cost, float(cost_ref.detach()))
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach())), (cost, float(cost_ref.detach()))
    report, bad = [], []
    for l, p, e_g, e_p, g_dev, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
        i = l.layer_index
        if p is getattr(l, "beta", None) and l.type_name == "conv":
            # the stem's bias in front of a batch norm: the normalisation removes it, its exact gradient is 0 (float64 leaves
            # 1e-17) and max|b| is no scale. The gradient is the column sum of dy: the error is taken against the largest sum of
            # |dy| over a channel, the magnitude those sums are formed from (tests/test_conv_rect_gpu.py does the same)
            assert model.layers[i + 1].type_name == "batchnorm"
            scale = float(outs[id(l)].grad.abs().sum(dim=(0, 2, 3)).max())
            v64 = torch.from_numpy(values[id(l)][1]).double()
            p_dev = torch.from_numpy(p.get_value().copy()).double()
            p_ref = v64 - LR * (g_ref + (DECAY if id(p) in weights else 0.0) * v64)
            e_g = float((g_dev - g_ref).abs().max()) / scale
            e_p = float(((p_dev - v64) - (p_ref - v64)).abs().max()) / (LR * scale)
        report.append("L%d %s %s: grad %.2e, update %.2e" % (i, l.type_name, p.name, e_g, e_p))
        if not (e_g <= 1e-3 and e_p <= 1e-3):
            bad.append(report[-1])
    print("\n".join(report))
    assert not bad, bad

    running = {}
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name == "batchnorm":
            rm, rs = torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double()
            m_ref = (1.0 - l.momentum) * stats[id(l)]["mean"]
            s_ref = l.momentum + (1.0 - l.momentum) * stats[id(l)]["stdinv"]
            assert _rel(rm, m_ref) <= 1e-3 and _rel(rs, s_ref) <= 1e-3, l.layer_index
            running[id(l)] = (rm, rs)

    # inference: the batch norms behind the dilated layers are folded into conv_dil_fwd's epilogue
    assert ops.INFER_FOLD
    with KernelAudit(model) as audit:
        pr = model.predict_output_step(x)
        torch.cuda.synchronize()
    _assert_dilated_rows(audit, False)
    now = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in before}
    with torch.no_grad():
        _, logits, _ = reference(model, x, now, cls, False, running=running)
    pr_ref = torch.softmax(logits, dim=1)
    assert pr.shape == (B, CLS)
    e_pr = float((torch.from_numpy(pr).double() - pr_ref).abs().max()) / float(pr_ref.max())
    print("test-mode probabilities: %.2e (largest %.3f)" % (e_pr, float(pr_ref.max())))
    assert e_pr <= 1e-3
    with ops.infer_fold(False):
        with KernelAudit(model) as audit:
            pr_unfolded = model.predict_output_step(x)
            torch.cuda.synchronize()
    _assert_dilated_rows(audit, False)
    assert float((torch.from_numpy(pr_unfolded).double() - pr_ref).abs().max()) / float(pr_ref.max()) <= 1e-3

    path = str(tmp_path / "dilated.mdl.gz")
    model_cnn.save_to_file(model, path)
    again = model_cnn.load_from_file(path, B)
    assert [l.output_shape for l in again.layers] == [l.output_shape for l in model.layers]
    assert [l.dilation for _, l in conv_layers(again)] == [l.dilation for _, l in conv_layers(model)]
    # as loaded, a model runs the `BN A` pairs inside an `original` block apart (ModelCNN.build_train_func is what counts the
    # readers and lets the fold take the activation in; every model with such blocks, dilated or not): the same function by
    # another rounding, so it is held to float64 here; once both models are prepared alike, the bits are the same
    pr_loaded = again.predict_output_step(x)
    assert float((torch.from_numpy(pr_loaded).double() - pr_ref).abs().max()) / float(pr_ref.max()) <= 1e-3
    prepared = model_cnn.load_from_file(path, B)
    prepared.build_train_func("sgd")                  # (before its first pass: a block keeps the plan its first inference pass made)
    pr2 = prepared.predict_output_step(x)
    assert np.array_equal(pr2.view(np.int32), pr.view(np.int32))

    # bf16 training moves the eligible square layers only: the dilated ones run conv_dil_kernel (fp32) in every pass
    with ops.train_precision("bf16"):
        m16 = _model(B, CLS, seed=3)
        m16.build_train_func("sgd")
        with KernelAudit(m16) as audit:
            cost16, _ = m16.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
            torch.cuda.synchronize()
    rows = _assert_dilated_rows(audit, True)
    assert all("bf16" not in s for name in DILATED_ROWS for s in rows[name]["fwd"] + rows[name]["bwd"])
    assert abs(cost16 - cost) <= 1e-3 * abs(cost), (cost16, cost)      # no layer of this model is eligible: the same fp32 step
