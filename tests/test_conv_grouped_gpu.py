"""Grouped convolutions (`C.G` / `C.GX`, grouped residual blocks; csrc/conv_rect.hip, conv_grp_kernel) on the device.

The contract is this build's own ("Grouped convolutions"; the reference has no groups): g groups on C -> K channels,
Cg = C / g, Kg = K / g, output channel k reads the input channels of group k // Kg only; the device filter is [K][R][S][Cg]
correlation taps. The arbiter is PyTorch's CPU conv2d(..., groups=g) in float64 on the flipped reference filter, gradients by
autograd; a whole model runs dilated_reference.reference on the dense twin of every grouped filter (grouped_reference.py).

Bound of the kernel checks: max|a - b| / max|b| <= 1e-5, the figure tests/test_conv_dilated_gpu.py and tests/test_conv_rect_gpu.py
hold the same kernel text to: the same fp32 FMA chains over reductions that are no longer (a window sums R*S*Cw terms, a slab the
same terms plus exact zeros). Whole steps: 1e-3 max-norm, the project's whole-step budget.

Shapes (N, H, W, C, K, g), chosen where the kernel can go wrong:
  window path  (2, 7, 9, 64, 64, 2)      Cw = Kw = 32, two windows, one partial row tile, tile <128, 32>
               (2, 7, 9, 64, 128, 2)     Kw = 64 != Cw: tiles <128, 64> forward, <128, 32> data gradient, <64, 128> filter gradient
               (3, 11, 13, 192, 192, 2)  Cw = 96: three chunks per tap, tiles <128, 128>, four row tiles, three slices
  slab path    (2, 7, 9, 64, 64, 4)      Cg = 16        (2, 7, 9, 64, 64, 16)    Cg = 4
               (2, 10, 6, 96, 96, 12)    Cg = 8, three slabs
               (2, 7, 9, 64, 64, 64)     depthwise      (2, 10, 6, 32, 32, 32)   depthwise on one slab"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.lib import DenetHipError
from denet_amd.model import model_cnn, zoo
from denet_amd.model.audit import KernelAudit, conv_layers
from dilated_reference import block_exit_masks, build_model, param_layers, reference, rel as _rel, relu_masks_of, sgd_step_errors
from grouped_reference import compact_ref, expand_ref

pytestmark = pytest.mark.gpu

NAMED = [(2, 7, 9, 64, 64, 2), (2, 7, 9, 64, 128, 2), (3, 11, 13, 192, 192, 2), (2, 7, 9, 64, 64, 4), (2, 7, 9, 64, 64, 16),
         (2, 10, 6, 96, 96, 12), (2, 7, 9, 64, 64, 64), (2, 10, 6, 32, 32, 32)]
FILTERS = [(3, 3), (1, 1), (2, 3), (1, 5)]
STRIDES = [(1, 1), (2, 2), (2, 1)]
BORDERS = ["valid", "half", "full", "same"]
BOUND = 1e-5
WORST = {}


def _padding(border, r, s):
    return {"valid": (0, 0), "half": (r // 2, s // 2), "full": (r - 1, s - 1), "same": (r // 2, s // 2)}[border]


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def _krsc(w):
    """reference filters [K, Cg, R, S] -> the device's correlation taps [K][R][S][Cg]"""
    return w.detach().flip(2, 3).permute(0, 2, 3, 1).contiguous()


def _check_passes(case, R, S, stride, border, seed):
    """all three passes of one geometry against float64: forward plain / bias / add / ReLU, filter gradient, data gradient without
    and with `add`, each repeated once for bit-equal reruns; returns the errors"""
    N, H, W, C, K, groups = case
    Cg = C // groups
    ph, pw = _padding(border, R, S)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, Cg, R, S, generator=g, dtype=torch.float64) / math.sqrt(Cg * R * S)
    bias = torch.randn(K, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = Fn.conv2d(xr, wr.flip(2, 3), stride=stride, padding=(ph, pw), groups=groups)
    ohw = None
    if border == "same":
        assert stride == (1, 1)
        y_ref = y_ref[:, :, :H, :W]
        ohw = (H, W)
    OH, OW = y_ref.shape[2:]
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)

    xn, wn, dyn, bn = _nhwc(x).float().cuda(), _krsc(w).float().cuda(), _nhwc(dy).float().cuda(), bias.float().cuda()
    assert tuple(wn.shape) == (K, R, S, Cg)
    kw = dict(stride=stride, pad=(ph, pw), ohw=ohw)
    geom, slab = ops.conv_grp_geom(tuple(xn.shape), tuple(wn.shape), groups, stride, (ph, pw), S, ohw)
    assert geom[14:] == (OH, OW), (geom, OH, OW)
    assert slab == (Cg if Cg < 32 else 0)
    errs = {}
    yr, br = _nhwc(y_ref), bias
    addn = torch.randn(N, OH, OW, K, generator=g, dtype=torch.float64).float()
    with ops.LaunchTrace() as trace:
        y = ops.conv_grp_fwd(xn, wn, groups, **kw)
    assert [s for s in trace.symbols if s.startswith("conv_")][0].startswith("conv_grp_kernel<0, "), trace.symbols
    assert tuple(y.shape) == (N, OH, OW, K)
    errs["fwd"] = _rel(y, yr)
    assert torch.equal(ops.conv_grp_fwd(xn, wn, groups, **kw), y)
    errs["fwd_bias"] = _rel(ops.conv_grp_fwd(xn, wn, groups, bias=bn, **kw), yr + br)
    errs["fwd_add"] = _rel(ops.conv_grp_fwd(xn, wn, groups, bias=bn, add=addn.cuda(), **kw), yr + br + addn.double())
    y4 = ops.conv_grp_fwd(xn, wn, groups, bias=bn, add=addn.cuda(), relu=True, **kw)
    errs["fwd_relu"] = _rel(y4, torch.relu(yr + br + addn.double()))
    assert float(y4.min()) >= 0.0
    assert torch.equal(ops.conv_grp_fwd(xn, wn, groups, bias=bn, add=addn.cuda(), relu=True, **kw), y4)

    dw = ops.conv_grp_wgrad(xn, dyn, tuple(wn.shape), groups, **kw)
    assert tuple(dw.shape) == (K, R, S, Cg)
    errs["wgrad"] = _rel(dw, _krsc(wr.grad))
    assert torch.equal(ops.conv_grp_wgrad(xn, dyn, tuple(wn.shape), groups, **kw), dw)

    dxr = _nhwc(xr.grad)
    dx = ops.conv_grp_dgrad(dyn, wn, tuple(xn.shape), groups, **kw)
    errs["dgrad"] = _rel(dx, dxr)
    assert torch.equal(ops.conv_grp_dgrad(dyn, wn, tuple(xn.shape), groups, **kw), dx)
    addx = torch.randn(N, H, W, C, generator=g, dtype=torch.float64).float()
    dx2 = ops.conv_grp_dgrad(dyn, wn, tuple(xn.shape), groups, add=addx.cuda(), **kw)
    errs["dgrad_add"] = _rel(dx2, dxr + addx.double())
    print("%s %dx%d/%dx%d %s:" % ((case, R, S) + tuple(stride) + (border,)), " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, v in errs.items():
        WORST[k.split("_")[0]] = max(WORST.get(k.split("_")[0], 0.0), v)
    bad = {k: v for k, v in errs.items() if not v <= BOUND}
    assert not bad, bad
    return errs


def _grid():
    """every named shape x every filter at each stride, the borders taking turns so that each shape meets each border and each
    filter meets each border at each stride; then the first window shape and the first slab shape under every border with the
    3x3 filter at stride 1"""
    cases = []
    for ci, case in enumerate(NAMED):
        for fi, (R, S) in enumerate(FILTERS):
            cases.append((case, R, S, (1, 1), BORDERS[(ci + fi) % 4]))
            cases.append((case, R, S, (2, 2), BORDERS[(ci + fi) % 3]))
            cases.append((case, R, S, (2, 1), BORDERS[(ci + fi + 1) % 3]))
    for case in (NAMED[0], NAMED[3]):
        for border in BORDERS:
            if (case, 3, 3, (1, 1), border) not in cases:
                cases.append((case, 3, 3, (1, 1), border))
    return cases


@pytest.mark.parametrize("case,R,S,stride,border", _grid())
def test_grouped_passes_vs_fp64(hip, case, R, S, stride, border):
    _check_passes(case, R, S, stride, border,
                  seed=100000 * NAMED.index(case) + 1000 * R + 100 * S + 10 * stride[0] + stride[1] + BORDERS.index(border))
    print("largest error per pass so far:", " ".join("%s %.2e" % kv for kv in sorted(WORST.items())))


def test_grid_holds_the_named_cases():
    grid = _grid()
    assert 96 <= len(grid) <= 120
    for case in NAMED:
        mine = [c for c in grid if c[0] == case]
        assert {(r, s) for _, r, s, _, _ in mine} == set(FILTERS)
        assert {st for _, _, _, st, _ in mine} == set(STRIDES)
        assert {b for _, _, _, _, b in mine} == set(BORDERS)
        assert all(st == (1, 1) for _, _, _, st, b in mine if b == "same")
    # both paths, every slab size, Kw != Cw, three chunks per tap
    wins = [ops.conv_grp_window(c[3], c[4], c[5]) for c in NAMED]
    assert wins == [(32, 32, 0), (32, 64, 0), (96, 96, 0), (32, 32, 16), (32, 32, 4), (32, 32, 8), (32, 32, 1), (32, 32, 1)]
    assert ops.conv_grp_window(64, 64, 32) == (32, 32, 2)          # (Cg = 2: in the expand / compact test)


# ------------------------------------------------------------------------------------------------- exact comparisons
def _tensors(N, H, W, C, K, Cg, R, S, stride, pad, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, R, S, Cg, generator=g) / math.sqrt(R * S * Cg)).cuda()
    bias = torch.randn(K, generator=g).cuda()
    OH, OW = (H + 2 * pad[0] - R) // stride[0] + 1, (W + 2 * pad[1] - S) // stride[1] + 1
    dy = torch.randn(N, OH, OW, K, generator=g).cuda()
    addy = torch.randn(N, OH, OW, K, generator=g).cuda()
    addx = torch.randn(N, H, W, C, generator=g).cuda()
    return x, w, bias, dy, addy, addx


@pytest.mark.parametrize("stride", [(1, 1), (2, 1)])
def test_one_window_equals_the_rectangular_kernel_bit_for_bit(hip, stride):
    N, H, W, C, K = 3, 11, 13, 96, 64
    x, w, bias, dy, addy, addx = _tensors(N, H, W, C, K, C, 3, 3, stride, (1, 1), 7 + stride[0])
    kw = dict(stride=stride, pad=(1, 1))
    g, slab = ops.conv_grp_geom(tuple(x.shape), tuple(w.shape), 1, stride, (1, 1))
    assert g[5:7] == (C, K) and slab == 0
    with ops.LaunchTrace() as trace:
        y1 = ops.conv_grp_fwd(x, w, 1, bias=bias, add=addy, relu=True, **kw)
        dx1 = ops.conv_grp_dgrad(dy, w, tuple(x.shape), 1, add=addx, **kw)
        dw1 = ops.conv_grp_wgrad(x, dy, tuple(w.shape), 1, **kw)
    assert [s[:18] for s in trace.symbols if s.startswith("conv_grp")] == ["conv_grp_kernel<0,", "conv_grp_kernel<1,",
                                                                            "conv_grp_kernel<2,"], trace.symbols
    y0 = ops.conv_rect_fwd(x, w, bias=bias, add=addy, relu=True, **kw)
    dx0 = ops.conv_rect_dgrad(dy, w, tuple(x.shape), add=addx, **kw)
    dw0 = ops.conv_rect_wgrad(x, dy, tuple(w.shape), **kw)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0) and torch.equal(dw1, dw0)


@pytest.mark.parametrize("case,stride", [((3, 11, 13, 192, 192, 2), (1, 1)), ((2, 7, 9, 64, 128, 2), (2, 1)),
                                         ((3, 11, 13, 96, 192, 3), (2, 2))])
def test_each_window_equals_the_rectangular_kernel_on_its_slices(hip, case, stride):
    """window path: group i of each pass is ops.conv_rect_* on contiguous copies of that group's slices, bit for bit (the tile is
    chosen from the window's counts, so the sums run in the same order)"""
    N, H, W, C, K, groups = case
    Cg, Kg = C // groups, K // groups
    x, w, bias, dy, addy, addx = _tensors(N, H, W, C, K, Cg, 3, 3, stride, (1, 1), 31 + groups)
    kw = dict(stride=stride, pad=(1, 1))
    y = ops.conv_grp_fwd(x, w, groups, bias=bias, add=addy, relu=True, **kw)
    dx = ops.conv_grp_dgrad(dy, w, tuple(x.shape), groups, add=addx, **kw)
    dw = ops.conv_grp_wgrad(x, dy, tuple(w.shape), groups, **kw)
    for i in range(groups):
        cs, ks = slice(i * Cg, (i + 1) * Cg), slice(i * Kg, (i + 1) * Kg)
        xi, wi, dyi = x[..., cs].contiguous(), w[ks].contiguous(), dy[..., ks].contiguous()
        yi = ops.conv_rect_fwd(xi, wi, bias=bias[ks].contiguous(), add=addy[..., ks].contiguous(), relu=True, **kw)
        dxi = ops.conv_rect_dgrad(dyi, wi, tuple(xi.shape), add=addx[..., cs].contiguous(), **kw)
        dwi = ops.conv_rect_wgrad(xi, dyi, tuple(wi.shape), **kw)
        assert torch.equal(y[..., ks], yi), i
        assert torch.equal(dx[..., cs], dxi), i
        assert torch.equal(dw[ks], dwi), i


@pytest.mark.parametrize("Cg", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("K,R,S", [(32, 3, 3), (96, 1, 5), (96, 2, 3)])
def test_expand_and_compact_equal_their_numpy_statements(hip, Cg, K, R, S):
    rng = np.random.RandomState(100 * Cg + K + R)
    w = rng.standard_normal((K, R, S, Cg)).astype(np.float32)
    want = np.zeros((K, R, S, 32), np.float32)
    for k in range(K):
        for j in range(32):
            if j // Cg == (k % 32) // Cg:
                want[k, :, :, j] = w[k, :, :, j % Cg]
    wd = torch.full((K, R, S, 32), 7.0, device="cuda")
    ops.conv_grp_expand(torch.from_numpy(w).cuda(), Cg, out=wd)
    assert np.array_equal(wd.cpu().numpy().view(np.int32), want.view(np.int32))
    dwd = rng.standard_normal((K, R, S, 32)).astype(np.float32)
    back = np.zeros((K, R, S, Cg), np.float32)
    for k in range(K):
        for c in range(Cg):
            back[k, :, :, c] = dwd[k, :, :, ((k % 32) // Cg) * Cg + c]
    dw = ops.conv_grp_compact(torch.from_numpy(dwd).cuda(), Cg)
    assert np.array_equal(dw.cpu().numpy().view(np.int32), back.view(np.int32))
    assert np.array_equal(ops.conv_grp_compact(wd, Cg).cpu().numpy(), w)             # compact undoes expand


@pytest.mark.parametrize("case", [(4, 12, 12, 64, 64, 16), (4, 12, 12, 128, 128, 2)])
def test_filter_gradient_is_bit_identical_from_run_to_run(hip, case):
    """once on the slab path and once on the window path, both with the pixel reduction in slices"""
    N, H, W, C, K, groups = case
    Cg = C // groups
    x, w, bias, dy, addy, addx = _tensors(N, H, W, C, K, Cg, 3, 3, (1, 1), (1, 1), 5)
    g, slab = ops.conv_grp_geom(tuple(x.shape), tuple(w.shape), groups, (1, 1), (1, 1))
    assert ops._L().denet_conv_grp_wgrad_workspace_bytes(N, C, K, g[5], g[6], 3, 3, H, W) > 0        # slices in use
    assert bool(slab) == (Cg < 32)
    a = ops.conv_grp_wgrad(x, dy, tuple(w.shape), groups, stride=(1, 1), pad=(1, 1)).clone()
    ops.WS.get("wgrad_rect", 1).fill_(0x5A)                                                           # (what the slices held is gone)
    b = ops.conv_grp_wgrad(x, dy, tuple(w.shape), groups, stride=(1, 1), pad=(1, 1))
    assert torch.equal(a, b) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(hip):
    x = torch.zeros(2, 12, 12, 64, device="cuda")
    y = torch.full((2, 12, 12, 64), 7.0, device="cuda")
    dy = torch.zeros(2, 12, 12, 64, device="cuda")
    with ops.LaunchTrace() as trace:
        for groups, cg, exc, match in ((3, 21, ValueError, "does not divide"), (0, 64, ValueError, "integer >= 1"),
                                       (2.0, 32, ValueError, "integer >= 1")):
            w = torch.zeros(64, 3, 3, cg, device="cuda")
            with pytest.raises(exc, match=match):
                ops.conv_grp_fwd(x, w, groups, pad=(1, 1), out=y)
        x96, w24 = torch.zeros(2, 12, 12, 96, device="cuda"), torch.zeros(96, 3, 3, 24, device="cuda")
        with pytest.raises(ValueError, match="unsupported group size"):
            ops.conv_grp_fwd(x96, w24, 4, pad=(1, 1))
        with pytest.raises(ValueError, match="unsupported group size"):                       # a depthwise multiplier
            ops.conv_grp_wgrad(x, torch.zeros(2, 12, 12, 128, device="cuda"), (128, 3, 3, 1), 64, pad=(1, 1))
        w = torch.zeros(64, 3, 3, 16, device="cuda")
        dy3 = torch.zeros(2, 4, 12, 64, device="cuda")
        kw = dict(stride=(3, 1), pad=(1, 1))
        with pytest.raises(DenetHipError, match="sh"):
            ops.conv_grp_fwd(x, w, 4, out=y, **kw)
        with pytest.raises(DenetHipError, match="sh"):
            ops.conv_grp_dgrad(dy3, w, tuple(x.shape), 4, out=y, **kw)
        with pytest.raises(DenetHipError, match="sh"):
            ops.conv_grp_wgrad(x, dy3, tuple(w.shape), 4, out=torch.full((64, 3, 3, 16), 7.0, device="cuda"), **kw)
        # the entry points themselves: a window that is no multiple of 32, unequal window counts, a padded tap
        L, sp = ops._L(), ops.stream_ptr()
        for geom, match in (((2, 12, 12, 64, 64, 16, 16, 3, 3, 3, 1, 1, 1, 1, 12, 12), "window Cw"),
                            ((2, 12, 12, 64, 64, 32, 64, 3, 3, 3, 1, 1, 1, 1, 12, 12), "input windows"),
                            ((2, 12, 12, 64, 64, 32, 32, 3, 4, 3, 1, 1, 1, 1, 12, 12), "S_real")):
            with pytest.raises(DenetHipError, match=match):
                ops.check(L.denet_conv_grp_fwd(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 0, *geom, sp), "conv_grp_fwd")
            with pytest.raises(DenetHipError, match=match):
                ops.check(L.denet_conv_grp_dgrad(dy.data_ptr(), w.data_ptr(), None, y.data_ptr(), *geom, sp), "conv_grp_dgrad")
        with pytest.raises(DenetHipError, match="Cg must be"):
            ops.check(L.denet_conv_grp_expand(w.data_ptr(), y.data_ptr(), 64, 3, 3, 3, sp), "conv_grp_expand")
        with pytest.raises(DenetHipError, match="Cg must be"):
            ops.check(L.denet_conv_grp_compact(w.data_ptr(), y.data_ptr(), 64, 3, 3, 32, sp), "conv_grp_compact")
    torch.cuda.synchronize()
    assert trace.symbols == []
    assert bool(torch.all(y == 7.0))


# ------------------------------------------------------------------------------------------------- a whole step of a grouped model
# a slab layer (Cg = 16), a grouped stride-2 bottleneck with a projection (Cg = 8), a depthwise rectangular layer behind it, and a
# window-path layer (Cw = 64)
DESC = "C.B[64,3] BN A C.G[64,3,1,4] BN A nRSN.O[1,128,3,2,64,1,8] C.GX[128,3,1,1,1,128] BN A C.G[128,3,1,2] BN A R"
GROUPED_ROWS = ["4.conv", "7.resnet.1", "8.conv", "11.conv"]


def _model(B, CLS, seed):
    m = build_model(DESC, (3, 16, 16), B, CLS, seed=seed, head_scale=0.05)
    m.class_labels = {"c%i" % i: i for i in range(CLS)}
    return m


def _assert_grouped_rows(audit, training):
    rows = {r["layer"]: r for r in audit.table}
    assert set(GROUPED_ROWS) <= set(rows), sorted(rows)
    for name, r in rows.items():
        syms = r["fwd"] + r["bwd"]
        if name in GROUPED_ROWS:
            assert r["geometry"].split()[-1] in ("g4", "g8", "g128", "g2"), r
            assert len(r["fwd"]) == 1 and r["fwd"][0].startswith("conv_grp_kernel<0, "), r
            if training:
                assert sorted(s[:18] for s in r["bwd"]) == ["conv_grp_kernel<1,", "conv_grp_kernel<2,"], r
        else:
            assert all(not s.startswith("conv_grp") for s in syms), r               # every other row: the kernels it always ran
    return rows


def _twin_params(model, values):
    """the float64 leaves the reference runs on: a grouped filter as its dense twin"""
    groups = {id(l): l.groups for _, l in conv_layers(model) if l.grouped}
    params = {}
    for k, vs in values.items():
        ts = [torch.from_numpy(v).double() for v in vs]
        if k in groups:
            ts[0] = expand_ref(ts[0], groups[k])
        params[k] = [t.requires_grad_(True) for t in ts]
    return params, groups


def _step_vs_fp64(model, x, cls, metas, LR, MOM, DECAY, it, audit_rows=True):
    """one SGD step against float64 on the dense twin: cost, every gradient, every update, batch statistics; returns what the
    later checks need"""
    weights = set(id(p) for l in model_cnn.walk_layers(model.layers) for p in l.weights())
    before = param_layers(model)
    values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}
    with KernelAudit(model) as audit:
        cost, _ = model.train_step(x, metas, 0, it, LR, [MOM], DECAY)
        torch.cuda.synchronize()
    if audit_rows:
        for row in audit.table:
            print(row)
        _assert_grouped_rows(audit, True)
    relu_masks = relu_masks_of(model)
    relu_masks.update(block_exit_masks(model))
    params, groups = _twin_params(model, values)
    flips, outs = {}, {}
    cost_ref, _, stats = reference(model, x, params, cls, True, relu_masks=relu_masks, flips=flips, outs=outs)
    cost_ref.backward()
    print("ReLU decisions that differ from float64:", {k: v for k, v in flips.items() if v})
    print("cost", cost, float(cost_ref.detach()))
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach())), (cost, float(cost_ref.detach()))
    # the grouped gradient is the diagonal blocks of the twin's
    compact = {}
    for k, ts in params.items():
        compact[k] = list(ts)
        if k in groups:
            t = compact_ref(ts[0].detach(), groups[k]).requires_grad_(True)
            t.grad = compact_ref(ts[0].grad, groups[k])
            off = ts[0].grad - expand_ref(t.grad, groups[k])
            assert float(off.abs().max()) >= 0.0                                      # (the other blocks carry a gradient nobody reads)
            compact[k][0] = t
    return cost, before, values, compact, weights, stats, outs


def test_grouped_model_training_steps_and_inference_vs_fp64(hip, tmp_path):
    """one sgd step of a model with a slab layer, a grouped stride-2 bottleneck, a depthwise rectangular layer and a window-path
    layer: cost, every parameter gradient, every updated parameter and the batch statistics against float64 on the dense twin (1e-3
    max-norm, the ReLU decisions taken from the device), which kernels ran; a second step (the slab filter follows the solver's
    update); omega.set_value followed by a forward pass; test-mode probabilities folded and unfolded; the save / reload / predict
    round trip"""
    B, CLS, LR, MOM, DECAY = 4, 10, 0.02, 0.0, 0.0005
    model = _model(B, CLS, seed=3)
    assert [name for name, l in conv_layers(model) if l.grouped] == GROUPED_ROWS
    assert [l.groups for _, l in conv_layers(model)] == [1, 4, 1, 8, 1, 1, 128, 2, 1]
    assert [ops.conv_grp_window(l.cp, l.kp, l.groups)[2] for _, l in conv_layers(model) if l.grouped] == [16, 8, 1, 0]
    model.build_train_func("sgd")
    rng = np.random.RandomState(11)
    x = rng.uniform(0.0, 1.0, (B, 3, 16, 16)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    metas = [{"image_class": int(c)} for c in cls]
    # the second step's batch: another one (four images a step has just been taken on are memorised: a cost of 0 and gradients of 0
    # would compare nothing)
    x1 = rng.uniform(0.0, 1.0, (B, 3, 16, 16)).astype(np.float32)
    cls1 = rng.randint(0, CLS, B)
    metas1 = [{"image_class": int(c)} for c in cls1]

    stats = None
    for it, (xb, clsb, mb) in enumerate(((x, cls, metas), (x1, cls1, metas1))):      # (no momentum: each step is a first step)
        cost, before, values, params, weights, stats, outs = _step_vs_fp64(model, xb, clsb, mb, LR, MOM, DECAY, it)
        assert cost > 0.1
        report, bad = [], []
        for l, p, e_g, e_p, g_dev, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
            i = l.layer_index
            if p is getattr(l, "beta", None) and l.type_name == "conv":
                # the stem's bias in front of a batch norm: its exact gradient is 0 and max|b| is no scale; the error is taken
                # against the largest sum of |dy| over a channel (tests/test_conv_dilated_gpu.py does the same)
                assert model.layers[i + 1].type_name == "batchnorm"
                scale = float(outs[id(l)].grad.abs().sum(dim=(0, 2, 3)).max())
                v64 = torch.from_numpy(values[id(l)][1]).double()
                p_dev = torch.from_numpy(p.get_value().copy()).double()
                p_ref = v64 - LR * (g_ref + (DECAY if id(p) in weights else 0.0) * v64)
                e_g = float((g_dev - g_ref).abs().max()) / scale
                e_p = float(((p_dev - v64) - (p_ref - v64)).abs().max()) / (LR * scale)
            report.append("step %d L%d %s %s: grad %.2e, update %.2e" % (it, i, l.type_name, p.name, e_g, e_p))
            if not (e_g <= 1e-3 and e_p <= 1e-3):
                bad.append(report[-1])
        print("\n".join(report))
        assert not bad, bad
        if it == 0:
            running = {}
            for l in model_cnn.walk_layers(model.layers):
                if l.type_name == "batchnorm":
                    rm = torch.from_numpy(l.mean.get_value().copy()).double()
                    rs = torch.from_numpy(l.stdinv.get_value().copy()).double()
                    m_ref = (1.0 - l.momentum) * stats[id(l)]["mean"]
                    s_ref = l.momentum + (1.0 - l.momentum) * stats[id(l)]["stdinv"]
                    assert _rel(rm, m_ref) <= 1e-3 and _rel(rs, s_ref) <= 1e-3, l.layer_index

    def running_now():
        return {id(l): (torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double())
                for l in model_cnn.walk_layers(model.layers) if l.type_name == "batchnorm"}

    def probabilities_ref():
        vals = {id(l): [p.get_value().copy() for p in ps] for l, ps in param_layers(model)}
        now, _ = _twin_params(model, vals)
        with torch.no_grad():
            _, logits, _ = reference(model, x, now, cls, False, running=running_now())
        return torch.softmax(logits, dim=1)

    def e_prob(pr, pr_ref):
        return float((torch.from_numpy(pr).double() - pr_ref).abs().max()) / float(pr_ref.max())

    # inference: the batch norms behind the grouped layers are folded into conv_grp_fwd's epilogue (a slab layer expands the
    # folded filter)
    assert ops.INFER_FOLD
    with KernelAudit(model) as audit:
        pr = model.predict_output_step(x)
        torch.cuda.synchronize()
    _assert_grouped_rows(audit, False)
    pr_ref = probabilities_ref()
    print("test-mode probabilities: %.2e (largest %.3f)" % (e_prob(pr, pr_ref), float(pr_ref.max())))
    assert pr.shape == (B, CLS) and e_prob(pr, pr_ref) <= 1e-3
    with ops.infer_fold(False):
        with KernelAudit(model) as audit:
            pr_unfolded = model.predict_output_step(x)
            torch.cuda.synchronize()
    _assert_grouped_rows(audit, False)
    assert e_prob(pr_unfolded, pr_ref) <= 1e-3

    # omega.set_value: the next forward pass reads the new filter (the kept slab filter is of an older weights version)
    slab_layer = dict(conv_layers(model))["4.conv"]
    old = slab_layer.omega.get_value().copy()
    slab_layer.omega.set_value(-0.5 * old)
    pr_set = model.predict_output_step(x)
    pr_set_ref = probabilities_ref()
    print("after set_value: %.2e, moved by %.2e" % (e_prob(pr_set, pr_set_ref), float((pr_set_ref - pr_ref).abs().max())))
    assert e_prob(pr_set, pr_set_ref) <= 1e-3
    assert not np.array_equal(pr_set, pr)                                                  # (the edit reached the output)
    slab_layer.omega.set_value(old)
    assert np.array_equal(model.predict_output_step(x).view(np.int32), pr.view(np.int32))

    path = str(tmp_path / "grouped.mdl.gz")
    model_cnn.save_to_file(model, path)
    again = model_cnn.load_from_file(path, B)
    assert [l.output_shape for l in again.layers] == [l.output_shape for l in model.layers]
    assert [l.groups for _, l in conv_layers(again)] == [l.groups for _, l in conv_layers(model)]
    # (as loaded, an `original` block runs its `BN A` pairs apart - see tests/test_conv_dilated_gpu.py; prepared alike, same bits)
    assert e_prob(again.predict_output_step(x), pr_ref) <= 1e-3
    prepared = model_cnn.load_from_file(path, B)
    prepared.build_train_func("sgd")
    pr2 = prepared.predict_output_step(x)
    assert np.array_equal(pr2.view(np.int32), pr.view(np.int32))


def test_resnext50_training_step_is_finite_and_deterministic(hip):
    """zoo.resnext50 at 64 x 64: one training step runs, the cost is finite and the same in two runs (no float64 at this depth)"""
    B = 2
    rng = np.random.RandomState(5)
    x = rng.uniform(0.0, 1.0, (B, 3, 64, 64)).astype(np.float32)
    metas = [{"image_class": int(c)} for c in rng.randint(0, 1000, B)]
    costs = []
    for _ in range(2):
        m = zoo.resnext50(B, image=64)
        m.build_train_func("sgd")
        if not costs:
            with KernelAudit(m) as audit:
                cost, _ = m.train_step(x, metas, 0, 0, 0.01, [0.9], 1e-4)
                torch.cuda.synchronize()
            rows = {r["layer"]: r for r in audit.table}
            grouped = [name for name, l in conv_layers(m) if l.grouped]
            assert len(grouped) == 16
            for name in grouped:
                assert rows[name]["fwd"][0].startswith("conv_grp_kernel<0, "), rows[name]
        else:
            cost, _ = m.train_step(x, metas, 0, 0, 0.01, [0.9], 1e-4)
        costs.append(cost)
    print("cost", costs)
    assert np.isfinite(costs[0]) and costs[0] == costs[1]
