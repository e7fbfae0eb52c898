"""Opt-in bf16 training (ops.TRAIN_PRECISION = "bf16", csrc/conv_bf16.hip + csrc/conv_bf16_train.hip) on the device.

The numerics contract ("bf16 training") and the checkers that state its bound - fp64 on the operands a kernel really
multiplies, for the forward pass and the two gradients - are in tests/bf16_reference.py."""
import glob
import os

import numpy as np
import pytest
import torch

from bf16_reference import bits, check_dgrad, check_fwd, check_wgrad, draw, ties
from denet_amd import ops
from denet_amd.model import audit, model_cnn, zoo
from fp64_model import build_model, png_dataset as _png_dataset

pytestmark = pytest.mark.gpu

FWD = "conv_bf16_kernel"
WGRAD = "conv_bf16_wgrad_kernel"
REDUCE = "conv_bf16_wgrad_reduce_kernel"
COPY = "filter_to_bf16_dgrad_kernel"


# ------------------------------------------------------------------------------------------------------ 1: the data gradient
# (N, H, W, C physical, C logical, K, filter, pad, with add)
DGRAD = {
    "one-tile": (1, 8, 8, 32, 32, 32, 3, 1, False),
    "partial-tiles": (2, 9, 7, 96, 96, 160, 3, 1, False),
    "17-chunks-1x1": (1, 6, 5, 32, 32, 544, 1, 0, False),
    "with-add": (2, 9, 7, 96, 96, 160, 3, 1, True),
    "pad-channels": (1, 8, 8, 128, 100, 32, 3, 1, True),
    "pad-full": (1, 6, 7, 32, 32, 64, 3, 2, False),
    "pad-zero": (1, 9, 8, 64, 64, 32, 3, 0, False),
}


def _dgrad_case(name):
    N, H, W, C, Cl, K, k, pad, with_add = DGRAD[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    OH, OW = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    dy = draw(rng, N, OH, OW, K)
    w = draw(rng, K, k, k, C, scale=(k * k * K) ** -0.5)
    w[..., Cl:] = 0.0                                # pad channels of a filter are zero, as Param packs them
    add = None
    if with_add:
        add = draw(rng, N, H, W, C)
        add[..., Cl:] = 0.0
    wt = ops.filter_to_bf16_dgrad(w.cuda())
    dx = ops.conv_dgrad_bf16(dy.cuda(), wt, (N, H, W, C), add=None if add is None else add.cuda(), pad=pad)
    torch.cuda.synchronize()
    return dy, w, add, wt, dx


@pytest.mark.parametrize("name", list(DGRAD))
def test_data_gradient_against_fp64_on_the_rounded_operands(hip, name):
    N, H, W, C, Cl, K, k, pad, with_add = DGRAD[name]
    dy, w, add, wt, dx = _dgrad_case(name)
    # the rotated, transposed copy is the RNE rounding of the fp32 filter, bit for bit
    want = w.bfloat16().flip(1, 2).permute(3, 1, 2, 0).contiguous()
    assert torch.equal(wt.cpu().view(torch.int16), want.view(torch.int16))
    check_dgrad(dx, dy, w, (N, H, W, C), add=add, stride=1, pad=pad, what="dgrad " + name)
    if Cl != C:
        assert int(bits(dx[..., Cl:]).abs().max()) == 0, "pad channels must be +0 (sign bit clear)"
        assert bool((dy < 0).any())


def test_data_gradient_rounds_to_nearest_even_bit_for_bit(hip):
    """1x1 identity filter: dx is the staged (rounded) dy itself"""
    vals = ties()
    dy = np.random.RandomState(3).standard_normal((2, 5, 7, 32)).astype(np.float32)
    dy.reshape(-1)[:: 3][:vals.size * 8] = np.tile(vals, 8)
    dy = torch.from_numpy(dy)
    w = torch.eye(32).reshape(32, 1, 1, 32).contiguous()
    dx = ops.conv_dgrad_bf16(dy.cuda(), ops.filter_to_bf16_dgrad(w.cuda()), (2, 5, 7, 32))
    assert torch.equal(bits(dx.cpu()), bits(dy.bfloat16().float()))


# ---------------------------------------------------------------------------------------------------- 2: the filter gradient
# (N, H, W, C physical, C logical, K physical, K logical, filter, stride, pad, slices the rule gives)
WGRADS = {
    "one-pixel": (1, 1, 1, 32, 32, 32, 32, 1, 1, 0, 1),
    "less-than-a-chunk": (1, 4, 5, 32, 32, 32, 32, 3, 1, 1, 1),
    "ragged-chunks": (2, 9, 7, 32, 32, 64, 64, 3, 1, 1, 1),
    "stride-2-odd-map": (2, 9, 7, 64, 64, 32, 32, 3, 2, 1, 1),
    "1x1": (2, 6, 6, 64, 64, 96, 96, 1, 1, 0, 1),
    "partial-tiles": (2, 9, 7, 96, 96, 160, 160, 3, 1, 1, 1),
    "three-slices-ragged": (2, 15, 14, 32, 32, 32, 32, 3, 1, 1, 3),
    "pad-rows-and-columns": (1, 8, 8, 128, 100, 64, 50, 3, 1, 1, 1),
}


def _wgrad_case(name):
    N, H, W, C, Cl, K, Kl, k, stride, pad, slices = WGRADS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = draw(rng, N, H, W, C)
    dy = draw(rng, N, OH, OW, K)
    x[..., Cl:] = 0.0                                # pad channels of activations and gradients are +0
    dy[..., Kl:] = 0.0
    g = ops.conv_geom(x.shape, (K, k, k, C), stride, pad)
    dw = ops.conv_wgrad_bf16(x.cuda(), dy.cuda(), (K, k, k, C), stride=stride, pad=pad)
    torch.cuda.synchronize()
    return x, dy, dw, ops.conv_wgrad_bf16_slices(g)


@pytest.mark.parametrize("name", list(WGRADS))
def test_filter_gradient_against_fp64_on_the_rounded_operands(hip, name):
    N, H, W, C, Cl, K, Kl, k, stride, pad, slices = WGRADS[name]
    x, dy, dw, got_slices = _wgrad_case(name)
    assert got_slices == slices, (name, got_slices)
    check_wgrad(dw, x, dy, stride=stride, pad=pad, slices=slices, what="wgrad " + name)
    if Kl != K:
        assert not bits(dw[Kl:]).any() and not bits(dw[..., Cl:]).any(), "pad rows and columns must be exactly 0"
        assert bool(dw[:Kl, ..., :Cl].abs().min() > 0)


def test_three_slices_case_has_a_ragged_last_slice(hip):
    """14 chunks of 32 pixels (420 pixels: the last chunk holds 4) in 3 slices of 5 + 5 + 4 chunks"""
    N, H, W, C, Cl, K, Kl, k, stride, pad, slices = WGRADS["three-slices-ragged"]
    M = N * H * W
    chunks = -(-M // 32)
    per = -(-chunks // slices)
    assert M % 32 != 0 and chunks % per != 0 and slices >= 3
    assert hip.denet_conv_wgrad_bf16_slices(N, C, K, k, k, H, W) == slices


def test_filter_gradient_rounds_to_nearest_even_bit_for_bit(hip):
    """one pixel, x = 1: dw[k][c] is the staged (rounded) dy[k] itself"""
    vals = ties()
    dy = np.random.RandomState(4).standard_normal(32).astype(np.float32)
    dy[:vals.size] = vals
    dy = torch.from_numpy(dy).reshape(1, 1, 1, 32)
    x = torch.ones(1, 1, 1, 32)
    dw = ops.conv_wgrad_bf16(x.cuda(), dy.cuda(), (32, 1, 1, 32))
    want = dy.bfloat16().float().reshape(32, 1, 1, 1).expand(32, 1, 1, 32).contiguous()
    assert torch.equal(bits(dw.cpu()), bits(want))


def test_two_calls_are_bit_identical(hip):
    a, b = _wgrad_case("three-slices-ragged"), _wgrad_case("three-slices-ragged")
    assert torch.equal(bits(a[2]), bits(b[2]))
    a, b = _dgrad_case("partial-tiles"), _dgrad_case("partial-tiles")
    assert torch.equal(bits(a[4]), bits(b[4]))


# ------------------------------------------------------------------------------------------------ 3: a model, layer by layer
STACK_DESC = "C[32,3] BN A C[64,3] BN A C[64,3,2] BN A C[96,1] BN A P.A[8] R"
RSN_DESC = "C[32,3] BN A RSN[32,3] RSN.O[64,3,2] P.A[8] R"
STACK_B, STACK_IMG, STACK_CLASSES = 4, 16, 10


def _build(desc, seed=5, solver="nesterov"):
    m = build_model(desc, (3, STACK_IMG, STACK_IMG), STACK_B, STACK_CLASSES, seed=seed, head_scale=0.05)
    m.build_train_func(solver)
    return m


def _batch(seed=4):
    return zoo.synthetic_batch(STACK_B, STACK_IMG, STACK_CLASSES, seed=seed)


def _all(rows, key):
    return [s for r in rows for s in r[key]]


class _Recorder:
    """wraps ops.conv_fwd / conv_dgrad / conv_wgrad: keeps what every bf16-mode call read and wrote"""

    def __init__(self, monkeypatch):
        self.fwd, self.dgrad, self.wgrad = [], [], []
        f0, d0, w0 = ops.conv_fwd, ops.conv_dgrad, ops.conv_wgrad
        keep = lambda t: None if t is None else t.detach().clone()

        def fwd(x, w, bias=None, add=None, stride=1, pad=0, **kw):
            cache, link, up = kw.get("cache"), kw.get("link"), kw.get("up")
            if not (cache and cache.get("bf16_train")):
                return f0(x, w, bias=bias, add=add, stride=stride, pad=pad, **kw)
            xin = x if x is not None else (link if link is not None else up).materialise()
            rec = dict(x=keep(xin), w=keep(w), bias=keep(bias), add=keep(add), stride=stride, pad=pad)
            out = f0(x, w, bias=bias, add=add, stride=stride, pad=pad, **kw)
            rec["y"] = keep(out)
            self.fwd.append(rec)
            return out

        def dgrad(dy, w, x_shape, add=None, stride=1, pad=0, **kw):
            cache = kw.get("cache")
            if not (cache and cache.get("bf16_train")):
                return d0(dy, w, x_shape, add=add, stride=stride, pad=pad, **kw)
            rec = dict(dy=keep(dy), w=keep(w), add=keep(add), x_shape=tuple(x_shape), stride=stride, pad=pad)
            out = d0(dy, w, x_shape, add=add, stride=stride, pad=pad, **kw)
            rec["dx"] = keep(out)
            self.dgrad.append(rec)
            return out

        def wgrad(x, dy, w_shape, stride=1, pad=0, **kw):
            cache = kw.get("cache")
            if not (cache and cache.get("bf16_train")):
                return w0(x, dy, w_shape, stride=stride, pad=pad, **kw)
            rec = dict(x=keep(x), dy=keep(dy), stride=stride, pad=pad)
            out = w0(x, dy, w_shape, stride=stride, pad=pad, **kw)
            rec["dw"] = keep(out)
            rec["slices"] = ops.conv_wgrad_bf16_slices(ops.conv_geom(x.shape, w_shape, stride, pad))
            self.wgrad.append(rec)
            return out

        monkeypatch.setattr(ops, "conv_fwd", fwd)
        monkeypatch.setattr(ops, "conv_dgrad", dgrad)
        monkeypatch.setattr(ops, "conv_wgrad", wgrad)

    def check(self, what, nonzero=True):
        """-> the number of bf16 data gradients checked. nonzero=False: a gradient that is exactly zero (a head without RoIs in a
        cold first step) must come out exactly zero; self.live counts the gradient passes with something in them"""
        for i, r in enumerate(self.fwd):
            check_fwd(r["y"], r["x"], r["w"], bias=r["bias"], add=r["add"], stride=r["stride"], pad=r["pad"],
                      what="%s fwd %d" % (what, i))
        n16 = self.live = 0
        for i, r in enumerate(self.dgrad):
            if r["stride"] != 1:
                continue                             # (the strided data gradient runs the exact fp32 kernels)
            self.live += check_dgrad(r["dx"], r["dy"], r["w"], r["x_shape"], add=r["add"], stride=1, pad=r["pad"],
                                     what="%s dgrad %d" % (what, i), nonzero=nonzero)
            n16 += 1
        for i, r in enumerate(self.wgrad):
            self.live += check_wgrad(r["dw"], r["x"], r["dy"], stride=r["stride"], pad=r["pad"], slices=r["slices"],
                                     what="%s wgrad %d" % (what, i), nonzero=nonzero)
        return n16


def test_stack_step_kernels_and_layers_against_fp64(hip, monkeypatch):
    model = _build(STACK_DESC)
    x, metas = _batch()
    rec = _Recorder(monkeypatch)
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert np.isfinite(cost)
    rows = ka.table
    assert len(rows) == 5, rows
    for r in (rows[0], rows[-1]):                    # the stem (4 planar channels) and the convolution the softmax reads: fp32
        assert r["fwd"] and r["bwd"] and not any("bf16" in s for s in r["fwd"] + r["bwd"]), r
    assert [r["fwd"] for r in rows[1:4]] == [[FWD + "<128, 64>"], [FWD + "<128, 64>"], [FWD + "<128, 128>"]], rows
    for i, r in enumerate(rows[1:4]):
        assert not any("wino" in s for s in r["fwd"] + r["bwd"]), r
        assert sum(s.startswith(WGRAD + "<") for s in r["bwd"]) == 1, r
        if i == 1:                                   # the stride-2 layer: its data gradient stays on an fp32 kernel
            assert not any(s.startswith(FWD) or s == COPY for s in r["bwd"]), r
            assert any(s.startswith("dgrad_s2_kernel") or s.startswith("igemm_kernel") for s in r["bwd"]), r
        else:
            assert sum(s.startswith(FWD + "<") for s in r["bwd"]) == 1 and r["bwd"].count(COPY) == 1, r
            assert not any(s.startswith("dgrad_s2_kernel") or s.startswith("igemm_kernel") for s in r["bwd"]), r
    assert len(rec.fwd) == 3 and len(rec.dgrad) == 3 and len(rec.wgrad) == 3
    assert rec.check("stack") == 2
    # the recorded filter gradients are what the solver read
    convs = [l for _, l in audit.conv_layers(model)]
    for conv, r in zip(reversed(convs[1:4]), rec.wgrad):
        assert torch.equal(bits(conv.omega.grad.view(conv.omega.dev_shape)), bits(r["dw"]))


def test_nothing_is_prepared_for_passes_that_do_not_run(hip):
    """the second step's filter prefetch (ops.wino_prefetch_filters) goes by what the first step's passes noted in the layer caches:
    an eligible layer notes no Winograd tile and no transposed filter, so nothing is transformed for it"""
    model = _build(STACK_DESC)
    x, metas = _batch()
    with ops.train_precision("bf16"):
        for it in range(2):
            model.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    convs = [l for _, l in audit.conv_layers(model)]
    for conv in convs[1:4]:
        c = conv._cache()
        assert c["bf16_train"] and c["w16_train"][0] == ops.WEIGHTS_VERSION - 1
        assert not c.get("fwd_tile_train") and not c.get("dgrad_tile") and not c.get("dgrad_1x1t") and not c.get("dgrad_t"), c.keys()
        assert ("u", 0) not in c and ("u", 1) not in c and "wt" not in c and "V" not in c, c.keys()
    assert not convs[0]._cache()["bf16_train"] and not convs[-1]._cache()["bf16_train"]


def test_kernel_profile_names_and_counts_the_bf16_launches(hip):
    """ops.KernelProfile (the event-pair profile bench.py's roofline leg uses): every record of a bf16 step has its FLOP entry"""
    model = _build(STACK_DESC)
    x, metas = _batch()
    with ops.train_precision("bf16"):
        model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
        prof = ops.KernelProfile()
        with ops.switches(PROFILE=prof):
            model.train_step(x, metas, 0, 1, 0.05, [0.9], 1e-4)
        agg = prof.summary()
    assert agg[WGRAD + "<64, 128>"]["launches"] == 2 and agg[WGRAD + "<128, 128>"]["launches"] == 1, agg
    assert agg[COPY]["launches"] == 2 and agg[COPY]["flops"] == 0, agg
    assert sum(a["launches"] for n, a in agg.items() if n.startswith(FWD + "<")) == 3 + 2, agg
    assert all(a["ms"] > 0 for a in agg.values())


def test_denet_skip_step_layers_against_fp64(hip, monkeypatch):
    """one bf16 step of DeNet-34 skip (batch 2, 128x128): every eligible layer's three passes on the tensors they read, the SKIP adds
    that ride in a convolution epilogue included; the corner and detect convolutions and the stem stay fp32"""
    model = zoo.denet34(2, "skip", 128, class_num=80, seed=1)
    zoo.warm_corner_head(model, 4.0, 0.3)            # (as initialised the corner softmax saturates: no gradient reaches the base)
    model.build_train_func("nesterov")
    x, metas = zoo.synthetic_batch(2, 128, seed=2)
    rec = _Recorder(monkeypatch)
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert np.isfinite(cost)
    n_bf16 = 0
    for i, r in enumerate(ka.table):
        top = r["layer"].split(".")[1]
        if i == 0 or top in ("denet-corner", "denet-detect"):
            assert r["fwd"] and not any("bf16" in s for s in r["fwd"] + r["bwd"]), r
        else:
            assert r["fwd"] and all(s.startswith(FWD) for s in r["fwd"]), r
            assert sum(s.startswith(WGRAD + "<") for s in r["bwd"]) == 1 and not any("wino" in s for s in r["bwd"]), r
            n_bf16 += 1
    assert n_bf16 >= 30 and len(rec.fwd) == n_bf16 and len(rec.wgrad) == n_bf16, (n_bf16, len(rec.fwd), len(rec.wgrad))
    assert sum(r["add"] is not None for r in rec.fwd) >= 1, "no SKIP add rode in a bf16 epilogue"
    assert rec.check("DeNet-34 skip", nonzero=False) >= 20
    assert rec.live >= 40, rec.live                  # (the corner cost reaches the whole base network)


def test_residual_blocks_step_against_fp64(hip, monkeypatch):
    model = _build(RSN_DESC, seed=6)
    x, metas = _batch(10)
    rec = _Recorder(monkeypatch)
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert np.isfinite(cost)
    inner = [r for r in ka.table if ".resnet" in r["layer"]]
    assert len(inner) == 5, ka.table                 # RSN: 2 convolutions; RSN.O with a stride: 2 + the shortcut projection
    for r in inner:
        assert r["fwd"] and all(s.startswith(FWD) for s in r["fwd"]), r
        assert sum(s.startswith(WGRAD + "<") for s in r["bwd"]) == 1 and not any("wino" in s for s in r["bwd"]), r
    for r in (ka.table[0], ka.table[-1]):
        assert r["fwd"] and not any("bf16" in s for s in r["fwd"] + r["bwd"]), r
    assert len(rec.fwd) == 5 and len(rec.wgrad) == 5 and len(rec.dgrad) == 5
    print("RSN: bf16 forward passes with a residual in the epilogue: %d, bf16 data gradients onto an accumulated gradient: %d"
          % (sum(r["add"] is not None for r in rec.fwd), sum(r["add"] is not None and r["stride"] == 1 for r in rec.dgrad)))
    assert rec.check("RSN") >= 3


def _state(model):
    return [bits(model.P).cpu().numpy(), bits(model.G).cpu().numpy()]


def _one_step(desc, precision, seed=5):
    model = _build(desc, seed=seed)
    x, metas = _batch()
    with ops.train_precision(precision), audit.KernelAudit(model) as ka:
        cost, costs = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    return _state(model) + [np.float32(cost).view(np.uint32), np.array(costs, dtype=np.float32).view(np.uint32)], ka.table


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_fp32_steps_before_between_and_after_bf16_steps_are_bit_identical(hip):
    """whole steps of fresh models from one seed, one after the other: fp32, bf16, fp32 (its own block inside a bf16 block), bf16,
    fp32. (A model that lives WHILE a bf16 model steps: the next test.)"""
    before, t0 = _one_step(STACK_DESC, "fp32")
    low, tl = _one_step(STACK_DESC, "bf16")
    with ops.train_precision("bf16"):
        between, t1 = _one_step(STACK_DESC, "fp32")  # (the inner block of _one_step wins: the mode is read per forward pass)
    low2, _ = _one_step(STACK_DESC, "bf16")
    after, t2 = _one_step(STACK_DESC, "fp32")
    assert _same(before, between) and _same(before, after), "an fp32 step changed around a bf16 step"
    for t in (t0, t1, t2):
        assert not any("bf16" in s for s in _all(t, "fwd") + _all(t, "bwd")), t
    assert any(s.startswith(WGRAD) for s in _all(tl, "bwd"))
    assert _same(low, low2), "two bf16 steps from the same state differ"
    assert not _same(before[:1], low[:1]), "the bf16 step ran the fp32 kernels"


def _sweeps(model, x, metas, between=None):
    """the forward and the backward sweep of one step of `model` (no solver), with `between` run in the middle"""
    from denet_amd import layer as layer_mod
    layer_mod.set_iteration(0)
    layer_mod.set_epoch(0)
    layer_mod.set_rng_seed(model.rng_seed)
    with audit.KernelAudit(model) as ka:
        ctx = model.forward(x, metas, train=True)
        if between is not None:
            between()
            layer_mod.set_rng_seed(model.rng_seed)
        model.backward(ctx)
    torch.cuda.synchronize()
    return [bits(model.G).cpu().numpy(), bits(model.cost_buf).cpu().numpy()], ka.table


def test_an_fp32_model_is_untouched_by_a_bf16_model_stepping_beside_it(hip):
    """a bf16 model takes whole training steps between the forward and the backward sweep of an fp32 model of the same seed: the
    fp32 model's gradients and costs are those of a model that ran alone, bit for bit, and its audit names no bf16 kernel"""
    x, metas = _batch()
    alone, _ = _sweeps(_build(STACK_DESC), x, metas)
    with ops.train_precision("bf16"):
        low = _build(STACK_DESC)
    tables = []

    def bf16_steps():
        with ops.train_precision("bf16"), audit.KernelAudit(low) as ka:
            for it in range(2):
                low.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
        tables.append(ka.table)

    beside, t = _sweeps(_build(STACK_DESC), x, metas, between=bf16_steps)
    assert any(s.startswith(WGRAD) for s in _all(tables[0], "bwd")), "the model beside did not step in bf16"
    assert not any("bf16" in s for s in _all(t, "fwd") + _all(t, "bwd")), t
    assert int(np.count_nonzero(alone[0])) > 0
    assert _same(alone, beside), "an fp32 model's step changed while a bf16 model stepped beside it"


def test_head_bf16x3_is_refused_where_the_mode_is_read(hip, monkeypatch):
    """a model whose build_train_func ran in fp32 mode and that is then stepped in bf16 mode with the 3-term head split on: the first
    eligible layer's forward pass raises, before any bf16 kernel runs"""
    model = _build(STACK_DESC)
    x, metas = _batch()
    monkeypatch.setattr(ops, "HEAD_BF16X3", True)
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        with pytest.raises(ValueError):
            model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert not any("bf16" in s for s in _all(ka.table, "fwd") + _all(ka.table, "bwd")), ka.table


@pytest.mark.parametrize("desc", [STACK_DESC, RSN_DESC], ids=["stack", "RSN"])
def test_inference_after_a_bf16_step_is_fp32_inference(hip, desc):
    """the mode a training step recorded in the layer caches is that step's: a test-mode pass of the same model (batch norms folded,
    ReLU and residual in the epilogue) names no bf16 kernel, and equals bit for bit the inference of a twin that took an fp32 step
    and was then given the same parameters and running statistics"""
    x, metas = _batch()
    xin = np.random.RandomState(9).uniform(0.0, 1.0, (STACK_B, 3, STACK_IMG, STACK_IMG)).astype(np.float32)
    model, twin = _build(desc), _build(desc)
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    assert any(s.startswith(WGRAD) for s in _all(ka.table, "bwd"))
    twin.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert not torch.equal(model.P, twin.P)
    twin.P.copy_(model.P)
    twin.S.copy_(model.S)
    ops.bump_weights_version()
    assert ops.INFER_PRECISION == "fp32"
    with audit.KernelAudit(model) as ka:
        pr = model.predict_output_step(xin)
    assert _all(ka.table, "fwd") and not any("bf16" in s for s in _all(ka.table, "fwd")), ka.table
    want = twin.predict_output_step(xin)
    assert np.isfinite(pr).all() and abs(float(pr.sum()) - STACK_B) < 1e-3
    assert np.array_equal(pr.view(np.uint32), want.view(np.uint32))
    # ... and the other way round: the next training step of that model is a bf16 step again, an fp32 one is not
    with ops.train_precision("bf16"), audit.KernelAudit(model) as ka:
        model.train_step(x, metas, 0, 1, 0.05, [0.9], 1e-4)
    assert any(s.startswith(WGRAD) for s in _all(ka.table, "bwd"))
    with audit.KernelAudit(model) as ka:
        model.train_step(x, metas, 0, 2, 0.05, [0.9], 1e-4)
    assert not any("bf16" in s for s in _all(ka.table, "fwd") + _all(ka.table, "bwd")), ka.table


def test_backward_follows_the_mode_recorded_in_the_forward_pass(hip):
    """the global flips between the two sweeps of one step: the backward pass runs what the forward pass recorded"""
    model = _build(STACK_DESC)
    x, metas = _batch()
    from denet_amd import layer as layer_mod
    layer_mod.set_iteration(0)
    layer_mod.set_epoch(0)
    layer_mod.set_rng_seed(model.rng_seed)
    with audit.KernelAudit(model) as ka:
        with ops.train_precision("bf16"):
            ctx = model.forward(x, metas, train=True)
        assert ops.TRAIN_PRECISION == "fp32"
        model.backward(ctx)
    torch.cuda.synchronize()
    for r in ka.table[1:4]:
        assert sum(s.startswith(WGRAD + "<") for s in r["bwd"]) == 1, r


def test_it_trains(hip):
    """20 SGD steps on one fixed batch in both modes, same seed: a gross-failure detector (a wrong sign or a dropped gradient
    recovers none of the decrease), not a precision claim. The curves are recorded in EXPERIMENTS.md"""
    x, metas = _batch()
    curves = {}
    for precision in ("fp32", "bf16"):
        model = _build(STACK_DESC, solver="sgd")
        with ops.train_precision(precision):
            curves[precision] = [float(model.train_step(x, metas, 0, it, 0.05, [0.9], 0.0)[0]) for it in range(20)]
    for k, v in curves.items():
        print("cost curve %s: %s" % (k, " ".join("%.4f" % c for c in v)))
    assert all(np.isfinite(c) for v in curves.values() for c in v)
    drop32 = curves["fp32"][0] - curves["fp32"][-1]
    drop16 = curves["bf16"][0] - curves["bf16"][-1]
    print("cost decrease fp32 %.4f, bf16 %.4f, share %.3f" % (drop32, drop16, drop16 / max(drop32, 1e-30)))
    assert drop32 > 0, "the fp32 run did not train: the test has no yardstick"
    assert drop16 >= 0.5 * drop32


# ---------------------------------------------------------------------------------------------------------- 4: the driver
def test_model_train_with_precision_bf16(hip, tmp_path, monkeypatch):
    """two steps of `model-train --precision bf16 --test ...` on a folder dataset (in this process: the flag wraps the run), the
    epoch's test sweep on the model just trained, and a loadable model"""
    from denet_amd.model import train
    train_dir, test_dir, out = str(tmp_path / "train"), str(tmp_path / "test"), tmp_path / "out"
    _png_dataset(train_dir, classes=2, seed=1)
    _png_dataset(test_dir, classes=2, per_class=2, seed=2)      # (--test: the epoch ends with a test-mode sweep of the model just trained)
    out.mkdir()
    calls, w0 = [], ops.conv_wgrad_bf16

    def counted(*a, **k):
        calls.append(ops.TRAIN_PRECISION)
        return w0(*a, **k)

    monkeypatch.setattr(ops, "conv_wgrad_bf16", counted)
    monkeypatch.chdir(tmp_path)
    argv = ["--seed", "0", "--solver", "sgd", "--border-mode", "half", "--activation", "relu", "--epochs", "1", "--batch-size", "4",
            "--train", train_dir, "--test", test_dir, "--extension", "png", "--learn-rate", "0.05", "--learn-momentum", "0.9", "--output-prefix",
            str(out / "model"), "--precision", "bf16", "--model-desc"] + "C[32,3] BN A C[64,3] BN A C[64,3,2] BN A P.A[16] R".split()
    assert train.main(argv) == 0
    assert ops.TRAIN_PRECISION == "fp32"
    assert len(calls) >= 4 and len(calls) % 2 == 0 and set(calls) == {"bf16"}, calls      # 2 eligible layers per step, 2 steps
    assert os.path.exists(str(out / "model_epoch000.test"))
    final = glob.glob(str(out / "model_epoch000_final.mdl.gz"))
    assert final, os.listdir(str(out))
    model = model_cnn.load_from_file(final[0], 4)
    pr = model.predict_output_step(np.zeros((4, 3, 32, 32), dtype=np.float32))
    assert np.isfinite(pr).all() and pr.shape == (4, 2)
