"""Batch renormalisation on the device (csrc/bn_renorm.hip): `BN[m, eps, r, d, it]`, the JSON keys renormMaxR /
renormMaxD / renormMaxIt, `model-modify --modify-bn-renorm`.

The reference's implementation is the commented-out block denet/layer/batch_norm.py:65-73, so there is no reference run: the yardstick
is a float64 restatement of the definition (`_ref64` in this file, tests/fp64_model.py for the whole model), with autograd for the gradients:
    r = clip((1 / inv_b) * stdinv, 1 / r_max, r_max)            d = clip((mu_b - mean) * stdinv, -d_max, d_max)       (constants)
    y = (x - mu_b) * (gamma * inv_b * r) + (beta + gamma * d)   [+ res] [relu]
with mean / stdinv the running statistics of BEFORE the step's update. Batch norms run on unpadded channel counts only (a multiple
of 32, asserted by the layer), so no tensor of these tests has padded channels to keep at zero."""
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from denet_amd import layer as layer_mod
from denet_amd import ops
from denet_amd.layer import Act, InitialLayer
from denet_amd.layer.batch_norm import BatchNormLayer, renorm_limits
from denet_amd.model import audit, model_cnn
from fp64_model import build_model, param_layers as _param_layers, png_dataset as _png_dataset, reference as _reference
from fp64_model import rel as _rel, sgd_step_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, D = 3.0, 5.0
EPS = 1e-5


@pytest.fixture(autouse=True)
def _algorithm_tables_restored():
    """(as tests/test_activations_gpu.py) the per-geometry implementation tables are left as a fresh process has them"""
    epoch = layer_mod.get_epoch()
    with ops.algorithms():
        yield
    layer_mod.set_epoch(epoch)


def _close(a, b, rtol=1e-3, atol=None):
    """the rule of tests/test_kernels_gpu.py"""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    if atol is None:
        atol = 1e-4 * float(b.abs().max()) + 1e-7
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), "max err %.3e (tol %.3e), %d/%d bad" % (float(err.max()), float(tol.min()), int(bad.sum()), bad.numel())


def _batch_stats(x, eps):
    xf = x.reshape(-1, x.shape[-1])
    mu = xf.mean(0)
    return mu, 1.0 / torch.sqrt(xf.var(0, unbiased=False) + eps)


def _draw_running(mu, inv, g, r_lim, d_lim, lo=0.2, hi=5.0, span=8.0, margin=1e-3):
    """running statistics (float32 values, as float64 tensors) such that (1 / inv_b) * stdinv spans lo .. hi and (mu_b - mean) *
    stdinv spans -span .. span; the first four channels are pinned beyond the four limits; a channel whose unclipped value lies
    within `margin` (relative) of a limit is drawn again, so that fp32 and fp64 agree about the side of every clip"""
    C = mu.shape[0]

    def draw(n):
        return (torch.exp(torch.empty(n, dtype=torch.float64).uniform_(math.log(lo), math.log(hi), generator=g)),
                torch.empty(n, dtype=torch.float64).uniform_(-span, span, generator=g))

    ratio, dval = draw(C)
    ratio[0], ratio[1], dval[2], dval[3] = 0.9 * hi, 1.1 * lo, 0.9 * span, -0.9 * span
    for _ in range(100):
        stdinv = (ratio * inv).float().double()
        mean = (mu - dval / stdinv).float().double()
        rv, dv = (1.0 / inv) * stdinv, (mu - mean) * stdinv            # what the float32 statistics really give
        near = ((rv / r_lim - 1).abs() < margin) | ((rv * r_lim - 1).abs() < margin) | ((dv.abs() / d_lim - 1).abs() < margin)
        if not bool(near.any()):
            break
        nr, nd = draw(int(near.sum()))
        ratio[near], dval[near] = nr, nd
    assert not bool(near.any())
    return mean, stdinv, rv, dv


def _assert_clip_coverage(rv, dv, r_lim, d_lim, quarter=True):
    free = (rv < r_lim) & (rv > 1 / r_lim) & (dv.abs() < d_lim)
    assert bool((rv > r_lim).any()) and bool((rv < 1 / r_lim).any()) and bool((dv > d_lim).any()) and bool((dv < -d_lim).any())
    assert int(free.sum()) >= (rv.numel() + 3) // 4 if quarter else int(free.sum()) >= 1, int(free.sum())


def _ref64(x, gamma, beta, mean, stdinv, r_max, d_max, eps, momentum, relu, res, dy):
    """the definition in float64 on the host -> dict of everything the device path produces"""
    x = x.double().cpu().requires_grad_(True)
    gamma = gamma.double().cpu().requires_grad_(True)
    beta = beta.double().cpu().requires_grad_(True)
    res = res.double().cpu().requires_grad_(True) if res is not None else None
    mean, stdinv = mean.double().cpu(), stdinv.double().cpu()
    mu, inv = _batch_stats(x, eps)
    r = torch.clamp((1.0 / inv) * stdinv, 1.0 / r_max, r_max).detach()
    d = torch.clamp((mu - mean) * stdinv, -d_max, d_max).detach()
    y = (x - mu) * (gamma * inv * r) + (beta + gamma * d)
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    out = {"y": y.detach(), "mu": mu.detach(), "inv": inv.detach(), "r": r, "d": d,
           "run_mean": momentum * mean + (1 - momentum) * mu.detach(), "run_stdinv": momentum * stdinv + (1 - momentum) * inv.detach()}
    if dy is not None:
        y.backward(dy.double().cpu())
        out.update(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=res.grad if res is not None else None)
    return out


def _case(shape, res, seed):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = torch.randn(shape, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + torch.randn(C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    rs = torch.randn(shape, generator=g) if res else None
    dy = torch.randn(shape, generator=g)
    mu, inv = _batch_stats(x.double(), EPS)
    mean, stdinv, rv, dv = _draw_running(mu, inv, g, R, D)
    return x, gamma, beta, rs, dy, mean.float(), stdinv.float(), rv, dv


SHAPES = [(3, 5, 7, 32), (4, 16, 16, 64), (2, 8, 8, 1536)]
MODES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("relu,res", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_vs_fp64(hip, shape, relu, res):
    """forward, statistics, r / d, the running update and the four gradients against float64; R = 3, D = 5, it = 0, channels
    clipped at both ends of r and of d and at least a quarter unclipped (asserted on the reference before the device runs).
    Tolerances: those of test_kernels_gpu.test_bn_fwd_bwd for the same passes"""
    mom = 0.9
    x, gamma, beta, rs, dy, mean, stdinv, rv, dv = _case(shape, res, 11 + shape[-1])
    r_max, d_max = renorm_limits(R, D, 0, 0)
    assert (r_max, d_max) == (R, D)
    _assert_clip_coverage(rv, dv, R, D)
    ref = _ref64(x, gamma, beta, mean, stdinv, r_max, d_max, EPS, mom, relu, rs, dy)
    assert bool((ref["r"] == R).any()) and bool((ref["r"] == 1 / R).any()) and bool((ref["d"] == D).any()) and bool((ref["d"] == -D).any())

    xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    rd = rs.cuda() if res else None
    rm, rsi = mean.cuda(), stdinv.cuda()
    y, sm, si, state = ops.bn_renorm_fwd_train(xd, gd, bd, rm, rsi, r_max, d_max, mom, EPS, relu=relu, res=rd)
    _close(y, ref["y"])
    _close(sm, ref["mu"])
    _close(si, ref["inv"])
    _close(state[0], ref["r"])
    _close(state[1], ref["d"])
    _close(state[2], gamma.double() * ref["r"])
    _close(state[3], beta.double() + gamma.double() * ref["d"])
    _close(rm, ref["run_mean"])
    _close(rsi, ref["run_stdinv"])
    dgamma, dbeta = torch.full((shape[-1],), 7.0).cuda(), torch.full((shape[-1],), 7.0).cuda()
    dx, dres, dg, db = ops.bn_renorm_bwd(xd, y if (relu and res) else None, dyd, sm, si, state, relu=relu, want_dres=res,
                                         dgamma=dgamma, dbeta=dbeta)
    assert dg is dgamma and db is dbeta
    _close(dx, ref["dx"], rtol=2e-3)
    _close(dgamma, ref["dgamma"], rtol=2e-3)
    _close(dbeta, ref["dbeta"], rtol=2e-3)
    if res:
        _close(dres, ref["dres"])
    else:
        assert dres is None


@pytest.mark.parametrize("relu,res", MODES)
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_closed_limits_equal_plain_batch_norm(hip, shape, relu, res):
    """R = 3, D = 5, it = 10 at epoch 0: r_max = 1, d_max = 0, the layer computes plain batch norm. Statistics bit for bit, values
    within the pair tests/test_kernels_gpu.py uses between two statistics routes"""
    mom = 0.9
    r_max, d_max = renorm_limits(R, D, 10, 0)
    assert (r_max, d_max) == (1.0, 0.0)
    x, gamma, beta, rs, dy, mean, stdinv, _, _ = _case(shape, res, 5 + shape[-1])
    xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    rd = rs.cuda() if res else None
    rm0, rs0 = mean.cuda(), stdinv.cuda()
    rm1, rs1 = mean.cuda(), stdinv.cuda()
    y0, sm0, si0 = ops.bn_fwd_train(xd, gd, bd, rm0, rs0, mom, EPS, relu=relu, res=rd)
    y1, sm1, si1, state = ops.bn_renorm_fwd_train(xd, gd, bd, rm1, rs1, r_max, d_max, mom, EPS, relu=relu, res=rd)
    assert torch.equal(sm0, sm1) and torch.equal(si0, si1) and torch.equal(rm0, rm1) and torch.equal(rs0, rs1)
    assert bool((state[0] == 1).all()) and bool((state[1] == 0).all())
    yy = y0 if (relu and res) else None
    dx0, dres0, dg0, db0 = ops.bn_bwd(xd, yy, dyd, gd, sm0, si0, relu=relu, want_dres=res, beta=bd)
    dx1, dres1, dg1, db1 = ops.bn_renorm_bwd(xd, y1 if (relu and res) else None, dyd, sm1, si1, state, relu=relu, want_dres=res)
    for a, b in ((y1, y0), (dx1, dx0), (dg1, dg0), (db1, db0)) + (((dres1, dres0),) if res else ()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), float((a - b).abs().max())


def _layer(shape_nhwc, momentum, r, d, it):
    N, H, W, C = shape_nhwc
    logical = (N, C, H, W)
    bn = BatchNormLayer([InitialLayer(Act(logical), logical)], momentum, EPS, r, d, it)
    for p in bn.params():
        p.dev = torch.from_numpy(p.to_dev_layout()).cuda()
        p.grad = torch.zeros_like(p.dev)
    return bn


def test_ordering_two_steps(hip):
    """two consecutive steps of one layer, momentum 0.5: step one's r / d are taken against the initial running statistics, step
    two's against the statistics AFTER step one's update - never against the ones the same launch is about to write"""
    shape, mom = (4, 8, 8, 64), 0.5
    x1, gamma, beta, _, dy, mean, stdinv, rv, dv = _case(shape, False, 23)
    x2 = _case(shape, False, 29)[0]
    bn = _layer(shape, mom, R, D, 0)
    assert bn.renorm_active
    bn.omega.set_value(gamma.numpy())
    bn.beta.set_value(beta.numpy())
    bn.mean.set_value(mean.numpy())
    bn.stdinv.set_value(stdinv.numpy())
    ref1 = _ref64(x1, gamma, beta, mean, stdinv, R, D, EPS, mom, False, None, None)
    ref2 = _ref64(x2, gamma, beta, ref1["run_mean"], ref1["run_stdinv"], R, D, EPS, mom, False, None, None)
    # what an implementation that clips against already-updated statistics would produce: far outside the tolerance below
    late1 = _ref64(x1, gamma, beta, ref1["run_mean"], ref1["run_stdinv"], R, D, EPS, mom, False, None, None)
    late2 = _ref64(x2, gamma, beta, ref2["run_mean"], ref2["run_stdinv"], R, D, EPS, mom, False, None, None)
    for good, late in ((ref1, late1), (ref2, late2)):
        assert float((good["r"] - late["r"]).abs().max()) > 0.05 and float((good["d"] - late["d"]).abs().max()) > 0.05
    layer_mod.set_train(True)
    layer_mod.set_epoch(0)
    got = []
    for x in (x1, x2):
        bn.input.data = x.cuda()
        bn.forward(None)
        got.append((bn._renorm_state[0].clone(), bn._renorm_state[1].clone(), bn.output.data.clone()))
    torch.cuda.synchronize()
    for (r, d, y), ref in zip(got, (ref1, ref2)):
        _close(r, ref["r"])
        _close(d, ref["d"])
        _close(y, ref["y"])
    _close(bn.mean.dev, ref2["run_mean"])
    _close(bn.stdinv.dev, ref2["run_stdinv"])


def test_bitwise_reproducible(hip):
    shape = (3, 5, 7, 32)
    x, gamma, beta, rs, dy, mean, stdinv, _, _ = _case(shape, True, 31)
    xd, gd, bd, dyd, rd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), rs.cuda()

    def once():
        rm, rsi = mean.cuda(), stdinv.cuda()
        y, sm, si, state = ops.bn_renorm_fwd_train(xd, gd, bd, rm, rsi, R, D, 0.9, EPS, relu=True, res=rd)
        dx, dres, dg, db = ops.bn_renorm_bwd(xd, y, dyd, sm, si, state, relu=True, want_dres=True)
        return [t.clone() for t in (y, dx, dg, db, dres, rm, rsi, state)]

    a, b = once(), once()
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)


# ------------------------------------------------------------------------------------------------- model level
# (no bias on the convolutions in front of the batch norms: its gradient is zero up to rounding, nothing to compare against)
STACK = "C[32,3] BN%s C[32,3] BN%s A P[2] RSN.O[64,3,2] R.C"
ON = "[0.9,1e-5,3,5,0]"
ON_PARAM = {"renormMaxR": 3.0, "renormMaxD": 5.0, "renormMaxIt": 0}
B, CLS, LR, MOM, DECAY = 4, 10, 0.1, 0.9, 0.0005


def _build(bn_args, bn_param):
    """batch norms away from (gamma, beta) = (1, 0), logits of order one (see tests/test_activations_gpu.py)"""
    m = build_model(STACK % (bn_args, bn_args), (3, 32, 32), B, CLS, spread_bn=True, head_scale=0.05)
    j = m.export_json()
    for l in j["layers"]:
        if l["type"] == "resnet" and bn_param:
            l["bnParam"] = dict(l["bnParam"], **bn_param)
    m2 = model_cnn.load_from_json(j, B)
    m2.class_num = CLS
    return m2


def _bns(model):
    return [l for l in model_cnn.walk_layers(model.layers) if l.type_name == "batchnorm" and l.enabled]


def _batch(seed=11):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    return x, cls, [{"image_class": int(c)} for c in cls]


def test_training_step_vs_fp64(hip, monkeypatch):
    """one SGD step of a stack with a renorm BN behind a convolution, a renorm `BN A` pair in front of a max pool and an RSN.O
    block whose bnParam carries the keys (projection shortcut: res + ReLU + want_dres on its last batch norm), running statistics
    drawn so that every layer has clipped and unclipped channels: cost, gradients, updates, running statistics and the test-mode
    output afterwards within the project's 1e-3 max-norm budget of a float64 autograd restatement"""
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        model = _build(ON, ON_PARAM)
        bns = _bns(model)
        assert len(bns) == 5 and all(l.renorm_active for l in bns)
        block = [l for l in model.layers if l.type_name == "resnet"][0]
        assert len(block.layers) > block.n_main and block.bn_json_param["renormMaxR"] == 3.0
        model.build_train_func("sgd")
        assert bns[1].act_fused and bns[1].pool_behind is not None          # the fusions it must decline are on offer
        x, cls, metas = _batch()
        before = _param_layers(model)
        weights = set(id(p) for l in model.layers for p in l.weights())
        values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}

        # running statistics: drawn layer by layer on the float64 restatement, rounded to float32, written into the layers
        g = torch.Generator().manual_seed(17)
        running = {}
        p0 = {k: [torch.from_numpy(v).double() for v in vs] for k, vs in values.items()}
        with torch.no_grad():
            _reference(model, x, p0, cls, True, running=running, draw=lambda mu, inv: _draw_running(mu, inv, g, R, D, margin=1e-2)[:2])
        for l in bns:
            l.mean.set_value(running[id(l)][0].numpy())
            l.stdinv.set_value(running[id(l)][1].numpy())
        params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
        cost_ref, _, steps = _reference(model, x, params, cls, True, running=running)
        cost_ref.backward()
        for l in bns:
            _assert_clip_coverage(steps[id(l)]["rv"], steps[id(l)]["dv"], R, D)

        seen = []
        fwd0 = ops.bn_renorm_fwd_train
        monkeypatch.setattr(ops, "bn_renorm_fwd_train", lambda *a, **k: (seen.append(k.get("pre") is not None), fwd0(*a, **k))[1])
        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
        torch.cuda.synchronize()
        assert len(seen) == 5 and all(seen), seen                           # every one behind a convolution: the producer's sums
        assert not any(getattr(l, "_pooled", False) for l in bns)

        e_cost = abs(cost - float(cost_ref.detach())) / abs(float(cost_ref.detach()))
        report, bad = [], []
        for l, p, e_g, e_p, _, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
            assert float(g_ref.abs().max()) > 0, (l.layer_index, p.name)
            report.append((e_g, e_p))
            if not (e_g <= 1e-3 and e_p <= 1e-3):
                bad.append("L%d %s %s: grad %.2e, update %.2e" % (l.layer_index, l.type_name, p.name, e_g, e_p))
        print("cost %.6f (float64 %.6f, %.2e), worst gradient %.2e, worst update %.2e over %d arrays" % (
            cost, float(cost_ref.detach()), e_cost, max(r[0] for r in report), max(r[1] for r in report), len(report)))
        assert e_cost <= 1e-3, (cost, float(cost_ref.detach()))
        assert not bad, bad
        after, e_run, e_rd = {}, 0.0, 0.0
        for l in bns:
            rm, rs = torch.from_numpy(l.mean.get_value().copy()).double(), torch.from_numpy(l.stdinv.get_value().copy()).double()
            e_run = max(e_run, _rel(rm, steps[id(l)]["run_mean"]), _rel(rs, steps[id(l)]["run_stdinv"]))
            e_rd = max(e_rd, _rel(l._renorm_state[0], steps[id(l)]["r"]), _rel(l._renorm_state[1], steps[id(l)]["d"]))
            after[id(l)] = (rm, rs)
        print("running statistics %.2e, r / d %.2e" % (e_run, e_rd))
        assert e_run <= 1e-3 and e_rd <= 1e-3

        # test mode afterwards: unchanged arithmetic, with the updated parameters and statistics (the drawn running statistics are
        # far from the batch's, so the soft-max may saturate: the logit map is the comparison that bites)
        now = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in before}
        with torch.no_grad():
            _, logits, _ = _reference(model, x, now, cls, False, running=after)
        pr_ref = torch.softmax(logits, dim=1)
        head = model.layers[-1].input
        for fold in (True, False):
            with ops.infer_fold(fold):
                pr = torch.from_numpy(model.predict_output_step(x)).double()
                z = head.data.view(B, -1)[:, :CLS].double().cpu()
            e_z, e_p = _rel(z, logits), float((pr - pr_ref).abs().max() / pr_ref.max())
            print("test mode (fold %s): logits %.2e, probabilities %.2e" % (fold, e_z, e_p))
            assert e_z <= 1e-3 and e_p <= 1e-3


def _symbols(ka):
    return [s for r in ka.table for s in r["fwd"] + r["bwd"]] + list(ka.other)


def _audited_step(model):
    model.build_train_func("sgd")
    x, cls, metas = _batch(3)
    with audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
    torch.cuda.synchronize()
    grads = [p.get_grad().copy() for _, ps in _param_layers(model) for p in ps]
    vals = [p.get_value().copy() for _, ps in _param_layers(model) for p in ps]
    stats = [p.get_value().copy() for l in _bns(model) for p in (l.mean, l.stdinv)]
    return cost, grads + vals + stats, _symbols(ka)


def test_inactive_stack_runs_none_of_the_new_kernels(hip):
    """R = 1, D = 0 written out (grammar and bnParam) against a stack built without the arguments: no renorm launch in the kernel
    audit, the step bit for bit the same"""
    off = _build("[0.9,1e-5,1,0,0]", {"renormMaxR": 1.0, "renormMaxD": 0.0, "renormMaxIt": 0})
    plain = _build("", None)
    assert not any(l.renorm_active for l in _bns(off)) and len(_bns(off)) == 5
    cost_a, arrays_a, sym_a = _audited_step(off)
    cost_b, arrays_b, sym_b = _audited_step(plain)
    assert sym_a and not [s for s in sym_a + sym_b if s in ops.RENORM_KERNELS]
    assert sym_a == sym_b
    assert math.isfinite(cost_a) and np.float32(cost_a).tobytes() == np.float32(cost_b).tobytes()
    assert len(arrays_a) == len(arrays_b) > 20
    for a, b in zip(arrays_a, arrays_b):
        assert a.tobytes() == b.tobytes()


def test_active_stack_runs_the_new_kernels_and_no_fusion(hip, monkeypatch):
    """the renorm-active stack under the default policy: one statistics-finish and one gradient-fold launch per layer, and none
    of the linked / pool-fused / producer-finished forms (every batch norm of the stack is renorm-active)"""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("ops.%s called for a renorm-active batch norm" % name)
        return f

    for name in ("bn_fwd_train_link", "bn_bwd_link", "bn_relu_pool_fwd_train", "bn_relu_pool_bwd_pooled", "bn_fwd_train", "bn_bwd"):
        monkeypatch.setattr(ops, name, refuse(name))
    model = _build(ON, ON_PARAM)
    link, final, sums = list(ops.LINK_COUNT), list(ops.FINAL_COUNT), list(ops.SUMS_COUNT)
    cost, _, sym = _audited_step(model)
    assert math.isfinite(cost)
    assert sym.count("bn_renorm_stats_finish_kernel") == 5 and sym.count("bn_renorm_grad_fold_kernel") == 5, sym
    assert (ops.LINK_COUNT, ops.FINAL_COUNT, ops.SUMS_COUNT) == (link, final, sums)
    assert not any(getattr(l, "_pooled", False) for l in _bns(model))


# ------------------------------------------------------------------------------------------------- command line
def test_cli_modify_train_predict(hip, tmp_path):
    """model-modify --modify-bn-renorm 3 5 10 on a small saved model, model-train for two epochs of three batches on it (the log
    line, the ramp at epoch 1, finite costs, the keys in the saved model), model-predict on the result and on the same weights
    with the keys stripped (model-modify --modify-bn-renorm 1 0 0). Each command in a child process of its own. model-predict in
    `single` mode writes nothing but its Top-1 / Top-5 lines, which are compared between the two child runs; the bit-for-bit part
    (inference ignores renorm) is checked IN THIS PROCESS, on the probabilities predict_output_step gives for the two files the
    commands wrote"""
    train_dir, test_dir, out = str(tmp_path / "train"), str(tmp_path / "test"), tmp_path / "out"
    _png_dataset(train_dir, seed=1)
    _png_dataset(test_dir, per_class=2, seed=2)
    out.mkdir()
    np.random.seed(7)
    m = model_cnn.ModelCNN()
    m.batch_size = 4
    m.class_num = 3
    m.build("C.B[32,3] BN A P[2] C[32,3] BNA RSN.O[64,3,2] P.A[8] R", (3, 32, 32), "relu", "half", ["he-backward"])
    src, ren = str(out / "plain.mdl.gz"), str(out / "renorm.mdl.gz")
    model_cnn.save_to_file(m, src)

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        log = r.stdout + r.stderr
        assert r.returncode == 0, (cmd[0], log[-3000:])
        return log

    run([os.path.join(ROOT, "bin", "model-modify"), "--input", src, "--output", ren, "--modify-bn-renorm", "3", "5", "10"])
    log = run([os.path.join(ROOT, "bin", "model-train"), "--model", ren, "--seed", "0", "--solver", "sgd", "--epochs", "2",
               "--batch-size", "4", "--train", train_dir, "--extension", "png", "--learn-rate", "0.05", "--learn-momentum", "0.9",
               "--learn-decay", "0.0005", "--output-prefix", str(out / "model")])
    lines = re.findall(r"batch renorm: (\d+) active layers, epoch (\d+) limits r_max=(\S+) d_max=(\S+)", log)
    assert [(int(n), int(e)) for n, e, _, _ in lines] == [(5, 0), (5, 1)], log[-3000:]
    assert (float(lines[0][2]), float(lines[0][3])) == (1.0, 0.0)
    assert float(lines[1][2]) == pytest.approx(3.0 ** 0.1, rel=1e-5) and float(lines[1][3]) == pytest.approx(6.0 ** 0.1 - 1, rel=1e-5)
    costs = [float(c) for c in re.findall(r"cost: (\S+) \(lr", log)]
    assert len(costs) >= 2 and all(math.isfinite(c) for c in costs), log[-3000:]
    final = sorted(glob.glob(str(out / "model_epoch*_final.mdl.gz")))[-1:]
    assert final and "epoch001" in final[0], os.listdir(str(out))
    trained = model_cnn.load_from_file(final[0], 4)
    act = [l for l in model_cnn.walk_layers(trained.layers) if isinstance(l, BatchNormLayer)]
    assert len(act) == 5 and all(l.renorm_active and (l.renorm_max_r, l.renorm_max_d, l.renorm_max_it) == (3.0, 5.0, 10) for l in act)
    j = trained.export_json()
    assert all(l["renormMaxR"] == 3.0 for l in j["layers"] if l["type"] in ("batchnorm", "batchnorm-relu"))
    assert [l["bnParam"]["renormMaxR"] for l in j["layers"] if l["type"] == "resnet"] == [3.0]
    # the running statistics moved away from their initial values: the training steps ran the layers
    assert any(not np.array_equal(a.mean.get_value(), np.zeros_like(a.mean.get_value())) for a in act)

    stripped = str(out / "stripped.mdl.gz")
    run([os.path.join(ROOT, "bin", "model-modify"), "--input", final[0], "--output", stripped, "--modify-bn-renorm", "1", "0", "0"])
    plain = model_cnn.load_from_file(stripped, 4)
    assert not any(l.renorm_active for l in model_cnn.walk_layers(plain.layers) if isinstance(l, BatchNormLayer))
    predict = [os.path.join(ROOT, "bin", "model-predict"), "--input", test_dir, "--extension", "png", "--batch-size", "4",
               "--predict-mode", "single", "--model"]
    rates = []
    for f in (final[0], stripped):
        rates.append(re.findall(r"Top\d - Error Rate: \S+", run(predict + [f])))
    assert len(rates[0]) == 2 and rates[0] == rates[1]
    x = np.random.RandomState(9).uniform(0.0, 1.0, (4, 3, 32, 32)).astype(np.float32)
    pr_a, pr_b = trained.predict_output_step(x), plain.predict_output_step(x)
    assert np.isfinite(pr_a).all() and pr_a.tobytes() == pr_b.tobytes()
