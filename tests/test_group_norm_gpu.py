"""Group normalisation on the device (csrc/gn.hip): `BN.G[g, eps]` / `BNA.G[g, eps]`, the JSON key
normGroups, `model-modify --modify-bn-groups`.

The reference has no such layer. The arbiter of the op is `torch.nn.functional.group_norm` in float64 (group_norm_reference.gn_ref64,
autograd for the gradients); whole models are held against group_norm_reference.reference. The tolerances of the op are those of
tests/test_kernels_gpu.py::test_bn_fwd_bwd for the same passes (`_close`: y, mu, inv, dres at rtol 1e-3; dx, dgamma, dbeta at 2e-3;
atol = 1e-4 * max |ref|), the model's the project's 1e-3 max-norm budget."""
import math

import numpy as np
import pytest
import torch

from denet_amd import layer as layer_mod
from denet_amd import ops
from denet_amd.layer import Act, InitialLayer
from denet_amd.layer.batch_norm import BatchNormLayer, group_norm_layers
from denet_amd.layer.convolution import ConvLayer
from denet_amd.model import audit, model_cnn, modify, update_bn
from group_norm_reference import build_model, gn_ref64, param_layers, reference, rel, relu_masks_of, sgd_step_errors

pytestmark = pytest.mark.gpu

EPS = 1e-5
WORST = {}


@pytest.fixture(autouse=True)
def _algorithm_tables_restored():
    """(as tests/test_bn_renorm_gpu.py) the per-geometry implementation tables are left as a fresh process has them"""
    with ops.algorithms():
        yield


def _close(a, b, rtol=1e-3, atol=None, name=None):
    """the rule of tests/test_kernels_gpu.py; the largest error relative to max |ref| is kept per quantity and printed"""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    if atol is None:
        atol = 1e-4 * float(b.abs().max()) + 1e-7
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    if name is not None:
        e = float(err.max()) / max(float(b.abs().max()), 1e-30)
        WORST[name] = max(WORST.get(name, 0.0), e)
        print("%s: max err %.3e of max |ref| %.3e (worst so far %.3e)" % (name, float(err.max()), float(b.abs().max()), WORST[name]))
    assert not bad.any(), "%s: max err %.3e (tol %.3e), %d/%d bad" % (name, float(err.max()), float(tol.min()), int(bad.sum()), bad.numel())


def _case(shape, res, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = torch.randn(shape, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + torch.randn(C, generator=g) + offset
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    rs = torch.randn(shape, generator=g) if res else None
    dy = torch.randn(shape, generator=g)
    return x, gamma, beta, rs, dy


def _run(x, gamma, beta, rs, dy, G, relu, recompute_mask=None):
    """forward + backward on the device; the mask from y where a residual was added (or recompute_mask is False), else from x"""
    xd, gd, bd, dyd = x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda()
    rd = rs.cuda() if rs is not None else None
    y, sm, si = ops.gn_fwd(xd, gd, bd, G, EPS, relu=relu, res=rd)
    C = x.shape[-1]
    dgamma, dbeta = torch.full((C,), 7.0).cuda(), torch.full((C,), 7.0).cuda()
    from_y = (relu and rs is not None) if recompute_mask is None else not recompute_mask
    dx, dres, dg, db = ops.gn_bwd(xd, y if from_y else None, dyd, gd, sm, si, G, relu=relu, want_dres=rs is not None,
                                  dgamma=dgamma, dbeta=dbeta, beta=bd)
    assert dg is dgamma and db is dbeta
    torch.cuda.synchronize()
    return {"y": y, "mu": sm, "inv": si, "dx": dx, "dres": dres, "dgamma": dgamma, "dbeta": dbeta}


def _check(got, ref, res):
    for k in ("y", "mu", "inv"):
        _close(got[k], ref[k], name=k)
    for k in ("dx", "dgamma", "dbeta"):
        _close(got[k], ref[k], rtol=2e-3, name=k)
    if res:
        _close(got["dres"], ref["dres"], name="dres")
    else:
        assert got["dres"] is None


SHAPES = [(2, 7, 9, 64, 32),        # Cg = 2, ragged rows
          (3, 5, 7, 96, 2),         # Cg = 48: a group straddles the 32-channel lines; odd N
          (2, 4, 4, 32, 1),         # layer norm
          (2, 16, 16, 64, 64),      # instance norm, Cg = 1
          (1, 1, 1, 32, 32),        # m = 1
          (1, 3, 3, 1536, 32),      # the widest head width
          (2, 40, 40, 64, 8),       # a sample spans several first-stage workgroups
          (4, 8, 8, 128, 32)]       # the common case
MODES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("relu,res", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_op_vs_fp64(hip, shape, relu, res):
    """forward, saved statistics and the four gradients against float64 F.group_norm + autograd"""
    N, H, W, C, G = shape
    x, gamma, beta, rs, dy = _case((N, H, W, C), res, 13 + C + G)
    ref = gn_ref64(x, gamma, beta, G, EPS, relu, rs, dy)
    got = _run(x, gamma, beta, rs, dy, G, relu)
    assert got["mu"].shape == (N, G) and got["inv"].shape == (N, G)
    _check(got, ref, res)
    if H * W * (C // G) == 1:
        # m = 1: var = 0, so y = beta (+ res, relu) and dx = 0 EXACTLY
        want = beta.reshape(1, 1, 1, C) + (rs if res else 0.0)
        want = torch.relu(want) if relu else want
        assert torch.equal(got["y"].cpu(), want.float()), float((got["y"].cpu() - want).abs().max())
        assert bool((got["dx"] == 0).all()), float(got["dx"].abs().max())
        assert torch.equal(got["mu"].cpu().reshape(-1), x.reshape(-1))
        assert bool((got["inv"].cpu() == np.float32(1.0 / math.sqrt(np.float64(np.float32(EPS))))).all())


@pytest.mark.parametrize("relu,res", MODES[1:])
def test_op_with_a_large_mean_vs_fp64(hip, relu, res):
    """x = 50 + randn: a one-pass float32 variance loses the variance to the square of the mean (E[x^2] ~ 2500 against var ~ 1:
    relative rounding 6e-8 * 2500 = 1.5e-4 of var per term, and worse once thousands of terms are summed); sums in double do not"""
    N, H, W, C, G = 2, 40, 40, 64, 8
    g = torch.Generator().manual_seed(3)
    x = 50.0 + torch.randn((N, H, W, C), generator=g)
    _, gamma, beta, rs, dy = _case((N, H, W, C), res, 5)
    ref = gn_ref64(x, gamma, beta, G, EPS, relu, rs, dy)
    assert float(ref["mu"].min()) > 49.0 and 0.9 < float(ref["inv"].min()) < 1.1
    _check(_run(x, gamma, beta, rs, dy, G, relu), ref, res)


# ------------------------------------------------------------------------------------------------- bit properties
BIT_SHAPES = [(3, 40, 40, 64, 8), (3, 5, 7, 96, 2), (3, 3, 3, 1536, 32)]
KEYS = ("y", "mu", "inv", "dx", "dres", "dgamma", "dbeta")


def test_two_runs_are_identical(hip):
    x, gamma, beta, rs, dy = _case((3, 40, 40, 64), True, 31)
    a, b = _run(x, gamma, beta, rs, dy, 8, True), _run(x, gamma, beta, rs, dy, 8, True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", BIT_SHAPES)
def test_a_sample_does_not_depend_on_its_batch(hip, shape):
    """sample 0 of an N = 3 batch == the same sample run at N = 1 (y, dx, dres, the saved statistics), and overwriting samples 1 and
    2 leaves sample 0's bits; in the middle of the batch too (sample 1 against its own N = 1 run)"""
    N, H, W, C, G = shape
    x, gamma, beta, rs, dy = _case((N, H, W, C), True, 37 + C)
    full = _run(x, gamma, beta, rs, dy, G, True)
    for n in (0, 1):
        one = _run(x[n:n + 1], gamma, beta, rs[n:n + 1], dy[n:n + 1], G, True)
        for k in ("y", "mu", "inv", "dx", "dres"):
            assert torch.equal(full[k][n:n + 1], one[k]), (n, k)
    x2, rs2, dy2 = x.clone(), rs.clone(), dy.clone()
    g = torch.Generator().manual_seed(53)
    x2[1:] = 100.0 * torch.randn(x2[1:].shape, generator=g) - 7.0
    rs2[1:] = 0.0
    dy2[1:] = torch.randn(dy2[1:].shape, generator=g)
    other = _run(x2, gamma, beta, rs2, dy2, G, True)
    for k in ("y", "mu", "inv", "dx", "dres"):
        assert torch.equal(full[k][:1], other[k][:1]), k
        assert not torch.equal(full[k][1:], other[k][1:]), k


@pytest.mark.parametrize("shape", BIT_SHAPES[:2])
def test_recomputed_mask_equals_the_mask_from_y(hip, shape):
    N, H, W, C, G = shape
    x, gamma, beta, _, dy = _case((N, H, W, C), False, 41 + C)
    a = _run(x, gamma, beta, None, dy, G, True, recompute_mask=True)
    b = _run(x, gamma, beta, None, dy, G, True, recompute_mask=False)
    assert bool((a["y"] == 0).any()) and bool((a["y"] > 0).any())
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k


def _layer(shape_nhwc, groups, relu=False):
    from denet_amd.layer.batch_norm_relu import BatchNormReluLayer
    N, H, W, C = shape_nhwc
    logical = (N, C, H, W)
    cls = BatchNormReluLayer if relu else BatchNormLayer
    bn = cls([InitialLayer(Act(logical), logical)], eps=EPS, norm_groups=groups)
    for p in bn.params():
        p.dev = torch.from_numpy(p.to_dev_layout()).cuda()
        p.grad = torch.zeros_like(p.dev)
    return bn


@pytest.mark.parametrize("relu", [False, True])
def test_test_mode_gives_the_bits_of_training_mode(hip, relu):
    """one op for both modes; the running statistics are neither read nor written by either"""
    shape = (3, 5, 7, 64)
    x, gamma, beta, _, _ = _case(shape, False, 43)
    bn = _layer(shape, 16, relu)
    bn.omega.set_value(gamma.numpy())
    bn.beta.set_value(beta.numpy())
    bn.mean.set_value(np.full(64, 3.0, np.float32))
    bn.stdinv.set_value(np.full(64, 0.25, np.float32))
    out = []
    try:
        for train in (True, False):
            layer_mod.set_train(train)
            bn.input.data = x.cuda()
            bn.forward(None)
            out.append(bn.output.data.clone())
    finally:
        layer_mod.set_train(True)
    assert torch.equal(out[0], out[1])
    _close(out[0], gn_ref64(x, gamma, beta, 16, EPS, relu)["y"])
    assert bool((bn.mean.dev == 3.0).all()) and bool((bn.stdinv.dev == 0.25).all())


# ------------------------------------------------------------------------------------------------- layer and model
# a `BN.G A` pair in front of a max pool (the fusions a group-mode layer declines are on offer), a fused `BNA.G` behind a stride-2
# convolution, a pre-activation block that takes the mode through its bnParam
STACK = "C[32,3] BN.G[8] A P[2] C[64,3,2] BNA.G[32] RSN[64,3] P.A[4] R"
MIXED = "C[32,3] BN A P[2] C[64,3,2] BNA.G[32] RSN[64,3] P.A[4] R"
B, CLS, LR, MOM, DECAY = 3, 10, 0.02, 0.0, 0.0005
BLOCK_GROUPS = 16


def _build(desc=STACK, seed=5):
    m = build_model(desc, (3, 16, 16), B, CLS, seed=seed, spread_bn=True, head_scale=0.05)
    j = m.export_json()
    for l in j["layers"]:
        if l["type"] == "resnet":
            l["bnParam"] = dict(l["bnParam"], normGroups=BLOCK_GROUPS)
    m2 = model_cnn.load_from_json(j, B)
    m2.class_num = CLS
    m2.class_labels = {"c%i" % i: i for i in range(CLS)}
    rng = np.random.RandomState(seed + 2)
    for l in group_norm_layers(m2):          # (spread_bn reaches `batchnorm` layers only: the fused one and the block's too)
        l.omega.set_value(rng.uniform(0.7, 1.3, l.omega.value.shape))
        l.beta.set_value(rng.normal(0.0, 0.3, l.beta.value.shape))
    return m2


def _batch(seed=11):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (B, 3, 16, 16)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    return x, cls, [{"image_class": int(c)} for c in cls]


def _norms(model):
    return [l for l in model_cnn.walk_layers(model.layers) if isinstance(l, BatchNormLayer) and l.enabled]


def _symbols(ka):
    return [s for r in ka.table for s in r["fwd"] + r["bwd"]] + list(ka.other)


def _refuse(monkeypatch, names):
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("ops.%s called in a model whose norms are all in group mode" % name)
        return f
    for name in names:
        monkeypatch.setattr(ops, name, refuse(name))


BN_ROUTES = ("bn_fwd_train", "bn_fwd_train_link", "bn_bwd", "bn_bwd_link", "bn_relu_pool_fwd_train", "bn_relu_pool_bwd_pooled",
             "bn_renorm_fwd_train", "bn_renorm_bwd", "bn_fwd_test", "bn_fold")


def test_training_steps_vs_fp64(hip, monkeypatch):
    """two SGD steps of the stack: cost, every gradient and every update against the float64 restatement inside 1e-3 (max norm), the
    ReLU decisions taken from the device; the launch trace holds the six gn_* kernels once per layer and none of the batch-norm
    routes runs (statistics, link, pool-fused, producer-finished); the running statistics are left untouched"""
    model = _build()
    norms = _norms(model)
    assert [l.norm_groups for l in norms] == [8, 32, BLOCK_GROUPS, BLOCK_GROUPS] and len(group_norm_layers(model)) == 4
    model.build_train_func("sgd")
    assert norms[0].act_fused and norms[0].pool_behind is None and model.layers[4].type_name == "pool"
    _refuse(monkeypatch, BN_ROUTES)
    weights = set(id(p) for l in model_cnn.walk_layers(model.layers) for p in l.weights())
    counts = list(ops.LINK_COUNT), list(ops.FINAL_COUNT), list(ops.SUMS_COUNT)
    for it, seed in enumerate((11, 12)):          # (no momentum: each step is a first step; another batch for the second)
        x, cls, metas = _batch(seed)
        before = param_layers(model)
        assert sum(l.type_name != "conv" for l, _ in before) == 4
        values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, it, LR, [MOM], DECAY)
            torch.cuda.synchronize()
        sym = _symbols(ka)
        for name in ops.GN_KERNELS:
            assert sym.count(name) == 4, (name, sym)
        assert not [s for s in sym if s.startswith("bn_")], sym
        masks = relu_masks_of(model)
        params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
        flips = {}
        cost_ref, _, _ = reference(model, x, params, cls, True, relu_masks=masks, flips=flips)
        cost_ref.backward()
        print("step %d: cost %.6f (float64 %.6f); ReLU decisions that differ: %s" % (it, cost, float(cost_ref.detach()),
                                                                                    {k: v for k, v in flips.items() if v}))
        assert cost > 0.1 and abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach()))
        report, bad = [], []
        for l, p, e_g, e_p, _, g_ref in sgd_step_errors(before, values, params, weights, LR, DECAY):
            assert float(g_ref.abs().max()) > 0, (l.layer_index, p.name)
            report.append("step %d L%d %s %s: grad %.2e, update %.2e" % (it, l.layer_index, l.type_name, p.name, e_g, e_p))
            if not (e_g <= 1e-3 and e_p <= 1e-3):
                bad.append(report[-1])
        print("\n".join(report))
        assert not bad, bad
    assert (list(ops.LINK_COUNT), list(ops.FINAL_COUNT), list(ops.SUMS_COUNT)) == counts
    for l in norms:
        assert not l.mean.get_value().any() and bool((l.stdinv.get_value() == 1).all())


def test_inference_save_load_and_modify(hip, tmp_path, monkeypatch):
    """predict_output_step of the stack against float64; no convolution is folded with the norm behind it and the gn_* forward
    kernels run once per layer; save -> load -> the same predictions bit for bit; --modify-bn-groups switches a plain model over
    and back (0: the plain model's bits again)"""
    model = _build()
    model.build_train_func("sgd")
    x, cls, _ = _batch(21)
    assert ops.INFER_FOLD
    folded = []
    f0 = ConvLayer.forward_folded
    monkeypatch.setattr(ConvLayer, "forward_folded", lambda self, *a, **k: (folded.append(self), f0(self, *a, **k))[1])
    for name in BN_ROUTES:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError("ops." + _n)))
    with audit.KernelAudit(model) as ka:
        pr = model.predict_output_step(x)
        torch.cuda.synchronize()
    sym = _symbols(ka)
    assert not folded
    for name in ops.GN_FWD_KERNELS:
        assert sym.count(name) == 4, (name, sym)
    assert not [s for s in sym if s in ops.GN_BWD_KERNELS]
    vals = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in param_layers(model)}
    with torch.no_grad():
        _, logits, _ = reference(model, x, vals, cls, False)
    pr_ref = torch.softmax(logits, dim=1)
    e = float((torch.from_numpy(pr).double() - pr_ref).abs().max()) / float(pr_ref.max())
    print("test-mode probabilities: %.2e (largest %.3f)" % (e, float(pr_ref.max())))
    assert pr.shape == (B, CLS) and e <= 1e-3
    with ops.infer_fold(False):
        assert np.array_equal(model.predict_output_step(x).view(np.int32), pr.view(np.int32))

    path = str(tmp_path / "gn.mdl.gz")
    model_cnn.save_to_file(model, path)
    again = model_cnn.load_from_file(path, B)
    assert [l.norm_groups for l in _norms(again)] == [8, 32, BLOCK_GROUPS, BLOCK_GROUPS]
    again.build_train_func("sgd")
    assert np.array_equal(again.predict_output_step(x).view(np.int32), pr.view(np.int32))
    monkeypatch.undo()

    # --modify-bn-groups on a plain model: every norm in the mode, predictions those of the float64 group norm; 0 goes back
    plain = build_model(STACK.replace(".G[8]", "").replace(".G[32]", ""), (3, 16, 16), B, CLS, seed=5, spread_bn=True, head_scale=0.05)
    pr_plain = plain.predict_output_step(x)
    on = modify.modify_bn_groups(plain, 16)
    assert [l.norm_groups for l in _norms(on)] == [16] * 4
    vals = {id(l): [torch.from_numpy(p.get_value().copy()).double() for p in ps] for l, ps in param_layers(on)}
    with torch.no_grad():
        _, logits, _ = reference(on, x, vals, cls, False)
    pr_on, pr_on_ref = on.predict_output_step(x), torch.softmax(logits, dim=1)
    assert float((torch.from_numpy(pr_on).double() - pr_on_ref).abs().max()) / float(pr_on_ref.max()) <= 1e-3
    assert not np.array_equal(pr_on, pr_plain)
    off = modify.modify_bn_groups(on, 0)
    assert np.array_equal(off.predict_output_step(x).view(np.int32), pr_plain.view(np.int32))


def test_mixed_model_keeps_the_plain_layers_routes(hip, monkeypatch):
    """one plain `BN A` in front of the max pool, the rest in group mode: the plain layer still runs its pool-fused pass on the
    producer's sums, is folded into its convolution in inference, and is the only layer model-update-bn touches"""
    model = _build(MIXED)
    norms = _norms(model)
    assert [l.norm_groups for l in norms] == [0, 32, BLOCK_GROUPS, BLOCK_GROUPS]
    model.build_train_func("sgd")
    plain = norms[0]
    assert plain.act_fused and plain.pool_behind is not None and plain.input.stats_bn is plain
    pooled = []
    p0 = ops.bn_relu_pool_fwd_train
    monkeypatch.setattr(ops, "bn_relu_pool_fwd_train", lambda *a, **k: (pooled.append(k.get("pre") is not None), p0(*a, **k))[1])
    x, cls, metas = _batch(11)
    before = param_layers(model)
    values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}
    weights = set(id(p) for l in model_cnn.walk_layers(model.layers) for p in l.weights())
    with audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, LR, [MOM], DECAY)
        torch.cuda.synchronize()
    sym = _symbols(ka)
    assert len(pooled) == 1 and plain._pooled
    for name in ops.GN_KERNELS:
        assert sym.count(name) == 3, (name, sym)
    masks = relu_masks_of(model)
    assert id(plain.act_behind) not in masks     # (the pool-fused pass never writes relu(bn(x)): the host takes its own decisions)
    params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
    cost_ref, _, stats = reference(model, x, params, cls, True, relu_masks=masks)
    cost_ref.backward()
    assert abs(cost - float(cost_ref.detach())) <= 1e-3 * abs(float(cost_ref.detach()))
    for l, p, e_g, e_p, _, _ in sgd_step_errors(before, values, params, weights, LR, DECAY):
        assert e_g <= 1e-3 and e_p <= 1e-3, (l.layer_index, l.type_name, p.name, e_g, e_p)
    assert rel(plain.mean.get_value(), (1.0 - plain.momentum) * stats[id(plain)]["mean"]) <= 1e-3
    for l in norms[1:]:
        assert not l.mean.get_value().any() and bool((l.stdinv.get_value() == 1).all())

    # inference: the plain pair is folded into its convolution, the convolutions in front of the group norms are not
    folded = []
    f0 = ConvLayer.forward_folded
    monkeypatch.setattr(ConvLayer, "forward_folded", lambda self, *a, **k: (folded.append(self), f0(self, *a, **k))[1])
    pr = model.predict_output_step(x)
    assert folded == [model.layers[1]] and np.isfinite(pr).all()

    # model-update-bn: only the plain layer's statistics move, and the group-mode layers are listed as skipped
    lines = []
    old = {id(l): (l.mean.get_value().copy(), l.stdinv.get_value().copy()) for l in norms}
    gb = {id(l): (l.omega.get_value().copy(), l.beta.get_value().copy()) for l in norms}
    out = update_bn.update_bn(model, [_batch(31)[0], _batch(32)[0]], log=lines.append)
    assert [o[0] for o in out] == [plain]
    assert sum("group norm" in s and s.startswith("Skipping") for s in lines) == 3
    assert not np.array_equal(plain.mean.get_value(), old[id(plain)][0]) and not np.array_equal(plain.stdinv.get_value(), old[id(plain)][1])
    for l in norms:
        assert np.array_equal(l.omega.get_value(), gb[id(l)][0]) and np.array_equal(l.beta.get_value(), gb[id(l)][1])
    for l in norms[1:]:
        assert np.array_equal(l.mean.get_value(), old[id(l)][0]) and np.array_equal(l.stdinv.get_value(), old[id(l)][1])


def test_ema_and_an_unreachable_clip_leave_the_step(hip):
    """model.ema_decay on and a gradient-clip limit the norm never reaches: parameters, momentum and statistics after two steps are
    bit for bit the plain run's (gamma / beta of a group norm are ordinary trained biases to both features)"""
    def two_steps(model):
        model.build_train_func("sgd")
        for it, seed in enumerate((11, 12)):
            x, _, metas = _batch(seed)
            model.train_step(x, metas, 0, it, LR, [0.9], DECAY)
        torch.cuda.synchronize()
        return [t.clone() for t in (model.P, model.M, model.S)]

    base = two_steps(_build())
    other = _build()
    other.ema_decay = 0.9
    other.gradient_clip = 1e30
    got = two_steps(other)
    for a, b in zip(got, base):
        assert a.numel() == b.numel() and torch.equal(a, b)
    assert not torch.equal(base[1], torch.zeros_like(base[1]))
