"""tests/fp64_model.py checked against itself on models built on the host (no device): the yardstick of the whole-step GPU tests must
not be wrong in a way those tests cannot see. The models are the ones the GPU files run, at B = 2 (the batch norms at the 1 x 1 maps
need more than one sample per channel)."""
import numpy as np
import pytest
import torch

import fp64_model
from denet_amd.model import model_cnn, zoo
from fp64_model import build_model, param_layers, reference, rel

B, CLS = 2, 10
RENORM = "[0.9,1e-5,3,5,0]"
# name: (desc, data shape, border mode, activation)
MODELS = {
    "simple-cifar10": (zoo.SIMPLE_CIFAR10_DESC, (3, 32, 32), "same", "relu"),
    "activations": ("C.B[32,3] A C[32,3] BN A P[2] nRSN.O[2,64,3,2] nRSN[2,64,3,2,32] R.C", (3, 32, 32), "half", "elu"),
    "renorm": ("C[32,3] BN%s C[32,3] BN%s A P[2] RSN.O[64,3,2] R.C" % (RENORM, RENORM), (3, 32, 32), "half", "relu"),
    "rectangular": ("C.B[32,3] BN A C.X[64,1,7] BN A C.X[64,7,1,2,1] BN A DC.X[32,3,1,2,1] C.X[32,3,3,1,2] BN A R", (3, 16, 24), "half",
                    "relu"),
    "border pool": ("C.B[32,7,2] P.B[3,2] R", (3, 32, 32), "half", "relu"),
    "average border pool": ("C.B[32,3] P.AB[2] R", (3, 15, 15), "half", "relu"),
}


def _model(name, seed=5):
    desc, shape, border, activation = MODELS[name]
    return build_model(desc, shape, B, CLS, activation, border, seed=seed, spread_bn=True, head_scale=0.05)


def _batch(model, seed=11):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, (B,) + tuple(model.data_shape)).astype(np.float32), rng.randint(0, CLS, B)


def _params(model, grad=True):
    return {id(l): [torch.from_numpy(p.get_value().copy()).double().requires_grad_(grad) for p in ps] for l, ps in param_layers(model)}


def _dropout(model, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {id(l): (torch.rand(l.input_shape, generator=g, dtype=torch.float64) >= l.dropout_rate).double() / (1.0 - l.dropout_rate)
            for l in model.layers if l.type_name == "dropout"}


def _bns(model):
    return [l for l in model_cnn.walk_layers(model.layers) if l.type_name == "batchnorm" and l.enabled]


def _initial_running(model):
    return {id(l): (torch.zeros(l.output_shape[1], dtype=torch.float64), torch.ones(l.output_shape[1], dtype=torch.float64))
            for l in _bns(model)}


@pytest.mark.parametrize("name", list(MODELS))
def test_every_layer_has_its_declared_shape_in_both_modes(name):
    """reference() asserts every layer's output shape against the layer's own; train and test mode, finite cost, gradients for all"""
    model = _model(name)
    x, cls = _batch(model)
    params = _params(model)
    cost, logits, stats = reference(model, x, params, cls, True, running=_initial_running(model), masks=_dropout(model))
    assert tuple(logits.shape) == (B, CLS) and bool(torch.isfinite(cost))
    cost.backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for ts in params.values() for t in ts)
    assert set(stats) == set(id(l) for l in _bns(model))
    after = {k: (s["run_mean"], s["run_stdinv"]) for k, s in stats.items()}
    with torch.no_grad():
        cost2, logits2, stats2 = reference(model, x, _params(model, grad=False), cls, False, running=after)
    assert tuple(logits2.shape) == (B, CLS) and bool(torch.isfinite(cost2)) and stats2 == {}


def _own_relu_decisions(monkeypatch, model, x, cls, masks):
    """{id(activation layer): the sign decisions of the reference's own training-mode pass}: act64 is wrapped for one pass, and its
    calls are matched to the layers in the order reference() runs them (a block's sub-layers, then the block's own exit)"""
    def order(l):
        if l.type_name == "activation":
            return [l]
        if l.type_name == "resnet":
            return [a for s in l.layers for a in order(s)] + ([] if "pre-activation" in l.version else [l])
        return []

    calls = []
    inner = fp64_model.act64
    monkeypatch.setattr(fp64_model, "act64", lambda name, h: (calls.append(h.detach() > 0), inner(name, h))[1])
    with torch.no_grad():
        cost, _, _ = reference(model, x, _params(model, False), cls, True, running=_initial_running(model), masks=masks)
    monkeypatch.setattr(fp64_model, "act64", inner)
    layers = [a for l in model.layers for a in order(l)]
    assert len(layers) == len(calls)
    return cost, {id(l): m for l, m in zip(layers, calls) if l.type_name == "activation"}


@pytest.mark.parametrize("name", ["simple-cifar10", "rectangular", "renorm"])
def test_teacher_forcing_its_own_relu_decisions_changes_nothing(monkeypatch, name):
    """the ReLU decisions of the reference itself, handed back as relu_masks: no element flips, and the cost is the same bits"""
    model = _model(name)
    x, cls = _batch(model)
    masks = _dropout(model)
    cost, own = _own_relu_decisions(monkeypatch, model, x, cls, masks)
    assert own and any(bool((~m).any()) for m in own.values()) and any(bool(m.any()) for m in own.values())
    flips = {}
    with torch.no_grad():
        forced, _, _ = reference(model, x, _params(model, False), cls, True, running=_initial_running(model), masks=masks,
                                 relu_masks=own, flips=flips)
    assert set(flips) == set(own) and not any(flips.values()), flips
    assert float(forced) == float(cost)
    # and the counter counts: one decision turned over is one flip in that layer (the layers behind see another tensor)
    k = next(iter(own))
    turned = dict(own)
    turned[k] = own[k].clone()
    turned[k].view(-1)[0] = not bool(own[k].view(-1)[0])
    with torch.no_grad():
        reference(model, x, _params(model, False), cls, True, running=_initial_running(model), masks=masks, relu_masks=turned, flips=flips)
    assert flips[k] == 1


def test_closed_renorm_limits_are_plain_batch_norm():
    """r_max = 1, d_max = 0 written out: cost and every gradient as the stack built without the arguments, to 1e-12"""
    desc = "C[32,3] BN%s C[32,3] BN%s A P[2] RSN.O[64,3,2] R.C"
    plain = build_model(desc % ("", ""), (3, 32, 32), B, CLS, spread_bn=True, head_scale=0.05)
    closed = build_model(desc % ("[0.9,1e-5,1,0,0]", "[0.9,1e-5,1,0,0]"), (3, 32, 32), B, CLS, spread_bn=True, head_scale=0.05)
    x, cls = _batch(plain)
    g = torch.Generator().manual_seed(2)
    results = []
    for model, with_running in ((plain, False), (closed, True)):
        params = _params(model)
        running = None
        if with_running:        # far from the batch's statistics: open limits would clip and correct, closed ones must not look at them
            running = {id(l): (torch.randn(l.output_shape[1], generator=g, dtype=torch.float64),
                               torch.rand(l.output_shape[1], generator=g, dtype=torch.float64) + 0.5) for l in _bns(model)}
        cost, _, stats = reference(model, x, params, cls, True, running=running)
        cost.backward()
        if with_running:
            assert all(bool((s["r"] == 1).all()) and bool((s["d"] == 0).all()) and bool((s["rv"] != 1).any()) for s in stats.values())
        results.append((cost.detach(), [t.grad for l, _ in param_layers(model) for t in params[id(l)]]))
    (cost_a, grads_a), (cost_b, grads_b) = results
    assert abs(float(cost_a) - float(cost_b)) <= 1e-12 * abs(float(cost_a))
    assert len(grads_a) == len(grads_b) > 5
    for a, b in zip(grads_a, grads_b):
        assert rel(b, a) <= 1e-12


def test_open_renorm_limits_differ_from_plain_batch_norm():
    """the counterpart: with open limits and running statistics away from the batch's, r and d are not (1, 0) and the cost moves"""
    model = _model("renorm")
    x, cls = _batch(model)
    g = torch.Generator().manual_seed(2)
    running = {id(l): (torch.randn(l.output_shape[1], generator=g, dtype=torch.float64),
                       torch.rand(l.output_shape[1], generator=g, dtype=torch.float64) + 0.5) for l in _bns(model)}
    with torch.no_grad():
        cost, _, stats = reference(model, x, _params(model, False), cls, True, running=running)
        plain, _, _ = reference(model, x, _params(model, False), cls, True)
    active = [l for l in _bns(model) if l.renorm_active]          # (the block's own batch norms are plain: the grammar has no slot)
    assert len(active) == 2 and len(stats) == 5
    for s in [stats[id(l)] for l in active]:
        assert bool((s["r"] != 1).any()) and bool((s["d"] != 0).any())
        assert float(s["r"].max()) <= 3.0 and float(s["r"].min()) >= 1 / 3.0 and float(s["d"].abs().max()) <= 5.0
        assert torch.equal(s["r"], torch.clamp(s["rv"], 1 / 3.0, 3.0)) and torch.equal(s["d"], torch.clamp(s["dv"], -5.0, 5.0))
    assert abs(float(cost) - float(plain)) > 1e-3 * abs(float(plain))


@pytest.mark.parametrize("name", ["simple-cifar10", "activations", "rectangular"])
def test_running_update_from_the_initial_statistics(name):
    """running statistics (0, 1): run_mean = (1 - m) * mean and run_stdinv = m + (1 - m) * stdinv, the forms the GPU tests write"""
    model = _model(name)
    x, cls = _batch(model)
    with torch.no_grad():
        _, _, stats = reference(model, x, _params(model, False), cls, True, running=_initial_running(model), masks=_dropout(model))
    bns = _bns(model)
    assert bns
    for l in bns:
        s = stats[id(l)]
        assert torch.equal(s["run_mean"], (1 - l.momentum) * s["mean"])
        assert rel(s["run_stdinv"], l.momentum + (1 - l.momentum) * s["stdinv"]) <= 1e-15
        assert bool((s["r"] == 1).all()) and bool((s["d"] == 0).all())


def test_an_unknown_layer_kind_raises():
    model = _model("border pool")
    x, cls = _batch(model)
    model.layers[2].type_name = "pool-of-another-kind"          # (an instance attribute over the class's)
    with pytest.raises(AssertionError, match="unexpected layer pool-of-another-kind"):
        reference(model, x, _params(model, False), cls, True)
