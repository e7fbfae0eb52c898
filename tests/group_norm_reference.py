"""Group normalisation restated in float64 on the host. A helper module: it holds no test.

The contract is DESIGN.md section 21: x NHWC [N][H*W][C], G groups of Cg = C / G consecutive channels, statistics per sample and
group (biased variance, eps inside the root), y = (x - mu) * inv * gamma[c] + beta[c] [+ res] [relu], the same in training and
inference. The ARBITER of the op is `torch.nn.functional.group_norm` in float64 on NCHW views, the gradients by autograd
(gn_ref64). `gn_closed_form` is the issue's closed-form backward written out in numpy float64 - the formula the kernels implement -
which the host test holds against autograd. For whole models `reference` restates the few layer kinds the small test models use
(conv, norm in either mode, activation, pool, resnet, regression), wired and keyed by id(layer) like fp64_model.reference, which
computes every `batchnorm` as a batch norm and so cannot serve."""
import numpy as np
import torch
import torch.nn.functional as Fn

from denet_amd.model import model_cnn
from fp64_model import act64, build_model, rel, sgd_step_errors  # noqa: F401 (re-exported)

NORMS = ("batchnorm", "batchnorm-relu")


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def gn_ref64(x, gamma, beta, groups, eps, relu=False, res=None, dy=None):
    """x, res, dy: NHWC [N, H, W, C] tensors of any float dtype. Returns a dict of float64 tensors: y, mu / inv [N, groups], and with
    dy also dx, dgamma, dbeta, dres (None without res)"""
    x = x.detach().double().cpu().requires_grad_(True)
    gamma = gamma.detach().double().cpu().requires_grad_(True)
    beta = beta.detach().double().cpu().requires_grad_(True)
    res = res.detach().double().cpu().requires_grad_(True) if res is not None else None
    N, C = x.shape[0], x.shape[-1]
    xn = _nchw(x)
    if x.numel() // C == 1:
        # F.group_norm's Python wrapper refuses a single value per channel ("when training": a check it shares with batch norm);
        # the operator it calls has no such limit, and the m = 1 edge of the contract lives exactly there
        y = _nhwc(torch.native_group_norm(xn.contiguous(), gamma, beta, N, C, 1, groups, eps)[0])
    else:
        y = _nhwc(Fn.group_norm(xn, groups, gamma, beta, eps))
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    xg = _nchw(x.detach()).reshape(N, groups, -1)
    mu = xg.mean(dim=2)
    out = {"y": y.detach(), "mu": mu, "inv": 1.0 / torch.sqrt(xg.var(dim=2, unbiased=False) + eps)}
    if dy is not None:
        y.backward(dy.detach().double().cpu())
        out.update(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=res.grad if res is not None else None)
    return out


def gn_closed_form(x, gamma, beta, groups, eps, relu=False, res=None, dy=None):
    """the contract's formulas in numpy float64 on [N][P][C] arrays (P = H * W); the ReLU mask from y. Returns the same dict"""
    x = np.asarray(x, np.float64)
    N, C = x.shape[0], x.shape[-1]
    shape = x.shape
    x = x.reshape(N, -1, C)
    P, Cg = x.shape[1], C // groups
    m = P * Cg
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    xg = x.reshape(N, P, groups, Cg)
    mu = xg.sum(axis=(1, 3)) / m
    var = ((xg - mu[:, None, :, None]) ** 2).sum(axis=(1, 3)) / m
    inv = 1.0 / np.sqrt(var + eps)
    mu_c, inv_c = np.repeat(mu, Cg, axis=1)[:, None, :], np.repeat(inv, Cg, axis=1)[:, None, :]      # [N, 1, C]
    xhat = (x - mu_c) * inv_c
    y = xhat * gamma + beta
    if res is not None:
        y = y + np.asarray(res, np.float64).reshape(N, P, C)
    if relu:
        y = np.maximum(y, 0.0)
    out = {"y": y.reshape(shape), "mu": mu, "inv": inv}
    if dy is not None:
        g = np.asarray(dy, np.float64).reshape(N, P, C)
        if relu:
            g = g * (y > 0)
        A, B = g.sum(axis=1), (g * xhat).sum(axis=1)                                                  # [N, C]
        S1 = (gamma * A).reshape(N, groups, Cg).sum(axis=2)
        S2 = (gamma * B).reshape(N, groups, Cg).sum(axis=2)
        S1c, S2c = np.repeat(S1, Cg, axis=1)[:, None, :], np.repeat(S2, Cg, axis=1)[:, None, :]
        dx = inv_c * (gamma * g - S1c / m - xhat * S2c / m)
        out.update(dx=dx.reshape(shape), dgamma=B.sum(axis=0), dbeta=A.sum(axis=0), dres=g.reshape(shape) if res is not None else None)
    return out


# ------------------------------------------------------------------------------------------------- whole models
def _per_channel(v):
    return v[None, :, None, None]


def param_layers(model):
    """[(layer, [its trained parameters])] of the convolutions and the enabled norms of both kinds, nested ones included"""
    out = []
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name == "conv":
            out.append((l, [l.omega] + ([l.beta] if l.use_bias else [])))
        elif l.type_name in NORMS and l.enabled:
            out.append((l, [l.omega, l.beta]))
    return out


def relu_masks_of(model):
    """{id(layer): the ReLU decisions of the last forward pass, [N, C, H, W] bool on the host} of the activation layers, the fused
    `batchnorm-relu` layers and the exits of `original` blocks, from the tensors the forward pass left. A ReLU whose output the
    pass never wrote (a plain `BN A` fused with the max pool behind it) has no entry: the host takes its own decisions there"""
    out = {}
    for l in model_cnn.walk_layers(model.layers):
        relu_exit = l.type_name == "resnet" and "pre-activation" not in l.version and l.activation in ("relu", "relu-safe")
        if l.type_name in ("activation", "batchnorm-relu") or relu_exit:
            d = l.output._data
            if d is None:
                continue
            out[id(l)] = (d[..., :l.output_shape[1]] > 0).permute(0, 3, 1, 2).cpu()
    return out


def reference(model, x, params, cls, train, running=None, relu_masks=None, flips=None):
    """the layer list in float64. params[id(layer)]: filter[, bias] of a conv, (gamma, beta) of a norm. A norm with norm_groups > 0
    is a group norm in both modes; any other is a batch norm: batch statistics in training, running[id(layer)] = (mean, stdinv)
    in test mode (eps twice, as the layer does). relu_masks / flips as in fp64_model.reference, also for `batchnorm-relu` layers and
    block exits. Returns (cost, logits, stats); a layer kind that is not restated here raises"""
    val = {id(model.layers[0].output): torch.from_numpy(x).double()}
    stats = {}

    def relu(l, h):
        if relu_masks is not None and id(l) in relu_masks:
            m = relu_masks[id(l)].double()
            if flips is not None:
                flips[id(l)] = int(((h.detach() > 0).double() != m).sum())
            return h * m
        return torch.relu(h)

    def run(l):
        t = l.type_name
        if t == "initial":
            return
        h = val[id(l.input)]
        if t == "conv":
            ps = params[id(l)]
            R, S = l.filter_shape[2:]
            pad = {"valid": (0, 0), "half": (R // 2, S // 2), "full": (R - 1, S - 1)}[l.border_mode]
            h = Fn.conv2d(h, ps[0].flip(2, 3), stride=tuple(l.stride), padding=pad)
            if l.use_bias:
                h = h + _per_channel(ps[1])
        elif t in NORMS:
            assert l.enabled
            gamma, beta = params[id(l)]
            if l.norm_groups:
                h = Fn.group_norm(h, l.norm_groups, gamma, beta, l.eps)
            elif train:
                mu = h.mean(dim=(0, 2, 3))
                inv = 1.0 / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=False) + l.eps)
                stats[id(l)] = {"mean": mu.detach(), "stdinv": inv.detach()}
                h = (h - _per_channel(mu)) * _per_channel(gamma * inv) + _per_channel(beta)
            else:
                rm, rs = running[id(l)]
                i2 = 1.0 / torch.sqrt((1.0 / rs) ** 2 + l.eps)
                h = (h - _per_channel(rm)) * _per_channel(gamma * i2) + _per_channel(beta)
            if t == "batchnorm-relu":
                h = relu(l, h)
        elif t == "activation":
            h = relu(l, h) if l.activation in ("relu", "relu-safe") else act64(l.activation, h)
        elif t == "pool":
            assert l.ignore_border
            pool = {"max": Fn.max_pool2d, "average_inc_pad": Fn.avg_pool2d}[l.mode]
            h = pool(h, l.size[0], l.stride[0], l.pad[0])
        elif t == "resnet":
            for s in l.layers:
                run(s)
            y = val[id(l.layers[l.n_main - 1].output)]
            sc = l.layers[l.n_main:]
            xs = val[id(sc[-1].output)] if sc else h
            if "pre-activation" in l.version:
                h = xs + y
            elif l.activation in ("relu", "relu-safe"):
                h = relu(l, xs + y)
            else:
                h = act64(l.activation, xs + y)
        elif t == "regression":
            assert tuple(h.shape[2:]) == (1, 1), tuple(h.shape)
            logits = h[:, :, 0, 0]
            lp = torch.log_softmax(logits, dim=1)
            val["cost"] = -lp[torch.arange(len(cls)), torch.from_numpy(np.asarray(cls))].mean()
            val["logits"] = logits
            return
        else:
            raise AssertionError("unexpected layer " + t)
        assert tuple(h.shape) == tuple(l.output_shape), (l.layer_index, t, tuple(h.shape), l.output_shape)
        val[id(l.output)] = h

    for l in model.layers:
        run(l)
    return val["cost"], val["logits"], stats
