"""A model restated in float64 on the host, and the small helpers the whole-step tests share. A helper module: it holds no test.

`reference` is the yardstick of the tests that compare a training step or a test-mode pass of a model with float64 (simple-cifar10,
the activations, batch renormalisation, rectangular convolutions, border-keeping pools): PyTorch's CPU operators in float64, the
gradients by autograd, the formulations those of the reference implementation (the file:line notes point into it). Parameters,
statistics and masks are keyed by id(layer), so a flat stack and the nested layers of a `resnet` block are one code path. Kernel-level
references (one pass of one kernel against a closed form) stay with their tests."""
import os

import numpy as np
import torch
import torch.nn.functional as Fn

from denet_amd import ops
from denet_amd.model import model_cnn


def rel(a, b):
    """max |a - b| / max |b| in float64; tensors (any device) or numpy arrays"""
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, np.float64)) for v in (a, b))
    return float((a - b).abs().max() / b.abs().max())


def act64(name, x):
    """the activations in the dtype of x (float64 here): denet/layer/activation.py:25-44"""
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


def _per_channel(v):
    return v[None, :, None, None]


def reference(model, x, params, cls, train, running=None, masks=None, relu_masks=None, flips=None, outs=None, draw=None):
    """the layer list in float64 on the host, wired like the layers themselves: every layer reads the tensor of its `input` handle
    and writes the one of its `output` handle. Every dict is keyed by id(layer):
      params      the reference-layout arrays of a conv / deconv (filter[, bias]) or an enabled batchnorm (gamma, beta)
      running     (mean, stdinv) of a batch norm BEFORE the step; the test-mode pass normalises with them. In training mode a batch
                  norm missing from it gets draw(mu_b, inv_b), and a layer whose renormalisation limits are open takes r and d
                  against them (constants: no gradient flows through r and d)
      masks       the dropout masks of a training step
      relu_masks  the device's ReLU decisions per activation layer, used in place of the host's own; flips receives the number of
                  elements whose sign the two disagree on
      outs        receives the output of every convolution, its gradient retained
    Returns (cost, logits, stats): stats[id(bn)] = {"mean", "stdinv"} of the batch, and with `running` also "r", "d", their
    unclipped values "rv", "dv", and the updated "run_mean", "run_stdinv". The shape of every layer's output is asserted against
    the layer's own output_shape; a layer kind that is not restated here raises"""
    val = {id(model.layers[0].output): torch.from_numpy(x).double()}
    stats = {}

    def run(l):
        t = l.type_name
        if t == "initial" or (t == "batchnorm" and not l.enabled):
            return
        h = val[id(l.input)]
        if t == "border":
            h = Fn.pad(h, l.border)                                                     # (left, right, top, bottom)
        elif t == "conv":
            ps = params[id(l)]
            w = ps[0].flip(2, 3)                                                        # (true convolution: convolution.py:80-83)
            R, S = l.filter_shape[2:]
            if l.border_mode == "same":                                                 # convolution.py:66-69,76-80: the full
                y0, x0 = (R - 1) // 2, (S - 1) // 2                                     # convolution, cropped to H x W
                h = Fn.conv2d(h, w, padding=(R - 1, S - 1))[:, :, y0:y0 + h.shape[2], x0:x0 + h.shape[3]]
            else:
                pad = {"valid": (0, 0), "half": (R // 2, S // 2), "full": (R - 1, S - 1)}[l.border_mode]
                h = Fn.conv2d(h, w, stride=l.stride, padding=pad)
            if l.use_bias:
                h = h + _per_channel(ps[1])
            if outs is not None:
                h.retain_grad()
                outs[id(l)] = h
        elif t == "deconv":
            ps = params[id(l)]
            R, S = l.filter_shape[2:]
            wt = torch.flip(ps[0].permute(1, 0, 2, 3), [2, 3])
            h = Fn.conv_transpose2d(h, wt, ps[1] if l.use_bias else None, stride=l.stride, padding=(R // 2, S // 2),
                                    output_padding=(l.stride[0] - 1, l.stride[1] - 1))
        elif t == "batchnorm":
            gamma, beta = params[id(l)]
            if train:
                mu = h.mean(dim=(0, 2, 3))
                inv = 1.0 / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=False) + l.eps)
                st = stats[id(l)] = {"mean": mu.detach(), "stdinv": inv.detach()}
                scale, shift = gamma * inv, beta
                if running is not None:
                    if id(l) not in running:
                        running[id(l)] = draw(mu.detach(), inv.detach())
                    mean, stdinv = running[id(l)]
                    rv, dv = ((1.0 / inv) * stdinv).detach(), ((mu - mean) * stdinv).detach()
                    r, d = torch.ones_like(mu), torch.zeros_like(mu)
                    if l.renorm_max_r > 1 or l.renorm_max_d > 0:
                        assert l.renorm_max_it == 0                                     # open limits: the ramp is not restated
                        r = torch.clamp(rv, 1.0 / l.renorm_max_r, l.renorm_max_r)
                        d = torch.clamp(dv, -l.renorm_max_d, l.renorm_max_d)
                    st.update(r=r, d=d, rv=rv, dv=dv, run_mean=l.momentum * mean + (1 - l.momentum) * mu.detach(),
                              run_stdinv=l.momentum * stdinv + (1 - l.momentum) * inv.detach())
                    scale, shift = scale * r, beta + gamma * d
                h = (h - _per_channel(mu)) * _per_channel(scale) + _per_channel(shift)
            else:
                rm, rs = running[id(l)]
                i2 = 1.0 / torch.sqrt((1.0 / rs) ** 2 + l.eps)                          # batch_norm.py:50-52: eps twice
                h = (h - _per_channel(rm)) * _per_channel(gamma * i2) + _per_channel(beta)
        elif t == "activation":
            if relu_masks is not None and l.activation in ("relu", "relu-safe"):
                m = relu_masks[id(l)].double()
                if flips is not None:
                    flips[id(l)] = int(((h.detach() > 0).double() != m).sum())
                h = h * m
            else:
                h = act64(l.activation, h)
        elif t == "pool":
            pool = {"max": Fn.max_pool2d, "average_inc_pad": Fn.avg_pool2d}[l.mode]
            if l.ignore_border:
                h = pool(h, l.size[0], l.stride[0], l.pad[0])
            else:                                                                       # the border-keeping forms: clipped windows
                h = pool(h, l.size, l.stride, padding=0, ceil_mode=True)
        elif t == "dropout":
            if train:
                h = h * masks[id(l)]
        elif t == "resnet":
            for s in l.layers:
                run(s)
            y = val[id(l.layers[l.n_main - 1].output)]
            sc = l.layers[l.n_main:]
            xs = val[id(sc[-1].output)] if sc else h
            h = xs + y if "pre-activation" in l.version else act64(l.activation, xs + y)      # resnet.py:109-113
        elif t == "regression":
            assert len(l.valid) == 1 or (not l.valid and tuple(h.shape[2:]) == (1, 1)), (l.valid, tuple(h.shape))
            yc, xc = l.valid[0][1:] if l.valid else (0, 0)                              # (a plain `R` reads its 1 x 1 map)
            logits = h[:, :, yc, xc]
            lp = torch.log_softmax(logits, dim=1)
            val["cost"] = -lp[torch.arange(len(cls)), torch.from_numpy(cls)].mean()
            val["logits"] = logits
            return
        else:
            raise AssertionError("unexpected layer " + t)
        assert tuple(h.shape) == tuple(l.output_shape), (l.layer_index, t, tuple(h.shape), l.output_shape)
        val[id(l.output)] = h

    for l in model.layers:
        run(l)
    return val["cost"], val["logits"], stats


def build_model(desc, data_shape, B, class_num, activation="relu", border="half", seed=5, spread_bn=False, head_scale=None):
    """a ModelCNN built from desc tokens under numpy seed `seed`. spread_bn: the batch norms drawn away from (gamma, beta) = (1, 0),
    so that both gradients carry weight. head_scale: the filters of the convolution in front of the regression layer scaled by it
    (with the initialisation as it is the logits of these small nets reach the hundreds, the soft-max saturates - the test-mode
    probabilities come out as exact zeros and ones - and a comparison of probabilities says nothing; 0.05 gives logits of order one)"""
    np.random.seed(seed)
    m = model_cnn.ModelCNN()
    m.batch_size = B
    m.class_num = class_num
    m.build(desc, tuple(data_shape), activation, border, ["he-backward"])
    if spread_bn:
        rng = np.random.RandomState(seed + 1)
        for l in model_cnn.walk_layers(m.layers):
            if l.type_name == "batchnorm" and l.enabled:
                l.omega.set_value(rng.uniform(0.7, 1.3, l.omega.value.shape))
                l.beta.set_value(rng.normal(0.0, 0.3, l.beta.value.shape))
    if head_scale is not None and m.layers[-1].type_name == "regression":
        head = m.layers[-2]
        head.omega.set_value(head.omega.get_value() * head_scale)
    return m


def param_layers(model):
    """[(layer, [its trained parameters])] of the convolutions and the enabled batch norms, nested ones included"""
    out = []
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name in ("conv", "deconv"):
            out.append((l, [l.omega] + ([l.beta] if l.use_bias else [])))
        elif l.type_name == "batchnorm" and l.enabled:
            out.append((l, [l.omega, l.beta]))
    return out


def relu_masks_of(model):
    """{id(activation layer): the ReLU decisions of the last forward pass, [N, C, H, W] bool on the host}, from the activation the
    forward pass left (the solver changed gamma / beta since: no recompute)"""
    out = {}
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name == "activation":
            d = l.output._data
            assert d is not None, l.layer_index
            out[id(l)] = (d[..., :l.output_shape[1]] > 0).permute(0, 3, 1, 2).cpu()
    return out


def dropout_masks_of(model):
    """{id(dropout layer): the mask of the last training step, [N, C, H, W] float64 on the host}, drawn again from the layer's seed"""
    out = {}
    for l in model_cnn.walk_layers(model.layers):
        if l.type_name == "dropout":
            assert l._seed is not None
            n, c, hh, ww = l.input_shape
            ones = torch.ones(n, hh, ww, l.input.cp, device="cuda")
            m = ops.dropout(ones, c, l.dropout_rate, l._seed)[..., :c]
            out[id(l)] = m.permute(0, 3, 1, 2).double().cpu()
    return out


def sgd_step_errors(before, values, params, weights, lr, decay):
    """the gradients and the updates of one SGD step at iteration 0 (no momentum yet; L2 decay on the arrays of `weights` only)
    against the reference's. before: param_layers(model); values[id(layer)]: the arrays before the step; params[id(layer)]: the
    float64 tensors the reference ran on, their .grad filled; weights: set of id(p). Yields (layer, param, e_grad, e_update, g_dev,
    g_ref) per array, errors as rel()"""
    for l, ps in before:
        for p, v, t in zip(ps, values[id(l)], params[id(l)]):
            g_dev = torch.from_numpy(p.get_grad().copy()).double()     # (copies: a 1x1 filter's view may keep negative strides)
            g_ref = t.grad
            v64 = torch.from_numpy(v).double()
            p_ref = v64 - lr * (g_ref + (decay if id(p) in weights else 0.0) * v64)
            p_dev = torch.from_numpy(p.get_value().copy()).double()
            yield l, p, rel(g_dev, g_ref), rel(p_dev - v64, p_ref - v64), g_dev, g_ref


def png_dataset(root, classes=3, per_class=4, seed=0, size=32):
    """root/class<c>/img<j>.png: noise with channel c lifted, so that the classes can be told apart"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for c in range(classes):
        d = os.path.join(root, "class%i" % c)
        os.makedirs(d)
        for j in range(per_class):
            img = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
            img[..., c] = 200 + 10 * (j % 5)
            Image.fromarray(img).save(os.path.join(d, "img%i.png" % j))
