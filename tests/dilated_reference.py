"""A dilated model restated in float64 on the host. A helper module: it holds no test.

`fp64_model.reference` does not know dilation. This is the restatement the dilated whole-step test uses: PyTorch's CPU `conv2d(...,
dilation=)` in float64 on the flipped filter ("Dilated convolutions": y[n, oy, ox, k] = sum x[n, oy*sh - ph + r*dh,
ox*sw - pw + s*dw, c] * w[k, r, s, c] on the stored correlation taps), the gradients by autograd. It covers the layer kinds the
small dilated models use - conv, batchnorm, activation, resnet, regression - and is keyed and wired like fp64_model.reference; the
shared helpers come from there."""
import torch
import torch.nn.functional as Fn

from fp64_model import act64, build_model, param_layers, rel, relu_masks_of, sgd_step_errors  # noqa: F401 (re-exported)


def conv_padding(border, ke_h, ke_w):
    """the border modes on the effective extent ke = (k - 1) * d + 1"""
    if isinstance(border, (tuple, list)):
        return (int(border[0]), int(border[1]))
    if isinstance(border, int):
        return (border, border)
    return {"valid": (0, 0), "half": (ke_h // 2, ke_w // 2), "full": (ke_h - 1, ke_w - 1), "same": (ke_h // 2, ke_w // 2)}[border]


def conv64(h, w_ref, stride, border, dilation):
    """float64 conv2d of the reference-layout filter w_ref [K, C, R, S] (a true convolution: the filter is flipped), dilated"""
    R, S = w_ref.shape[2:]
    ke = ((R - 1) * dilation[0] + 1, (S - 1) * dilation[1] + 1)
    y = Fn.conv2d(h, w_ref.flip(2, 3), stride=tuple(stride), padding=conv_padding(border, *ke), dilation=tuple(dilation))
    if border == "same":
        y = y[:, :, :h.shape[2], :h.shape[3]]
    return y


def _per_channel(v):
    return v[None, :, None, None]


def reference(model, x, params, cls, train, running=None, relu_masks=None, flips=None, outs=None):
    """the layer list in float64, every dict keyed by id(layer) as in fp64_model.reference. Returns (cost, logits, stats) with
    stats[id(bn)] = {"mean", "stdinv"} of the batch. A layer kind that is not restated here raises"""
    val = {id(model.layers[0].output): torch.from_numpy(x).double()}
    stats = {}

    def run(l):
        t = l.type_name
        if t == "initial":
            return
        h = val[id(l.input)]
        if t == "conv":
            ps = params[id(l)]
            h = conv64(h, ps[0], l.stride, l.border_mode, getattr(l, "dilation", (1, 1)))
            if l.use_bias:
                h = h + _per_channel(ps[1])
            if outs is not None:
                h.retain_grad()
                outs[id(l)] = h
        elif t == "batchnorm":
            assert l.enabled
            gamma, beta = params[id(l)]
            if train:
                mu = h.mean(dim=(0, 2, 3))
                inv = 1.0 / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=False) + l.eps)
                stats[id(l)] = {"mean": mu.detach(), "stdinv": inv.detach()}
                h = (h - _per_channel(mu)) * _per_channel(gamma * inv) + _per_channel(beta)
            else:
                rm, rs = running[id(l)]
                i2 = 1.0 / torch.sqrt((1.0 / rs) ** 2 + l.eps)                          # (eps twice, as the layer does)
                h = (h - _per_channel(rm)) * _per_channel(gamma * i2) + _per_channel(beta)
        elif t == "activation":
            if relu_masks is not None and l.activation in ("relu", "relu-safe"):
                m = relu_masks[id(l)].double()
                if flips is not None:
                    flips[id(l)] = int(((h.detach() > 0).double() != m).sum())
                h = h * m
            else:
                h = act64(l.activation, h)
        elif t == "resnet":
            for s in l.layers:
                run(s)
            y = val[id(l.layers[l.n_main - 1].output)]
            sc = l.layers[l.n_main:]
            xs = val[id(sc[-1].output)] if sc else h
            if "pre-activation" in l.version:
                h = xs + y
            elif relu_masks is not None and id(l) in relu_masks and l.activation in ("relu", "relu-safe"):
                m = relu_masks[id(l)].double()                                          # the block's exit ReLU, as the device decided
                if flips is not None:
                    flips[id(l)] = int((((xs + y).detach() > 0).double() != m).sum())
                h = (xs + y) * m
            else:
                h = act64(l.activation, xs + y)
        elif t == "regression":
            assert tuple(h.shape[2:]) == (1, 1), tuple(h.shape)
            logits = h[:, :, 0, 0]
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


def block_exit_masks(model):
    """{id(resnet layer): the exit ReLU's decisions of the last forward pass, [N, C, H, W] bool on the host} of the `original`
    blocks whose output the forward pass left (relu_masks_of covers the activation layers, the exit of a block is none)"""
    out = {}
    for l in model.layers:
        if l.type_name == "resnet" and "pre-activation" not in l.version and l.activation in ("relu", "relu-safe"):
            d = l.output._data
            if d is not None:
                out[id(l)] = (d[..., :l.output_shape[1]] > 0).permute(0, 3, 1, 2).cpu()
    return out
