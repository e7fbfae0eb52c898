"""`BN` layer — spatial batch normalisation. Mirrors denet/layer/batch_norm.py (BatchNormLayer :12-129):
cuDNN batch statistics (biased variance, eps inside the sqrt), running `mean` and running INVERSE standard
deviation `stdinv` with momentum (:75-76), gamma/beta reported as biases (no L2 decay, :106-107), and the
test-time path that feeds var = 1/stdinv^2 to cuDNN which adds eps a second time (:50-52).
The batch renormalisation the reference keeps commented out (:65-73) runs here for the layers whose parameters ask for it
(renormMaxR > 1 or renormMaxD > 0): ops.bn_renorm_fwd_train / bn_renorm_bwd, DESIGN.md section 14.
GROUP NORMALISATION (Wu & He 2018) is a mode of the same layers, this build's own (`BN.G[g, eps]`, `BNA.G[g, eps]`, the JSON key
normGroups): per-sample statistics over g groups of consecutive channels, identical in training and
inference (ops.gn_fwd / gn_bwd, csrc/gn.hip). `mean` / `stdinv` / `momentum` stay in the layer and in the file, unread."""
import math

import numpy

from . import AbstractLayer, Act, Param, get_epoch, get_train
from .. import ops


def renorm_active(max_r, max_d):
    """batch renormalisation is asked for (the condition of the reference's commented-out block, batch_norm.py:66)"""
    return max_r > 1.0 or max_d > 0.0


def renorm_check(max_r, max_d, max_it):
    """refuses limits no step could run with, when the layer is built"""
    for name, v in (("renormMaxR", max_r), ("renormMaxD", max_d), ("renormMaxIt", max_it)):
        if isinstance(v, bool) or not isinstance(v, (int, float, numpy.integer, numpy.floating)) or not math.isfinite(v):
            raise ValueError("batch norm: %s must be a finite number, got %r" % (name, v))
    if max_r < 1.0:
        raise ValueError("batch norm: renormMaxR must be >= 1 (1 = no correction of the scale), got %r" % (max_r,))
    if max_d < 0.0:
        raise ValueError("batch norm: renormMaxD must be >= 0 (0 = no correction of the mean), got %r" % (max_d,))
    if max_it < 0:
        raise ValueError("batch norm: renormMaxIt must be >= 0 (epochs over which the limits open; 0 = open from the start), "
                         "got %r" % (max_it,))


def renorm_limits(max_r, max_d, max_it, epoch):
    """(r_max, d_max) of a training step in `epoch` (batch_norm.py:67-70): the limits open from (1, 0) at epoch 0 to (max_r, max_d)
    at epoch max_it. The reference divides by max_it; the `BN[...]` grammar defaults it to 0, which means no ramp here"""
    if max_it <= 0:
        return float(max_r), float(max_d)
    r_max = min(float(max_r), math.exp(epoch * math.log(max_r) / max_it))
    d_max = min(float(max_d), math.exp(epoch * math.log(max_d + 1.0) / max_it) - 1.0)
    return max(r_max, 1.0), max(d_max, 0.0)


def renorm_layers(model):
    """the renorm-active batch norms of a model, nested ones included"""
    from ..model.model_cnn import walk_layers
    return [l for l in walk_layers(model.layers) if isinstance(l, BatchNormLayer) and l.enabled and l.renorm_active]


def renorm_log_line(model, epoch):
    """what model-train reports at the start of an epoch, or None for a model without renorm-active layers"""
    ls = renorm_layers(model)
    if not ls:
        return None
    lims = sorted({renorm_limits(l.renorm_max_r, l.renorm_max_d, l.renorm_max_it, epoch) for l in ls})
    return "batch renorm: %d active layers, epoch %d limits %s" % (
        len(ls), epoch, " ".join("r_max=%.6g d_max=%.6g" % lim for lim in lims))


def norm_groups_check(groups, channels=None, what="batch norm"):
    """refuses a normGroups value no layer could run with, when the layer is built; 0 = batch statistics (the mode is off)"""
    if isinstance(groups, (float, numpy.floating)) and float(groups).is_integer():
        groups = int(groups)          # (the desc grammar and JSON hand numbers over as they were written: `8.0` is 8)
    if isinstance(groups, bool) or not isinstance(groups, (int, numpy.integer)) or groups < 0:
        raise ValueError("%s: normGroups must be an integer >= 1 (0 in a model file: batch statistics), got %r" % (what, groups))
    groups = int(groups)
    if groups and channels is not None and channels % groups:
        raise ValueError("%s: normGroups %d does not divide the layer's %d channels" % (what, groups, channels))
    return groups


def desc_norm_groups(params):
    """g of a `BN.G[g, eps]` / `BNA.G[g, eps]` token (default 32). The token asks for the mode, so 0 - which in a model file
    means batch statistics - is refused here like every other value that is no integer >= 1"""
    g = params.get(0, 32)
    if not isinstance(g, bool) and g == 0:
        raise ValueError("batch norm: normGroups must be an integer >= 1 in a `.G[g, eps]` token, got %r" % (g,))
    return g


def group_norm_layers(model):
    """the batch-norm layers of a model that run as group norms, nested ones included"""
    from ..model.model_cnn import walk_layers
    return [l for l in walk_layers(model.layers) if isinstance(l, BatchNormLayer) and l.enabled and l.norm_groups]


def group_norm_log_line(model):
    """what model-train reports once at start, or None for a model without group-mode layers"""
    ls = group_norm_layers(model)
    if not ls:
        return None
    return "group norm: %d layers, groups %s" % (len(ls), " ".join(str(g) for g in sorted({l.norm_groups for l in ls})))


class BatchNormLayer(AbstractLayer):
    type_name = "batchnorm"
    fused_relu = False

    def __init__(self, layers, momentum=0.9, eps=1e-5, renorm_max_r=1.0, renorm_max_d=0.0, renorm_max_it=10,
                 json_param={}, norm_groups=0):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        self.enabled = json_param.get("enabled", True)
        self.momentum = json_param.get("momentum", momentum)
        self.renorm_max_r = json_param.get("renormMaxR", renorm_max_r)
        self.renorm_max_d = json_param.get("renormMaxD", renorm_max_d)
        self.renorm_max_it = json_param.get("renormMaxIt", renorm_max_it)
        self.eps = json_param.get("eps", eps)
        renorm_check(self.renorm_max_r, self.renorm_max_d, self.renorm_max_it)
        # renorm-active layers take a route of their own in training (csrc/bn_renorm.hip) and give up every fusion
        self.renorm_active = renorm_active(self.renorm_max_r, self.renorm_max_d)
        self.output_shape = self.input_shape
        # group normalisation: normGroups > 0 groups of consecutive channels, statistics per sample. Like a
        # renorm-active layer it takes a route of its own (csrc/gn.hip) and gives up every batch-norm fusion
        what = "batch norm layer %d" % self.layer_index
        self.norm_groups = norm_groups_check(json_param.get("normGroups", norm_groups), what=what)
        if self.norm_groups:
            if self.renorm_active:
                raise ValueError("%s: normGroups %d together with an active batch renormalisation (renormMaxR %r, renormMaxD %r) - "
                                 "a group norm has no batch statistics to correct" % (what, self.norm_groups, self.renorm_max_r,
                                                                                     self.renorm_max_d))
            if not self.enabled:
                raise ValueError("%s: normGroups %d on a layer with enabled false" % (what, self.norm_groups))
            norm_groups_check(self.norm_groups, self.input_shape[1], what)
        if self.enabled:
            assert self.input.cp == self.input_shape[1], "batch norm needs an unpadded channel count (multiple of 32)"
            c = self.input_shape[1]
            self.omega = Param(numpy.ones((c,)), "bn omega")
            self.beta = Param(numpy.zeros((c,)), "bn beta")
            self.mean = Param(numpy.zeros((c,)), "bn mean")
            self.stdinv = Param(numpy.ones((c,)), "bn std inv")
            self.output = Act(self.output_shape, self.input.cp, "bn%i" % self.layer_index)
            if not self.norm_groups:
                self.input.want_stats = True      # a convolution writing this tensor also emits its per-channel sums
                self.input.stats_bn = self        # ... and may finish this layer's statistics in its own launch (ops.BnFinal)
        else:
            self.output = self.input
        self._save = None

    @staticmethod
    def parse_desc(layers, name, tags, params):
        if name != "BN":
            return False
        if "G" in tags:
            # `BN.G[g, eps]`: the tag changes what the positional parameters mean (as on `C.G`); momentum keeps its default, unread
            layers.append(BatchNormLayer(layers, eps=params.get(1, 1e-5), norm_groups=desc_norm_groups(params)))
            return True
        layers.append(BatchNormLayer(layers, params.get(0, 0.9), params.get(1, 1e-5), params.get(2, 1),
                                     params.get(3, 0), params.get(4, 0)))
        return True

    def params(self):
        return [self.omega, self.beta, self.mean, self.stdinv] if self.enabled else []

    def updates(self, cost=None):
        return [self.mean, self.stdinv] if self.enabled else []

    def biases(self):
        return [self.omega, self.beta] if self.enabled else []

    def all_params(self):
        return [self.omega, self.beta] if self.enabled else []

    def export_json(self):
        json = super().export_json()
        json.update({"momentum": self.momentum,
                     "eps": self.eps,
                     "mean": self.mean.get_value() if self.enabled else None,
                     "std": self.stdinv.get_value() if self.enabled else None,
                     "gamma": self.omega.get_value() if self.enabled else None,
                     "bias": self.beta.get_value() if self.enabled else None,
                     "renormMaxR": self.renorm_max_r,
                     "renormMaxD": self.renorm_max_d,
                     "renormMaxIt": self.renorm_max_it,
                     "enabled": self.enabled})
        if self.norm_groups:
            json["normGroups"] = self.norm_groups      # (written by group-mode layers only: default files keep their keys)
        return json

    def import_json(self, json_param):
        if self.enabled:
            self.omega.set_value(numpy.asarray(json_param["gamma"], dtype=numpy.float32))
            self.beta.set_value(numpy.asarray(json_param["bias"], dtype=numpy.float32))
            self.mean.set_value(numpy.asarray(json_param["mean"], dtype=numpy.float32))
            self.stdinv.set_value(numpy.asarray(json_param["std"], dtype=numpy.float32))

    # ---- execution ----
    def stats_final(self, act):
        """for the convolution pass that writes `act` (this layer's input) in a training step: the description of this layer's
        statistics, so that the pass can finish them in its own launch (ops.BnFinal; the running statistics are updated there)"""
        if not (self.enabled and ops.FINAL_FOLD and act is self.input) or self.renorm_active or self.norm_groups:
            return None
        if getattr(self, "pool_behind", None) is not None and ops.BN_POOL_FUSE:
            # the fused BN + ReLU + max-pool pass reduces the partial rows itself and updates the running statistics there
            # (ops.bn_relu_pool_fwd_train reads only the rows): a producer that also finished them would advance run_mean /
            # run_stdinv twice per step. The producer keeps writing rows only.
            return None
        n, c = act.shape[0], act.cp
        m = 1
        for d in act.shape[2:]:
            m *= d
        return ops.BnFinal(1, n * m, c, self.__dict__.setdefault("_bnf_holder_fwd", {}), momentum=self.momentum, eps=self.eps,
                           run_mean=self.mean.dev, run_stdinv=self.stdinv.dev)

    def forward(self, ctx, res=None, relu=None, out_act=None):
        """res / relu / out_act let ResnetLayer fuse the residual add + ReLU into the normalisation pass"""
        if not self.enabled:
            return
        if relu is None and out_act is None and getattr(self, "act_fused", False):
            relu, out_act = True, self.act_behind.output          # `BN A`: see ActivationLayer
        relu = self.fused_relu if relu is None else relu
        out_act = self.output if out_act is None else out_act
        x = self.input.data
        if self.norm_groups:
            # group normalisation: one route for training and inference, no batch statistics, no BnLink, no pool fusion (the pool
            # runs behind it); the running statistics are neither read nor written
            train = bool(get_train())
            y, sm, si = ops.gn_fwd(x, self.omega.dev, self.beta.dev, self.norm_groups, self.eps, relu=relu, res=res, save=train)
            if train:
                self._save = (sm, si, relu, out_act, res is not None)
                self._pooled = False
            out_act.data = y
            return
        if get_train():
            # per-channel sums already written by the convolution that produced x (ConvLayer.forward), valid for this tensor only
            pre = getattr(self.input, "stats", None)
            self.input.stats = None
            if self.renorm_active:
                # batch renormalisation (batch_norm.py:65-73): the producer's sums or the layer's own, finished together with r, d
                # and the running statistics in one launch; the pointwise pass runs at once (no BnLink, no pool fusion)
                r_max, d_max = renorm_limits(self.renorm_max_r, self.renorm_max_d, self.renorm_max_it, get_epoch())
                y, sm, si, state = ops.bn_renorm_fwd_train(x, self.omega.dev, self.beta.dev, self.mean.dev, self.stdinv.dev, r_max,
                                                           d_max, self.momentum, self.eps, relu=relu, res=res, pre=pre)
                self._save = (sm, si, relu, out_act, res is not None)
                self._renorm_state = state
                self._pooled = False
                out_act.data = y
                return
            pool = getattr(self, "pool_behind", None)
            own_out = self.act_behind.output if getattr(self, "act_fused", False) else self.output
            if pool is not None and ctx is not None and relu and res is None and out_act is own_out and ops.BN_POOL_FUSE:
                # a max pool is the only reader of this layer's output (ModelCNN.build_train_func links it): one pass
                # writes the pooled tensor, relu(bn(x)) itself is never materialised (its gradient neither)
                k, s, p = pool.size[0], pool.stride[0], pool.pad[0]
                assert pre is None or len(pre) == 2, "statistics finished by the producer in front of a pool-fused batch norm"
                yp, arg, sm, si, xh = ops.bn_relu_pool_fwd_train(x, self.omega.dev, self.beta.dev, self.mean.dev, self.stdinv.dev,
                                                                 k, s, p, self.momentum, self.eps, pre=pre, xhat=True)
                pool.output.data, pool._arg, pool._fused_in = yp, arg, ctx      # valid for this pass (ctx) only
                # the backward reductions of this layer are sums over the pooled tensors (ops.bn_relu_pool_bwd_pooled); the
                # data-gradient pass that writes the pool output's gradient can leave them behind (sums_request)
                pool._xhat = xh
                pool.output.bn_producer = self
                out_act.data = None
                self._save = (sm, si, relu, out_act, False)
                self._pooled = True
                return
            self._pooled = False
            if pre is not None and ops.LINK_BN and ctx is not None:
                # the statistics are reduced now; the pointwise pass is left to the reader of the output (a Winograd convolution
                # runs it inside its input transform, anybody else triggers it by taking out_act.data - ops.BnLink)
                link, sm, si = ops.bn_fwd_train_link(x, self.omega.dev, self.beta.dev, self.mean.dev, self.stdinv.dev, pre,
                                                     self.momentum, self.eps, relu=relu, res=res)
                self._save = (sm, si, relu, out_act, res is not None)
                out_act.set_pending_data(link)
                out_act.bn_producer = self
                return
            y, sm, si = ops.bn_fwd_train(x, self.omega.dev, self.beta.dev, self.mean.dev, self.stdinv.dev,
                                         self.momentum, self.eps, relu=relu, res=res, pre=pre)
            self._save = (sm, si, relu, out_act, res is not None)
            out_act.data = y
            out_act.bn_producer = self
            return
        else:
            probe = getattr(ctx, "bn_probe", None)
            if probe is not None and probe[0] is self:
                # model/update_bn.py: the moments of the raw input of this layer, taken before it normalises
                ops.bn_moments_accumulate(x, probe[1], probe[2])
            y = ops.bn_fwd_test(x, self.omega.dev, self.beta.dev, self.mean.dev, self.stdinv.dev, self.eps, relu=relu,
                                res=res, cache=self.__dict__.setdefault("_infer_cache", {}))
        out_act.data = y

    def sums_request(self, act):
        """for the data-gradient pass that writes the gradient of `act` (this layer's output of the current training step): the
        description of this batch norm, so that the pass leaves the two backward reductions behind (ops.BnSums)"""
        if not (self.enabled and self._save is not None) or self.renorm_active or self.norm_groups:
            return None
        if getattr(self, "_pooled", False):
            # the fused BN + ReLU + max pool: `act` is the POOL's output; over the pooled tensors the layer looks like a batch norm
            # with input xhat (already normalised: mean 0, invstd 1) and forward output y_pool
            pool = self.pool_behind
            if act is not pool.output or getattr(pool, "_xhat", None) is None:
                return None
            C = act.data.shape[-1]
            return ops.BnSums(pool._xhat, act.data, self.omega.dev, self.beta.dev, ops.const_vec(0.0, C), ops.const_vec(1.0, C), True)
        sm, si, relu, out_act, has_res = self._save
        if out_act is not act:
            return None
        # the data-gradient pass may also FINISH the two reductions (dgamma, dbeta, their means) in its own launch (ops.BnFinal)
        x = self.input.data
        fin = None
        if ops.FINAL_FOLD and self.omega.grad is not None and self.beta.grad is not None:
            fin = ops.BnFinal(2, x.numel() // x.shape[-1], x.shape[-1], self.__dict__.setdefault("_bnf_holder", {}),
                              dgamma=self.omega.grad, dbeta=self.beta.grad)
        return ops.BnSums(x, out_act.data if (relu and has_res) else None, self.omega.dev, self.beta.dev, sm, si, relu, final=fin)

    def backward(self, ctx, want_dres=False):
        if not self.enabled:
            return None
        sm, si, relu, out_act, has_res = self._save
        if self.norm_groups:
            y = out_act.data if (relu and has_res) else None      # (no residual: the mask is recomputed from x)
            dx, dres, _, _ = ops.gn_bwd(self.input.data, y, out_act.grad, self.omega.dev, sm, si, self.norm_groups, relu=relu,
                                        want_dres=want_dres, dgamma=self.omega.grad, dbeta=self.beta.grad, beta=self.beta.dev)
            self.input.add_grad(dx)
            return dres
        if self.renorm_active:
            y = out_act.data if (relu and has_res) else None      # (no residual: the mask is recomputed from x, as in the forward)
            dx, dres, _, _ = ops.bn_renorm_bwd(self.input.data, y, out_act.grad, sm, si, self._renorm_state, relu=relu,
                                               want_dres=want_dres, dgamma=self.omega.grad, dbeta=self.beta.grad)
            self.input.add_grad(dx)
            return dres
        if getattr(self, "_pooled", False):
            pool = self.pool_behind
            k, s, p = pool.size[0], pool.stride[0], pool.pad[0]
            dyp = pool.output.grad
            sums = pool.output.grad_sums       # left by the data-gradient pass that wrote dyp last (ConvLayer.backward)
            dx = ops.bn_relu_pool_bwd_pooled(self.input.data, pool._xhat, pool.output.data, dyp, pool._arg, self.omega.dev,
                                             self.beta.dev, sm, si, k, s, p, self.omega.grad, self.beta.grad,
                                             pre=sums.partial if sums is not None else None)
            pool._xhat = None
            self.input.add_grad(dx)
            return None
        # without a residual input the relu mask is recomputed from x in the kernel (no read of y)
        y = out_act.data if (relu and has_res) else None
        dy = out_act.grad
        sums = out_act.grad_sums           # left by the data-gradient pass that wrote dy last (ConvLayer.backward)
        pre = sums.partial if sums is not None else None
        if pre is not None and not (ops.LINK_BN and self.input._grad is None and self.input._pending_grad is None):
            link, dres = ops.bn_bwd_link(self.input.data, y, dy, self.omega.dev, sm, si, relu=relu, want_dres=want_dres,
                                         dgamma=self.omega.grad, dbeta=self.beta.grad, beta=self.beta.dev, pre=pre)
            self.input.add_grad(link.materialise())
            return dres
        if ops.LINK_BN and self.input._grad is None and self.input._pending_grad is None:
            # the two sums now; the gradient of the input is formed by whoever reads it - the convolution in front inside the
            # transform of its data- and filter-gradient passes (ConvLayer.backward), anybody else through Act.grad
            link, dres = ops.bn_bwd_link(self.input.data, y, dy, self.omega.dev, sm, si, relu=relu,
                                         want_dres=want_dres, dgamma=self.omega.grad, dbeta=self.beta.grad, beta=self.beta.dev,
                                         pre=pre)
            self.input.set_pending_grad(link)
            return dres
        dx, dres, _, _ = ops.bn_bwd(self.input.data, y, dy, self.omega.dev, sm, si, relu=relu,
                                    want_dres=want_dres, dgamma=self.omega.grad, dbeta=self.beta.grad,
                                    beta=self.beta.dev)
        self.input.add_grad(dx)
        return dres


def test():
    """The reference's known-answer test (denet/layer/batch_norm.py:131-154), runnable on a GPU box."""
    from . import InitialLayer, set_train
    import torch
    numpy.random.seed(1002)
    eps = 1e-4
    input_shape = (64, 128, 32, 32)
    bn = BatchNormLayer([InitialLayer(Act(input_shape), input_shape)])
    for p in bn.params():
        p.dev = torch.from_numpy(p.to_dev_layout()).cuda()
    x = numpy.random.uniform(0.0, 1.0, input_shape).astype(numpy.float32)
    bn.input.data = ops.nchw_to_nhwc(torch.from_numpy(x).cuda(), 128)
    set_train(True)
    bn.forward(None)
    y = bn.output.data
    x_mean = bn.mean.get_value()
    x_std = bn.stdinv.get_value()
    if abs(float(y.mean())) > eps or abs(float(y.std()) - 1.0) > eps or abs(x_mean.mean() - x.mean() * 0.1) > eps \
            or abs(x_std.mean() - 1.24641) > eps:
        raise Exception("Batchnorm failed test! ", float(y.mean()), float(y.std()), x_mean.mean(), x_std.mean())
