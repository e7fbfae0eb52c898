"""`R` — final convolution + soft-max classification cost. Mirrors denet/layer/regression.py (RegressionLayer
:10-98, parse_desc :53-63 appends the conv then this layer). Cost: -mean(log_softmax(x)[b, image_class]) (:97-98).

Two paths. A 1x1 logit map with no `valid` list (`R` behind a full-size pooling: ResNet-34, cifar3): the detection-cost kernel
and a host softmax. Any other map (`R.C`, or a `valid` list): the views - the pixels of `valid`, or every pixel without one
(:31-38) - go to csrc/regression.hip: the cost over the views, and the probabilities averaged over them (:45-47). The reference
indexes its (B, C, V) log-probabilities with b * C + cls (:79-81, its output_shape is always 2-D), which picks the right entry
only for V = 1: training takes one view, prediction any number."""
import math

import numpy

from . import AbstractLayer, Act
from .convolution import ConvLayer
from .. import ops


class RegressionLayer(AbstractLayer):
    type_name = "regression"

    def __init__(self, layers, use_center=True, valid=[], json_param={}):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        if isinstance(layers[-1], ConvLayer):
            layers[-1].fp32_only = True    # the softmax reads it: never the opt-in bf16 kernel (ops.INFER_PRECISION)
        if use_center:
            valid = [(0, self.input_shape[-2] // 2, self.input_shape[-1] // 2)]
        self.valid = [tuple(int(a) for a in v) for v in json_param.get("valid", valid)]     # (JSON gives lists)
        B, C, H, W = self.input_shape
        # views: pixel indices y * W + x of the logits the cost / probabilities read; None on the 1x1 path
        self.views = None
        self.log_pr_shape = self.input_shape
        if len(self.valid) > 0 or H != 1 or W != 1:
            pix = [(v[1], v[2]) for v in self.valid] if len(self.valid) > 0 else [(y, x) for y in range(H) for x in range(W)]
            for y, x in pix:
                if not (0 <= y < H and 0 <= x < W):
                    raise ValueError("regression view (%i, %i) outside the %ix%i logit map" % (y, x, H, W))
            if len(set(pix)) != len(pix):
                raise ValueError("duplicate regression views in valid=%s" % (self.valid,))
            self.views = [y * W + x for y, x in pix]
            self.log_pr_shape = (B, C, len(self.views))
        self.output_shape = (self.input_shape[0], self.input_shape[1])
        self.output = Act(self.output_shape, self.input.cp, "regression")
        self.class_num = self.input_shape[1]
        self._target = None
        self._views_dev = None

    @staticmethod
    def parse_desc(layers, name, tags, params):
        if name != "R":
            return False
        use_bias = bool("B" in tags)
        use_center = bool("C" in tags)
        filter_shape = (params["classNum"], layers[-1].output_shape[1], params.get(0, layers[-1].output_shape[2]),
                        params.get(0, layers[-1].output_shape[3]))
        layers.append(ConvLayer(layers, filter_shape, (1, 1), use_bias, "valid", params["wb"]))
        layers.append(RegressionLayer(layers, use_center))
        return True

    def export_json(self):
        json = super().export_json()
        json.update({"valid": self.valid})
        return json

    def get_target(self, model, samples, metas):
        yt_index = [numpy.ravel_multi_index((b, metas[b]["image_class"]), self.output_shape) for b in range(len(metas))]
        return numpy.array(yt_index, dtype=numpy.int64), numpy.array([], dtype=numpy.float32)

    def cost(self, yt_index, yt_value):
        if self.views is not None and len(self.views) > 1:
            raise NotImplementedError(
                "training a regression layer over %i views: the reference's cost indexes its (B, C, V) log-probabilities with "
                "b * C + class (regression.py:79-81,97-98), which is right only for one view; train with `R.C` or a one-entry "
                "valid list (prediction takes any number of views)" % len(self.views))
        return True

    def views_dev(self):
        """the view pixel indices as an int32 device tensor (made once)"""
        if self._views_dev is None:
            import torch
            self._views_dev = torch.tensor(self.views, dtype=torch.int32, device="cuda")
        return self._views_dev

    def probabilities(self, logits):
        """[B, C] device tensor: the softmax averaged over the views (regression.py:45-47)"""
        return ops.regression_probs(logits, self.views_dev(), self.class_num)

    def forward(self, ctx):
        # probabilities are only materialised on request (predict); training needs the logits only
        self.output.data = self.input.data

    def set_target(self, ctx, yt_index, yt_value):
        import torch
        B, C = self.output_shape
        if self.views is not None:
            # the class of every sample: get_target's index is b * C + class
            cls = numpy.asarray(yt_index, dtype=numpy.int64) - numpy.arange(B, dtype=numpy.int64) * C
            self._target = torch.from_numpy(cls.astype(numpy.int32)).cuda()
            return
        t = numpy.zeros((B, C), dtype=numpy.float32)
        t.reshape(-1)[numpy.asarray(yt_index)] = 1.0
        self._target = torch.from_numpy(t).cuda()

    def loss_backward(self, ctx, cost_out, want_grad=True):
        """cost = -mean_b log_softmax(x)[b, cls]; evaluated with the detection-cost kernel (one wave per row):
        cost_factor = ln(C) cancels its 1/ln(C) normalisation, batch = B gives the mean."""
        B, C = self.output_shape
        if self.views is not None:
            # the view path: -mean log_softmax at the view pixel, gradient (softmax - onehot) / B there, zero elsewhere
            x = self.input.data
            dl = ops.empty(*x.shape) if want_grad else None
            ops.regression_loss(x, self.views_dev(), self._target, dl, cost_out, C)
            if want_grad:
                self.input.grad = dl
            return
        logits = self.input.data.view(B, self.input.cp)
        dl = ops.empty(B, self.input.cp) if want_grad else None
        ops.detect_loss(logits, self._target, None, None, None, dl, cost_out, B, C, 0, math.log(C), 0.0)
        if want_grad:
            self.input.grad = dl.view(self.input.data.shape)

    def backward(self, ctx):
        pass
