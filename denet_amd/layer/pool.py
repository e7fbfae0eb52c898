"""`P` layer — max / average_inc_pad pooling. Mirrors denet/layer/pool.py (PoolLayer :10-67).

ignore_border=True (`P`, `P.A`): the cuDNN path (pool.py:37-38; max: padded taps are -inf; average_inc_pad: divisor k*k), square
windows only, csrc/pool.hip.
ignore_border=False (`P.B`, `P.AB`): the border-keeping path (pool.py:39-40, Theano's pool_2d), csrc/pool_border.hip: no padding,
windows clipped at the bottom / right edge, the average divides by the clipped window's own tap count, the max gradient goes to
every tap equal to the maximum. Those rules are Theano's host op as read, not executed; the window may
differ per axis."""
import math

from . import AbstractLayer, Act
from .. import ops


class PoolLayer(AbstractLayer):
    type_name = "pool"

    def __init__(self, layers, size=(2, 2), stride=None, pad=(0, 0), mode="max", ignore_border=True, json_param={}):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        self.size = tuple(json_param.get("size", size))
        self.pad = tuple(json_param.get("pad", pad))
        self.ignore_border = json_param.get("ignoreBorder", ignore_border)
        self.mode = json_param.get("mode", mode)
        self.stride = json_param.get("stride", stride)
        if self.stride is None:
            self.stride = self.size
        self.stride = tuple(self.stride)
        if self.size[0] is None:
            raise Exception("P layer needs an explicit size (pool.py:51: params.get(0) has no default)")
        assert self.mode in ("max", "average_inc_pad"), self.mode
        if self.ignore_border:
            if not (self.size[0] == self.size[1] and self.stride[0] == self.stride[1] and self.pad[0] == self.pad[1]):
                raise ValueError("pool layer %i: size %s, stride %s, pad %s differ per axis, which only the border-keeping mode "
                                 "(ignoreBorder false, no padding) runs; the cuDNN mode (ignoreBorder true) takes one square window"
                                 % (self.layer_index, self.size, self.stride, self.pad))
            h = int(math.floor((self.input_shape[2] + 2 * self.pad[0] - self.size[0]) / self.stride[0])) + 1
            w = int(math.floor((self.input_shape[3] + 2 * self.pad[1] - self.size[1]) / self.stride[1])) + 1
        else:
            if tuple(self.pad) != (0, 0):
                raise ValueError("pool layer %i: pad %s with ignoreBorder false (`P.B[k,s,p]`, p > 0): the reference's pool_2d refuses "
                                 "padding unless ignore_border is true; drop the padding or the B tag"
                                 % (self.layer_index, self.pad))
            if min(self.size) < 1 or min(self.stride) < 1:
                raise ValueError("pool layer %i: size %s / stride %s must be positive" % (self.layer_index, self.size, self.stride))
            # the tensor pool_2d(..., ignore_border=False) returns, and the shape the reference's layer carries for it (pool.py:32-33)
            own = tuple(ops.pool_border_out(r, k, s) for r, k, s in zip(self.input_shape[2:], self.size, self.stride))
            ref = tuple(int(math.ceil(r / s)) for r, s in zip(self.input_shape[2:], self.stride))
            if own != ref:
                raise ValueError("pool layer %i: border-keeping pooling of a %i x %i map with size %s, stride %s yields %i x %i, but "
                                 "the reference's layer declares ceil(r / s) = %i x %i (pool.py:32-33): it carries a shape its tensor "
                                 "does not have, and this layer is built under neither"
                                 % ((self.layer_index,) + tuple(self.input_shape[2:]) + (self.size, self.stride) + own + ref))
            h, w = own
        self.output_shape = (self.input_shape[0], self.input_shape[1], h, w)
        self.output = Act(self.output_shape, self.input.cp, "pool%i" % self.layer_index)
        self._arg = None

    @staticmethod
    def parse_desc(layers, name, tags, params):
        if name != "P":
            return False
        size = (params.get(0), params.get(0))
        stride = (params.get(1, size[0]), params.get(1, size[0]))
        pad = (params.get(2, 0), params.get(2, 0))
        mode = "average_inc_pad" if "A" in tags else "max"
        ignore_border = bool(not "B" in tags)
        layers.append(PoolLayer(layers, size, stride, pad, ignore_border=ignore_border, mode=mode))
        return True

    def export_json(self):
        json = super().export_json()
        json.update({"mode": self.mode, "size": self.size, "stride": self.stride, "pad": self.pad,
                     "ignoreBorder": self.ignore_border})
        return json

    def forward(self, ctx):
        if not self.ignore_border:
            fwd = ops.maxpool_border_fwd if self.mode == "max" else ops.avgpool_border_fwd
            self.output.data = fwd(self.input.data, self.size, self.stride)
            return
        k, s, p = self.size[0], self.stride[0], self.pad[0]
        if ctx is not None and getattr(self, "_fused_in", None) is ctx:
            return                               # the BN + ReLU layer in front has already written output and argmax (this pass)
        if self.mode == "max":
            self.output.data, self._arg = ops.maxpool_fwd(self.input.data, k, s, p)
        else:
            self.output.data = ops.avgpool_fwd(self.input.data, k, s, p)

    def backward(self, ctx):
        if not self.ignore_border:
            if self.mode == "max":
                dx = ops.maxpool_border_bwd(self.input.data, self.output.data, self.output.grad, self.size, self.stride)
            else:
                dx = ops.avgpool_border_bwd(self.output.grad, tuple(self.input.data.shape), self.size, self.stride)
            self.input.add_grad(dx)
            return
        k, s, p = self.size[0], self.stride[0], self.pad[0]
        if ctx is not None and getattr(self, "_fused_in", None) is ctx:
            self._fused_in = None                # the BN + ReLU layer in front gathers this layer's gradient itself
            return
        shape = tuple(self.input.data.shape)
        if self.mode == "max":
            self.input.add_grad(ops.maxpool_bwd(self.output.grad, self._arg, shape, k, s, p))
        else:
            self.input.add_grad(ops.avgpool_bwd(self.output.grad, shape, k, s, p))
