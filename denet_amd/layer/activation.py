"""`A` layer — activation. Mirrors denet/layer/activation.py (ActivationLayer :10-56, apply :25-44).

On the device: relu / relu-safe ((x+|x|)/2 == max(x,0) for finite x) and none, as before, through the ReLU kernels and
the fused batch-norm passes; sigmoid, tanh, elu (alpha = 1) and softplus through csrc/activation.hip (ops.act_fwd /
act_bwd, the derivative written from the forward output). Those four are never fused into a batch norm, a convolution
epilogue or the inference fold: a `BN A` pair runs as the plain batch norm followed by the activation pass. Their kernels
write zeros to the padding channels (f(0) != 0), which the ReLU keeps for free.

Refused, at construction: `softmax` - the reference's tensor.nnet.softmax takes 1-D / 2-D input only and every `A` layer
input is 4-D, so the reference cannot run it either (Theano is not installed: this is read from memory of its API, not
executed) - and any other name (`leaky-relu` is in the reference's help text, its apply() raises on it)."""
from . import AbstractLayer, Act
from .. import ops

RELU_NAMES = ("relu", "relu-safe")
SMOOTH_NAMES = tuple(ops.ACT_KINDS)        # sigmoid, tanh, elu, softplus


def check_activation(name):
    """raises for a name no layer of this build runs; called where a layer is constructed, not at its first forward pass"""
    if name == "none" or name in RELU_NAMES or name in SMOOTH_NAMES:
        return name
    if name == "softmax":
        raise NotImplementedError("activation 'softmax': the reference's tensor.nnet.softmax takes 1-D / 2-D input only, an "
                                  "`A` layer's input is 4-D (the soft-max of a classifier is part of the `R` layer)")
    raise ValueError("Unknown activation type: '%s' (known: none, %s)" % (name, ", ".join(RELU_NAMES + SMOOTH_NAMES)))


class ActivationLayer(AbstractLayer):
    type_name = "activation"

    def __init__(self, layers, activation="relu", json_param={}):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        self.activation = check_activation(json_param.get("activation", activation))
        self.output_shape = self.input_shape
        self.output = self.input if self.activation == "none" else Act(self.output_shape, self.input.cp,
                                                                        "act%i" % self.layer_index)
        # `BN A` written as two layers (the un-converted ResNets, examples/resnet34-imagenet.sh): when this layer is the only
        # reader of the batch norm's output, the batch norm runs its fused BN + ReLU passes straight into this layer's output
        # (ModelCNN.build_train_func sets bn.act_fused after counting the readers) - what --convert-bn-relu does to the model
        # file, without touching the layer list or the JSON
        prev = layers[-1]
        self.fused_into = None
        if self.activation in RELU_NAMES and getattr(prev, "type_name", None) == "batchnorm" and prev.enabled \
                and prev.output is self.input:
            self.fused_into = prev
            prev.act_behind = self

    @staticmethod
    def parse_desc(layers, name, tags, params):
        if name != "A":
            return False
        layers.append(ActivationLayer(layers, params["activation"]))
        return True

    def export_json(self):
        json = super().export_json()
        json.update({"activation": self.activation})
        return json

    def _fused(self):
        return self.fused_into is not None and getattr(self.fused_into, "act_fused", False)

    def forward(self, ctx):
        if self.activation == "none" or self._fused():          # fused: the batch norm in front has written (or linked) the output
            return
        if self.activation in RELU_NAMES:
            self.output.data = ops.relu_fwd(self.input.data)
        else:
            self.output.data = ops.act_fwd(self.input.data, self.input_shape[1], self.activation)

    def backward(self, ctx):
        if self.activation == "none" or self._fused():          # fused: the batch norm's backward pass reads this output's gradient
            return
        if self.activation in RELU_NAMES:
            self.input.add_grad(ops.relu_bwd(self.output.data, self.output.grad))
        else:
            self.input.add_grad(ops.act_bwd(self.output.data, self.output.grad, self.input_shape[1], self.activation))
