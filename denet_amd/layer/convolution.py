"""`C` layer — 2-D convolution. Mirrors denet/layer/convolution.py (ConvLayer :10-136, parse_desc :99-112,
export/import_json :114-136). The reference lowers to Theano `conv2d` (a TRUE convolution: flipped filters,
convolution.py:80-83) and cuDNN; here forward / data-gradient / weight-gradient are the MFMA implicit-GEMM
kernels of csrc/igemm.hip, the filters being stored flipped in KRSC layout on the device (layer.Param)."""
import functools
import math

import numpy

from . import AbstractLayer, Act, Param, round_up
from .. import ops


def conv_padding(border_mode, k):
    """symmetric zero padding implied by a Theano border mode for a k-wide filter. `same` with an even k is the padding k // 2
    with the output cut to the input's size (same_crop): the reference takes the full convolution and crops it at (k - 1) // 2
    (convolution.py:66-69,76-80), i.e. pads k // 2 rows / columns in front and (k - 1) // 2 behind"""
    if border_mode == "valid":
        return 0
    if border_mode == "full":
        return k - 1
    if border_mode == "half":
        return k // 2
    if border_mode == "same":
        return k // 2
    if isinstance(border_mode, (tuple, list)):
        assert border_mode[0] == border_mode[1], "only symmetric padding is supported"
        return int(border_mode[0])
    if isinstance(border_mode, int):  # includes False == 0 (denet_corner.py:39)
        return int(border_mode)
    raise Exception("Unknown border mode: " + str(border_mode))


def conv_padding2(border_mode, r, s):
    """(rows, columns) of zero padding for an r x s filter (convolution.py:55-80 works the border modes out per axis): the named
    modes pad each axis by its own filter extent, an integer n pads (n, n), a pair is taken as given"""
    if isinstance(border_mode, (tuple, list)):
        return (int(border_mode[0]), int(border_mode[1]))
    return (conv_padding(border_mode, r), conv_padding(border_mode, s))


def same_crop(border_mode, k):
    """True when the output of conv_padding's symmetric padding loses its last row and column (`same`, even k)"""
    return border_mode == "same" and k % 2 == 0


def conv_dilation2(dilation, r, s):
    """(rows, columns) of a layer's dilation ("Dilated convolutions"): an integer d is (d, d), a pair is taken as given;
    every entry an integer >= 1 (ValueError otherwise). On an axis whose filter extent is 1 a dilation has no effect and reads 1"""
    pair = tuple(dilation) if isinstance(dilation, (tuple, list)) else (dilation, dilation)
    if len(pair) != 2:
        raise ValueError("dilation %r: an integer or a pair (rows, columns)" % (dilation,))
    for d in pair:
        if isinstance(d, bool) or not isinstance(d, (int, numpy.integer)) or d < 1:
            raise ValueError("dilation %r: every entry must be an integer >= 1" % (dilation,))
    return (int(pair[0]) if r > 1 else 1, int(pair[1]) if s > 1 else 1)


def effective_extent(k, d):
    """the span of a k-tap filter axis whose taps lie d apart"""
    return (k - 1) * d + 1


def conv_groups(groups, c_in, k_out, who):
    """the group count of a layer with c_in input and k_out output channels ("Grouped convolutions"): an integer >= 1
    that divides both (ValueError otherwise, `who` names the layer or token)"""
    if isinstance(groups, bool) or not isinstance(groups, (int, numpy.integer)) or groups < 1:
        raise ValueError("%s: groups %r must be an integer >= 1" % (who, groups))
    if c_in % groups or k_out % groups:
        raise ValueError("%s: groups %i does not divide both channel counts (%i input, %i output)" % (who, groups, c_in, k_out))
    return int(groups)


class ConvLayer(AbstractLayer):
    type_name = "conv"

    def __init__(self, layers, filter_shape=None, filter_stride=(1, 1), use_bias=False, border_mode="half",
                 wb="he-backward", json_param={}, dilation=(1, 1), groups=1):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        who = "conv layer %i" % self.layer_index

        self.border_mode = json_param.get("border", border_mode)
        if isinstance(self.border_mode, list):
            self.border_mode = tuple(self.border_mode)
        self.filter_shape = tuple(json_param.get("shape", filter_shape))
        self.stride = tuple(json_param.get("stride", filter_stride))
        self.use_bias = json_param.get("useBias", use_bias)
        self.size = (self.filter_shape[2], self.filter_shape[3])
        self.enabled = json_param.get("enabled", True)

        fs = self.filter_shape
        # a grouped layer (`C.G`, `C.GX`, the JSON key "groups"; DESIGN.md, "Grouped convolutions"): g groups, output channel k reads
        # the fs[1] = C / g input channels of group k // (K / g) only. The filter (K, C / g, R, S), its initialisation bound and the
        # numpy.random calls below are those of that shape. g == 1 is no grouped layer: everything it was
        self.groups = json_param.get("groups", groups)
        if isinstance(self.groups, bool) or not isinstance(self.groups, (int, numpy.integer)) or self.groups < 1:
            raise ValueError("%s: groups %r must be an integer >= 1" % (who, self.groups))
        self.groups = int(self.groups)
        self.grouped = self.groups != 1
        if self.grouped and (fs[1] * self.groups != self.input_shape[1] or fs[0] % self.groups):
            raise ValueError("%s: groups %i does not divide both channel counts (%i input channels against %i per group, %i output)"
                             % (who, self.groups, self.input_shape[1], fs[1], fs[0]))
        # weight initialisation bound (convolution.py:31-40)
        if type(wb) is float or type(wb) is int:
            self.w_bound = float(wb)
        elif "he-forward" in wb:
            self.w_bound = math.sqrt(2.0 / (fs[2] * fs[3] * fs[1]))
        elif "he-backward" in wb:
            self.w_bound = math.sqrt(2.0 / (fs[2] * fs[3] * fs[0]))
        elif "xavier-forward" in wb:
            self.w_bound = math.sqrt(1.0 / (fs[2] * fs[3] * fs[1]))
        elif "xavier-backward" in wb:
            self.w_bound = math.sqrt(1.0 / (fs[2] * fs[3] * fs[0]))
        else:
            raise Exception("Unknown weight initialisation: " + str(wb))

        # same numpy.random call sequence as the reference (convolution.py:42-48)
        if self.w_bound > 0:
            if type(wb) is str and "uniform" in wb:
                w = numpy.random.uniform(-self.w_bound, self.w_bound, size=fs)
            else:
                w = numpy.random.normal(0.0, self.w_bound, size=fs)
        else:
            w = numpy.zeros(shape=fs)

        assert fs[1] * self.groups == self.input_shape[1], "filter channels %i x %i groups != input channels %i" % (
            fs[1], self.groups, self.input_shape[1])
        # a layer whose filter, stride or padding differs between rows and columns (`C.X`, an `R` head behind a non-square map)
        # runs the per-axis kernels of csrc/conv_rect.hip (ops.conv_rect_*) and carries its padding as a pair; a square layer keeps
        # the scalar padding and every line of the square path (tuned decisions, Winograd, fused statistics)
        # a dilated layer (`C.D`, `C.DX`, the JSON key "dilation"; DESIGN.md, "Dilated convolutions"): the taps of an axis lie d apart,
        # the border modes and the output size work on the effective extent ke = (k - 1) * d + 1, the filter and its
        # initialisation bound stay as they are. It runs the same direct kernels with dilated taps (ops.conv_dil_*)
        self.dilation = conv_dilation2(json_param.get("dilation", dilation), fs[2], fs[3])
        self.dilated = self.dilation != (1, 1)
        ke = (effective_extent(fs[2], self.dilation[0]), effective_extent(fs[3], self.dilation[1]))
        pad2 = conv_padding2(self.border_mode, ke[0], ke[1])
        self.anisotropic = fs[2] != fs[3] or self.stride[0] != self.stride[1] or pad2[0] != pad2[1]
        self.pad = pad2 if self.direct else pad2[0]
        if self.border_mode == "same":
            assert self.stride == (1, 1)

        # device geometry: physical channels, padded taps for the small-C first layer
        self.cp = self.input.cp
        if self.dilated:
            for axis, name in ((0, "row"), (1, "column")):
                if self.dilation[axis] > 1 and self.stride[axis] != 1:
                    raise ValueError("conv layer %i: %s dilation %i with %s stride %i - a dilated axis takes stride 1 only"
                                     % (self.layer_index, name, self.dilation[axis], name, self.stride[axis]))
            if self.cp < 32:
                raise ValueError("conv layer %i: a dilated layer needs 32 physical input channels or more (this input has %i: the "
                                 "raw image)" % (self.layer_index, self.cp))
            for axis, name in ((0, "rows"), (1, "columns")):
                padded = self.input_shape[2 + axis] + 2 * pad2[axis]
                if ke[axis] > padded:
                    raise ValueError("conv layer %i: effective filter extent %i (%i taps, dilation %i) is larger than the padded "
                                     "map's %i %s" % (self.layer_index, ke[axis], fs[2 + axis], self.dilation[axis], padded, name))
        self.kp = round_up(fs[0], 32)
        self.s_pad = fs[3] if self.cp >= 32 else round_up(fs[3], 32 // self.cp)
        if self.grouped:
            if self.dilated:
                raise ValueError("%s: groups %i with dilation %s - a grouped layer is not dilated" % (who, self.groups, self.dilation))
            if self.cp < 32:
                raise ValueError("%s: a grouped layer needs 32 physical input channels or more (this input has %i: the raw image)"
                                 % (who, self.cp))
            if self.cp != self.input_shape[1] or self.kp != fs[0]:
                raise ValueError("%s: a grouped layer takes no padded channels - %i input and %i output channels must be multiples "
                                 "of 32" % (who, self.input_shape[1], fs[0]))
            for axis, name in ((0, "row"), (1, "column")):
                st = self.stride[axis]
                if st < 1 or st & (st - 1):
                    raise ValueError("%s: %s stride %i of a grouped layer must be a power of two" % (who, name, st))
            try:
                ops.conv_grp_window(self.cp, self.kp, self.groups)       # window path, slab path or refused
            except ValueError as e:
                raise ValueError("%s: %s" % (who, e)) from None
        # the device filter [K][R][S][C] correlation taps; grouped: [K][R][S][C / g] (no padded channel or tap)
        self.omega = Param(w, "conv omega", "conv", (self.kp, fs[2], self.s_pad, fs[1] if self.grouped else self.cp), s_real=fs[3])
        if self.use_bias:
            self.beta = Param(numpy.zeros((fs[0],)), "conv beta", "vector", (self.kp,))

        # output shape (convolution.py:55-74)
        oh = int(math.ceil((self.input_shape[-2] + 2 * pad2[0] - ke[0] + 1) / self.stride[0]))
        ow = int(math.ceil((self.input_shape[-1] + 2 * pad2[1] - ke[1] + 1) / self.stride[1]))
        # `same` with an even filter: the passes get the output size explicitly (ops.conv_geom's ohw), None = the derived one
        self.ohw = None
        if same_crop(self.border_mode, ke[0]) or same_crop(self.border_mode, ke[1]):
            oh, ow = self.input_shape[-2], self.input_shape[-1]
            self.ohw = (oh, ow)
        self.output_shape = (self.input_shape[0], fs[0], oh, ow)
        self.output = Act(self.output_shape, self.kp, "conv%i" % self.layer_index)

    @property
    def direct(self):
        """the layer runs the direct per-axis kernels of csrc/conv_rect.hip - ops.conv_rect_*, dilated ops.conv_dil_*, grouped
        ops.conv_grp_* - and none of the square path: no tuned decision, no Winograd, no bf16 kernel, no fused statistics or skip add"""
        return self.anisotropic or self.dilated or self.grouped

    @staticmethod
    def parse_desc(layers, name, tags, params):
        """C[k, size, stride], C.X[k, kh, kw, sh, sw]; the D tag appends the dilation: C.D[k, size, stride, d],
        C.DX[k, kh, kw, sh, sw, dh, dw]; the G tag appends the groups: C.G[k, size, stride, g], C.GX[k, kh, kw, sh, sw, g];
        B: with bias"""
        if name != "C":
            return False
        use_bias = bool("B" in tags)
        extra = {}                                 # (a token without the D or G tag makes the constructor call it always made)
        if "G" in tags and "D" in tags:
            raise ValueError("C.%s: the G tag together with the D tag - a grouped layer is not dilated" % tags)
        if bool("X" in tags):
            filter_shape = (params.get(0), layers[-1].output_shape[1], params.get(1), params.get(2))
            filter_stride = (params.get(3, 1), params.get(4, 1))
            if "D" in tags:
                extra["dilation"] = (params.get(5, 1), params.get(6, 1))
            if "G" in tags:
                extra["groups"] = params.get(5, 1)
        else:
            filter_shape = (params.get(0), layers[-1].output_shape[1], params.get(1, 1), params.get(1, 1))
            filter_stride = (params.get(2, 1), params.get(2, 1))
            if "D" in tags:
                extra["dilation"] = (params.get(3, 1), params.get(3, 1))
            if "G" in tags:
                extra["groups"] = params.get(3, 1)
        if "groups" in extra:
            # the filter spans the channels of one group: (K, C / g, R, S)
            g = conv_groups(extra["groups"], filter_shape[1], filter_shape[0], "C.%s" % tags)
            filter_shape = (filter_shape[0], filter_shape[1] // g) + filter_shape[2:]
        layers.append(ConvLayer(layers, filter_shape, filter_stride, use_bias, params["borderMode"], params["wb"], **extra))
        return True

    def weights(self):
        return super().weights() + ([self.omega] if self.enabled else [])

    def biases(self):
        return super().biases() + ([self.beta] if self.use_bias and self.enabled else [])

    def all_params(self):
        """every array of the layer, trained or frozen (device packing)"""
        return [self.omega] + ([self.beta] if self.use_bias else [])

    def import_json(self, json_param):
        super().import_json(json_param)
        if self.use_bias:
            self.beta.set_value(numpy.asarray(json_param["bias"], dtype=numpy.float32))
        self.omega.set_value(numpy.asarray(json_param["weight"], dtype=numpy.float32))

    def export_json(self):
        json = super().export_json()
        json.update({"shape": self.filter_shape,
                     "stride": self.stride,
                     "border": self.border_mode,
                     "enabled": self.enabled,
                     "useBias": self.use_bias,
                     "bias": self.beta.get_value() if self.use_bias else None,
                     "weight": self.omega.get_value()})
        if tuple(self.dilation) != (1, 1):
            json["dilation"] = self.dilation       # (written by dilated layers only: every other model saves what it saved before)
        if self.groups != 1:
            json["groups"] = self.groups           # (written by grouped layers only; "shape" is then (K, C / g, R, S))
        return json

    # ---- execution ----
    def _w(self):
        return self.omega.dev.view(self.omega.dev_shape)

    def _logical(self):
        return (self.filter_shape[1], self.filter_shape[0])

    def _cache(self):
        """per-layer state of the Winograd passes (chosen tiles, transformed filters, kept input transform)"""
        c = self.__dict__.get("_wino_cache")
        if c is None:
            c = self.__dict__["_wino_cache"] = {}
        return c

    def forward(self, ctx, add=None):
        from . import get_train
        if self.direct:
            # the direct per-axis kernel on the plain tensor: a pending input is written first (Act.data), no skip add or
            # statistics in the epilogue - the layers behind run their own passes
            fwd, _, _, kw = self._direct_calls()
            self.output.data = fwd(self.input.data, self._w(), bias=self.beta.dev if self.use_bias else None, add=add,
                                   logical=self._logical(), cache=self._cache(), **kw)
            self.output.stats = None
            return
        # the input may be the output of a batch norm whose pointwise pass is still pending (ops.BnLink): a Winograd pass runs it
        # inside its input transform; whatever path conv_fwd takes, the activation exists afterwards and is stored back
        link = self.input.take_pending_data()
        cache = self._cache()
        bf16 = self._record_mode(cache, bool(get_train()))
        if bf16 and ops.HEAD_BF16X3:
            raise ValueError(ops.BF16_CONFLICT)   # (also for a model whose build_train_func ran before the mode was switched on)
        # a batch norm directly behind this layer (it flags its input Act) gets its statistics from this pass's epilogue (never the
        # bf16 kernel's: the batch norm then measures its own, as behind an anisotropic layer)
        want_stats = bool(get_train()) and getattr(self.output, "want_stats", False) and not bf16
        cache["bn_final"] = None
        self._planar_x = None
        if isinstance(link, ops.NchwLink):
            # the network input, still in the reference's planar layout: the first layer's kernels read it as it is (forward and,
            # in backward(), the filter gradient); anybody else who asks the Act for .data gets the NHWC tensor made then
            self.input.set_pending_data(link)
            if add is None and self.use_bias and self.ohw is None and ops.conv_stem_ok(link.x, self.omega.dev_shape, self.stride[0],
                                                                                        self.pad, self.filter_shape[3]):
                self.output.data = ops.conv_stem_fwd(link.x, self._w(), self.beta.dev, cache, want_stats, logical=self._logical())
                self.output.stats = cache.pop("bn_stats", None) if want_stats else None
                self._planar_x = link.x
                return
            link = None
        up = None
        if isinstance(link, ops.UpLink):
            up, link = link, None                 # the pool-inverse layer in front has not written its output (ops.UpLink)
        x = self.input.data if (link is None and up is None) else None
        skip = getattr(self, "skip_behind", None)
        if skip is not None and add is None and get_train() and ctx is not None:
            # the SKIP layer behind adds its tap to this layer's output: here, in the epilogue (ModelCNN.build_train_func links the
            # two); the sum is the SKIP layer's output, and what a batch norm behind THAT wants to know about it is measured here
            want_skip_stats = getattr(skip.output, "want_stats", False) and not bf16
            sbn = getattr(skip.output, "stats_bn", None) if want_skip_stats else None
            cache["bn_final"] = sbn.stats_final(skip.output) if sbn is not None else None
            y = ops.conv_fwd(x, self._w(), bias=None, add=skip.y.data, stride=self.stride[0], pad=self.pad,
                             s_real=self.filter_shape[3], logical=self._logical(), cache=cache, bn_stats=want_skip_stats, link=link,
                             up=up, ohw=self.ohw)
            if link is not None:
                self.input.data = link.materialise()
            self._settle_up(up)
            self.output.data = None              # the convolution's own output is never written
            self.output.stats = None
            skip.output.data = y
            skip.output.stats = cache.pop("bn_stats", None) if want_skip_stats else None
            skip._fused_in = ctx
            return
        sbn = getattr(self.output, "stats_bn", None) if (want_stats and ctx is not None) else None
        cache["bn_final"] = sbn.stats_final(self.output) if sbn is not None else None
        self.output.data = ops.conv_fwd(x, self._w(), bias=self.beta.dev if self.use_bias else None, add=add,
                                        stride=self.stride[0], pad=self.pad, s_real=self.filter_shape[3],
                                        logical=self._logical(), cache=cache, bn_stats=want_stats, link=link, up=up, ohw=self.ohw)
        if link is not None:
            self.input.data = link.materialise()
        self._settle_up(up)
        self.output.stats = cache.pop("bn_stats", None) if want_stats else None

    def _direct_calls(self):
        """(fwd, dgrad, wgrad, their geometry arguments) of a direct layer: a dilated one takes the conv_dil_* calls, a grouped one
        conv_grp_* (its data gradient shares the forward pass's slab filter through the layer's cache), an anisotropic one that is
        neither keeps conv_rect_*"""
        kw = dict(stride=self.stride, pad=self.pad, s_real=self.filter_shape[3], ohw=self.ohw)
        if self.grouped:
            return (ops.conv_grp_fwd, functools.partial(ops.conv_grp_dgrad, cache=self._cache()), ops.conv_grp_wgrad,
                    dict(kw, groups=self.groups))
        if self.dilated:
            return ops.conv_dil_fwd, ops.conv_dil_dgrad, ops.conv_dil_wgrad, dict(kw, dilation=self.dilation)
        return ops.conv_rect_fwd, ops.conv_rect_dgrad, ops.conv_rect_wgrad, kw

    def _record_mode(self, cache, training):
        """what ops.conv_fwd / conv_dgrad / conv_wgrad read about this pass in the layer's cache -> cache["bf16_train"]"""
        cache["train"] = training and self.enabled and self.omega.grad is not None
        # an inference pass (never a pass of a training step, frozen layers included) may take the opt-in bf16 kernel
        # (ops.INFER_PRECISION) unless the layer is kept in fp32 (fp32_only: a softmax reads this layer's output)
        cache["infer"] = not training
        cache["fp32_only"] = getattr(self, "fp32_only", False)
        # a training-mode pass of an eligible layer takes the opt-in bf16 kernels (ops.TRAIN_PRECISION); the mode is recorded here,
        # and the backward pass of this step follows the record whatever the global says by then. (What a training step recorded
        # is that step's: inference never reads TRAIN_PRECISION)
        cache["bf16_train"] = training and ops.train_bf16() and self._bf16_train_eligible()
        return cache["bf16_train"]

    def _bf16_train_eligible(self):
        """the layers ops.TRAIN_PRECISION = "bf16" moves ("bf16 training"): square, not anisotropic, dilated or grouped, 32 physical input
        channels or more (never the stem), every tap real, a stride that is a power of two (the bf16 kernels take no other), no cut
        output, not kept in fp32 (a softmax reads the output)"""
        fs = self.filter_shape
        st = self.stride[0]
        return (type(self) is ConvLayer and not self.direct and fs[2] == fs[3] and self.cp % 32 == 0 and self.s_pad == fs[3]
                and st > 0 and st & (st - 1) == 0 and self.ohw is None and not getattr(self, "fp32_only", False))

    def _settle_up(self, up):
        """after a forward pass on an un-written up-sampled input: the tensor if the pass had to make it, else still pending (the
        filter gradient asks for it on its own stream, anybody else through Act.data)"""
        if up is None:
            return
        if up.result is not None:
            self.input.data = up.result
        else:
            self.input.set_pending_data(up)

    def forward_folded(self, ctx, bn, add=None, relu=False, out_act=None):
        """inference only: this convolution with the batch-norm layer behind it folded into its filters (recomputed
        when the weights change), residual `add` and ReLU in the epilogue; writes the batch norm's output"""
        assert not getattr(bn, "norm_groups", 0), "a group-mode norm cannot be folded into the convolution in front of it"
        cache = self._cache()
        self._record_mode(cache, False)
        ent = cache.get("fold")
        if ent is None or ent[0] != ops.WEIGHTS_VERSION or ent[1] is not bn:
            w_f, b_f = ops.bn_fold(self._w(), self.beta.dev if self.use_bias else None, bn.omega.dev, bn.beta.dev,
                                   bn.mean.dev, bn.stdinv.dev, bn.eps)
            ent = cache["fold"] = (ops.WEIGHTS_VERSION, bn, w_f, b_f)
        if self.direct:
            fwd, _, _, kw = self._direct_calls()
            y = fwd(self.input.data, ent[2], bias=ent[3], add=add, logical=self._logical(), cache=cache, relu=relu, **kw)
            self.output.data = y
            (out_act if out_act is not None else bn.output).data = y
            return y
        link = self.input.take_pending_data()
        if isinstance(link, ops.NchwLink):
            self.input.set_pending_data(link)          # (see forward: the first layer reads the planar batch)
            if add is None and self.ohw is None and ops.conv_stem_ok(link.x, self.omega.dev_shape, self.stride[0], self.pad,
                                                                     self.filter_shape[3]):
                y = ops.conv_stem_fwd(link.x, ent[2], ent[3], cache, False, logical=self._logical(), relu=relu)
                self.output.data = y
                (out_act if out_act is not None else bn.output).data = y
                return y
        elif link is not None:
            self.input.data = link.materialise()
        y = ops.conv_fwd(self.input.data, ent[2], bias=ent[3], add=add, stride=self.stride[0], pad=self.pad,
                         s_real=self.filter_shape[3], logical=self._logical(), cache=cache, relu=relu, ohw=self.ohw)
        self.output.data = y
        (out_act if out_act is not None else bn.output).data = y
        return y

    def _backward_rect(self, ctx):
        """backward of a direct layer (anisotropic, dilated or grouped): filter gradient on the second stream, bias gradient by column
        sums, data gradient"""
        dy = self.output.grad
        x = self.input.data
        _, dgrad, wgrad, kw = self._direct_calls()
        if self.enabled and self.omega.grad is not None:
            with ops.wgrad_stream():
                wgrad(x, dy, self.omega.dev_shape, out=self.omega.grad.view(self.omega.dev_shape), logical=self._logical(), **kw)
                if self.use_bias:
                    ops.colsum(dy.view(-1, self.kp), out=self.beta.grad)
        if getattr(self.input, "requires_grad", True):
            self.input.grad = dgrad(dy, self._w(), tuple(x.shape), add=self.input.grad, logical=self._logical(), **kw)

    def backward(self, ctx):
        if self.direct:
            return self._backward_rect(ctx)
        # (the first layer on the planar network input has no data gradient and reads the image as it is)
        planar = getattr(self, "_planar_x", None) if not getattr(self.input, "requires_grad", True) else None
        # an input that is the un-written output of a pool-inverse layer (ops.UpLink, see forward): the data gradient needs its shape
        # only, the filter gradient makes the tensor on ITS stream (it has the time) unless the transformed input was kept
        up = self.input._pending_data if isinstance(self.input._pending_data, ops.UpLink) and self.input._data is None else None
        if up is not None and self.output._pending_grad is not None:
            up = None                             # (a linked batch-norm gradient: the one-kernel form reads x itself)
        x = self.input.data if (planar is None and up is None) else None
        x_shape = tuple(up.shape) if up is not None else (tuple(x.shape) if x is not None else None)
        st, pad, sr = self.stride[0], self.pad, self.filter_shape[3]
        # the batch norm (of this training step) whose output is this layer's input: the data-gradient pass below writes the
        # gradient of that output, and a Winograd pass can leave that batch norm's two backward reductions behind (ops.BnSums)
        sums = None
        bn = self.input.bn_producer
        bf16 = bool(self._cache().get("bf16_train"))      # (bf16 mode: that batch norm does its own reductions)
        if (ops.BWD_SUMS and bn is not None and not bf16 and self._cache().get("train") and getattr(self.input, "requires_grad", True)
                and not getattr(self, "not_last_writer", False)):
            sums = bn.sums_request(self.input)
        link = self.output.take_pending_grad()
        if link is not None:
            # the gradient of the output is the pending pointwise pass of a batch norm's backward (ops.BnLink): a 3x3 layer whose
            # data- and filter-gradient passes are Winograd passes forms it inside ONE transform kernel that feeds both
            fs = self.filter_shape
            if (self.enabled and self.omega.grad is not None and getattr(self.input, "requires_grad", True) and not self.use_bias
                    and not bf16 and fs[2] == 3 and fs[3] == 3 and st == 1 and self.stride[1] == 1 and pad == 1 and self.ohw is None):
                dx = ops.conv_backward_linked(link, x, self._w(), self.omega.dev_shape, self.input.grad,
                                              self.omega.grad.view(self.omega.dev_shape), self._cache(), stride=st, pad=pad,
                                              s_real=sr, logical=self._logical(), sums=sums)
                if dx is not None:
                    self.input.grad = dx
                    self.input.grad_sums = sums
                    return
            self.output.grad = link.materialise()
        dy = self.output.grad
        need_dx = getattr(self.input, "requires_grad", True)
        # two MFMA-bound GEMMs of hundreds of GFLOP gain nothing from sharing the chip (measured: the 4736 -> 1536 head layer's
        # pair takes 4.9 ms side by side, 2.1 + 2.2 ms one after the other) and the data gradient is the one the backward sweep
        # waits for: it goes first, the filter gradient follows on the second stream beside the HBM-bound passes that come next
        first = need_dx and sr == 1 and st == 1 and 2e-9 * dy.numel() * x_shape[-1] >= ops.DGRAD_FIRST_GFLOP
        if first:
            self.input.grad = ops.conv_dgrad(dy, self._w(), x_shape, add=self.input.grad, stride=st, pad=pad,
                                             s_real=sr, logical=self._logical(), cache=self._cache(), sums=sums, ohw=self.ohw)
            self.input.grad_sums = sums
        if self.enabled and self.omega.grad is not None:
            # the first layer of the network has no data gradient: its filter gradient is the tail of the backward sweep on the
            # second stream, and the bias column sums (a pass over the largest tensor of the network) run beside it on the
            # compute stream, which has nothing left to do, instead of behind it
            tail = not getattr(self.input, "requires_grad", True)
            with ops.wgrad_stream():        # independent of the data-gradient chain below
                if planar is not None:
                    ops.conv_stem_wgrad(planar, dy, self.omega.dev_shape, self.omega.grad.view(self.omega.dev_shape),
                                        logical=self._logical())
                else:
                    if up is not None:
                        x = self.input.data          # (written here, on the filter-gradient stream)
                    ops.conv_wgrad(x, dy, self.omega.dev_shape, stride=st, pad=pad, s_real=sr,
                                   out=self.omega.grad.view(self.omega.dev_shape), logical=self._logical(),
                                   cache=self._cache(), ohw=self.ohw)
                if self.use_bias and not tail:
                    ops.colsum(dy.view(-1, self.kp), out=self.beta.grad)
            if self.use_bias and tail:
                ops.colsum(dy.view(-1, self.kp), out=self.beta.grad)
        if need_dx and not first:
            self.input.grad = ops.conv_dgrad(dy, self._w(), x_shape, add=self.input.grad, stride=st, pad=pad,
                                             s_real=sr, logical=self._logical(), cache=self._cache(), sums=sums, ohw=self.ohw)
            self.input.grad_sums = sums
