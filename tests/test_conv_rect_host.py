"""Rectangular filters and per-axis strides on the host: `C.X[k, kh, kw, sh, sw]` / `DC.X[...]` (reference: denet/layer/
convolution.py:55-80,99-112, deconvolution.py:54-60) build, report the reference's shapes, survive the JSON / .mdl.gz round trip,
and leave every square model exactly as it was. No GPU needed."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd.layer.convolution import ConvLayer
from denet_amd.layer.deconvolution import DeconvLayer
from denet_amd.layer.regression import RegressionLayer
from denet_amd.model import model_cnn, zoo
from denet_amd.model.audit import layer_geometry
from denet_amd.model.model_cnn import walk_layers

TOKENS = ["C.X[32,1,7]", "C.X[32,7,1]", "C.X[32,3,5,2,1]", "C.X[32,3,3,1,2]", "C.X[32,2,3]"]
H, W = 19, 38


def _build(desc, shape, border="half", batch=2):
    np.random.seed(0)
    m = model_cnn.ModelCNN()
    m.batch_size, m.class_num = batch, 4
    m.build(desc, shape, "relu", border, ["he-backward"])
    return m


def _padding(border, R, S):
    if isinstance(border, tuple):
        return border
    return {"valid": (0, 0), "half": (R // 2, S // 2), "full": (R - 1, S - 1), "same": (R // 2, S // 2)}[border]


@pytest.mark.parametrize("token", TOKENS)
@pytest.mark.parametrize("border", ["valid", "half", "full", "same", (1, 1)])
def test_output_shape_per_axis(token, border):
    """(1, 1) is what `--border-mode 1` hands to ModelCNN.build (model_cnn.initialize)"""
    nums = [int(v) for v in token[token.index("[") + 1:-1].split(",")]
    K, R, S = nums[:3]
    sh, sw = (nums[3], nums[4]) if len(nums) == 5 else (1, 1)
    if border == "same" and (sh, sw) != (1, 1):
        with pytest.raises(AssertionError):          # `same` is defined for stride 1 (as for the square layers)
            _build(token, (3, H, W), border)
        return
    m = _build(token, (3, H, W), border)
    l = m.layers[1]
    assert isinstance(l, ConvLayer) and l.filter_shape == (K, 3, R, S) and l.stride == (sh, sw)
    ph, pw = _padding(border, R, S)
    # the reference's formula (convolution.py:55-74) ...
    oh = int(math.ceil((H + 2 * ph - R + 1) / sh))
    ow = int(math.ceil((W + 2 * pw - S + 1) / sw))
    if border == "same":
        oh, ow = H, W
    assert l.output_shape == (2, K, oh, ow)
    # ... and what PyTorch's float64 conv2d returns for that padding
    y = Fn.conv2d(torch.zeros(2, 3, H, W, dtype=torch.float64), torch.zeros(K, 3, R, S, dtype=torch.float64), stride=(sh, sw),
                  padding=(ph, pw))
    if border == "same":
        y = y[:, :, :H, :W]
    assert tuple(y.shape) == l.output_shape
    assert l.anisotropic == (R != S or sh != sw or ph != pw)
    if l.anisotropic:
        assert l.pad == (ph, pw)
        g, txt = layer_geometry(l)
        assert g == (2, H, W, 4, 32, R, 8, S, sh, sw, ph, pw, oh, ow) and txt == "%dx%d 3->%d %dx%d/%dx%d" % (H, W, K, R, S, sh, sw)
    else:
        assert l.pad == ph
    # the first layer's device filter: S padded to 8 taps of the 4-channel input
    assert l.omega.dev_shape == (32, R, 8, 4)


def test_cli_border_mode_integer():
    """`--border-mode 1` pads one row and one column whatever the filter"""
    from denet_amd.model import train
    args = train.build_parser().parse_args(["--border-mode", "1", "--batch-size", "2", "--weight-init", "he-backward", "--model-desc",
                                            "C.X[32,1,7]", "C.X[32,3,5,2,1]"])
    np.random.seed(0)
    m = model_cnn.initialize(args, (3, H, W), {"a": 0, "b": 1}, 2)
    a, b = m.layers[1], m.layers[2]
    assert a.output_shape[2:] == (H + 2, W + 2 - 6) and a.pad == (1, 1) and a.anisotropic
    assert b.output_shape[2:] == (int(math.ceil((H + 2 + 2 - 3 + 1) / 2)), W - 4 + 2 - 5 + 1) and b.pad == (1, 1)


def test_deconv_output_shape_per_axis():
    m = _build("C[32,3] DC.X[16,3,1,2,1] DC.X[16,1,4,1,2]", (3, 16, 20))
    a, b = m.layers[2], m.layers[3]
    assert isinstance(a, DeconvLayer) and isinstance(b, DeconvLayer) and a.anisotropic and b.anisotropic
    # in * s - 2 * (k // 2) + k - 1 per axis (deconvolution.py:54-60)
    assert a.output_shape == (2, 16, 16 * 2 - 2 * 1 + 3 - 1, 20 * 1 - 0 + 1 - 1) == (2, 16, 32, 20)
    assert b.output_shape == (2, 16, 32 * 1 - 0 + 1 - 1, 20 * 2 - 2 * 2 + 4 - 1) == (2, 16, 32, 39)
    assert a.pad == (1, 0) and b.pad == (0, 2)
    assert a.omega.dev_shape == (32, 3, 1, 32) and b.omega.dev_shape == (32, 1, 4, 32)
    sq = _build("C[32,3] DC[16,4,2]", (3, 16, 20)).layers[2]
    assert not sq.anisotropic and sq.pad == 2 and sq.output_shape == (2, 16, 31, 39)


def test_head_behind_non_square_map():
    m = _build("C[32,3] R", (3, 16, 20))
    head, r = m.layers[2], m.layers[3]
    assert isinstance(head, ConvLayer) and isinstance(r, RegressionLayer)
    assert head.filter_shape == (4, 32, 16, 20) and head.border_mode == "valid" and head.anisotropic and head.pad == (0, 0)
    assert head.output_shape == (2, 4, 1, 1) and r.output_shape == (2, 4)
    m.build_train_func("sgd", skip_build=True)
    assert m.cost_layers == [r]


MIXED = "C.B[32,3] BN A C.X[64,1,7] BN A C.X[64,7,1,2,1] BN A DC.X[32,3,1,2,1] C.X[32,3,3,1,2] BN A R"


def test_mixed_model_shapes_and_round_trips(tmp_path):
    m = _build(MIXED, (3, 16, 24), batch=4)
    m.class_labels = {"c%i" % i: i for i in range(4)}
    convs = [l for l in m.layers if isinstance(l, (ConvLayer, DeconvLayer))]
    assert [l.output_shape[2:] for l in convs] == [(16, 24), (16, 24), (8, 24), (16, 24), (16, 12), (1, 1)]
    assert [l.anisotropic for l in convs] == [False, True, True, True, True, True]
    # layers that only pass shapes through accept the non-square maps
    for l in m.layers:
        if l.type_name in ("batchnorm", "activation"):
            assert l.output_shape == l.input_shape
    js = m.export_json()
    m2 = model_cnn.load_from_json(js, 4)
    path = str(tmp_path / "mixed.mdl.gz")
    model_cnn.save_to_file(m, path)
    m3 = model_cnn.load_from_file(path, 4)
    for other in (m2, m3):
        assert [type(l) for l in other.layers] == [type(l) for l in m.layers]
        assert [l.output_shape for l in other.layers] == [l.output_shape for l in m.layers]
        for a, b in zip(convs, [l for l in other.layers if isinstance(l, (ConvLayer, DeconvLayer))]):
            assert tuple(b.filter_shape) == tuple(a.filter_shape) and tuple(b.stride) == tuple(a.stride)
            assert b.border_mode == a.border_mode and b.pad == a.pad and b.anisotropic == a.anisotropic
            assert getattr(b, "ohw", None) == getattr(a, "ohw", None)
            np.testing.assert_array_equal(b.omega.get_value(), a.omega.get_value())
            # the device layout flips both axes independently and comes back
            np.testing.assert_array_equal(b.omega.from_dev_layout(b.omega.to_dev_layout()), a.omega.get_value())
    # a pair as the border mode survives as well
    p = _build("C.X[32,3,5]", (3, 16, 24), (2, 0))
    p.class_labels = {"a": 0}
    q = model_cnn.load_from_json(p.export_json(), 2)
    assert q.layers[1].pad == (2, 0) and q.layers[1].output_shape == p.layers[1].output_shape == (2, 32, 18, 20)


def test_passthrough_layers_on_non_square_maps():
    """pooling, skip-free residual blocks, split and dropout behind a rectangular layer build with per-axis shapes"""
    m = _build("C.X[32,3,5,2,1] BN A P[2,2] nRSN.O[1,32,3] D[0.5] P.A[2,2] R", (3, 32, 48))
    shapes = [l.output_shape[2:] for l in m.layers if len(l.output_shape) == 4]
    assert shapes[1] == (16, 48) and (8, 24) in shapes and shapes[-1] == (1, 1)
    head = [l for l in m.layers if isinstance(l, ConvLayer)][-1]
    assert head.filter_shape[2:] == (4, 12) and head.anisotropic


# every convolution of zoo.RESNET34_DESC at 224 x 224 as the parent commit builds it: (count, (output C x H x W, device filter
# [Kp][R][Sp][Cp], pad, stride, ohw)) in layer order
RESNET34_PARENT = [
    (1, ((64, 112, 112), (64, 7, 8, 4), 3, (2, 2), None)),
    (6, ((64, 56, 56), (64, 3, 3, 64), 1, (1, 1), None)),
    (1, ((128, 28, 28), (128, 3, 3, 64), 1, (2, 2), None)),
    (1, ((128, 28, 28), (128, 3, 3, 128), 1, (1, 1), None)),
    (1, ((128, 28, 28), (128, 1, 1, 64), 0, (2, 2), None)),
    (6, ((128, 28, 28), (128, 3, 3, 128), 1, (1, 1), None)),
    (1, ((256, 14, 14), (256, 3, 3, 128), 1, (2, 2), None)),
    (1, ((256, 14, 14), (256, 3, 3, 256), 1, (1, 1), None)),
    (1, ((256, 14, 14), (256, 1, 1, 128), 0, (2, 2), None)),
    (10, ((256, 14, 14), (256, 3, 3, 256), 1, (1, 1), None)),
    (1, ((512, 7, 7), (512, 3, 3, 256), 1, (2, 2), None)),
    (1, ((512, 7, 7), (512, 3, 3, 512), 1, (1, 1), None)),
    (1, ((512, 7, 7), (512, 1, 1, 256), 0, (2, 2), None)),
    (4, ((512, 7, 7), (512, 3, 3, 512), 1, (1, 1), None)),
    (1, ((1000, 1, 1), (1024, 1, 1, 512), 0, (1, 1), None)),
]
RESNET34_PARENT_TOP = [(3, 224, 224), (64, 112, 112), (64, 112, 112), (64, 112, 112), (64, 56, 56), (64, 56, 56), (64, 56, 56),
                       (64, 56, 56), (128, 28, 28), (128, 28, 28), (128, 28, 28), (128, 28, 28), (256, 14, 14), (256, 14, 14),
                       (256, 14, 14), (256, 14, 14), (256, 14, 14), (256, 14, 14), (512, 7, 7), (512, 7, 7), (512, 7, 7), (512, 1, 1),
                       (1000, 1, 1), (1000,)]


def test_square_model_is_untouched():
    m = zoo.resnet34(2, 224, 1000, seed=1)
    assert [tuple(l.output_shape[1:]) for l in m.layers] == RESNET34_PARENT_TOP
    convs = [l for l in walk_layers(m.layers) if l.type_name == "conv"]
    expect = [row for n, row in RESNET34_PARENT for _ in range(n)]
    assert len(convs) == len(expect) == 37
    for l, (out, dev, pad, stride, ohw) in zip(convs, expect):
        assert tuple(l.output_shape[1:]) == out and tuple(l.omega.dev_shape) == dev
        assert l.pad == pad and isinstance(l.pad, int) and tuple(l.stride) == stride and l.ohw == ohw
        assert l.anisotropic is False
        g, _ = layer_geometry(l)
        assert len(g) == 12                       # the square geometry tuple the tuned file is keyed by
