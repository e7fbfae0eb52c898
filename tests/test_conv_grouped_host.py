"""Grouped convolutions on the host: `C.G[k, size, stride, g]`, `C.GX[k, kh, kw, sh, sw, g]` and the grouped residual blocks
`RSN[k, size, stride, bottleneck, d, g]` / `nRSN[n, k, size, stride, bottleneck, d, g]` ("Grouped convolutions": this
build's own contract, the reference has no groups) parse to the stated layers, survive the JSON / .mdl.gz round trip, are refused
where the contract says so, stay off the square path, and leave every ungrouped model exactly as it was. No GPU needed."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import build as hip_build, lib as dlib, ops
from denet_amd.layer.convolution import ConvLayer
from denet_amd.layer.resnet import ResnetLayer
from denet_amd.model import model_cnn, zoo
from denet_amd.model.audit import conv_layers, decisions_cover, layer_geometry
from denet_amd.model.model_cnn import walk_layers
from grouped_reference import compact_ref, conv64_grouped, expand_ref

H, W = 12, 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undilated_export_keys.json")
MIXED = "C.B[32,3] BN A C.X[64,1,7] BN A C.X[64,7,1,2,1] BN A DC.X[32,3,1,2,1] C.X[32,3,3,1,2] BN A R"     # test_conv_rect_gpu.py's
RESNET50_DESC = ("C.B[64,7,2] BN A P[3,2,1] nRSN.O[3,256,3,1,64] nRSN.O[4,512,3,2,128] nRSN.O[6,1024,3,2,256] "
                 "nRSN.O[3,2048,3,2,512] P.A[7] R.TB")


def _build(desc, shape, border="half", batch=2, wb="he-backward"):
    np.random.seed(0)
    m = model_cnn.ModelCNN()
    m.batch_size, m.class_num = batch, 4
    m.build(desc, shape, "relu", border, [wb])
    return m


def _padding(border, r, s):
    return {"valid": (0, 0), "half": (r // 2, s // 2), "full": (r - 1, s - 1), "same": (r // 2, s // 2)}[border]


# ------------------------------------------------------------------------------------------------- the helper itself
def test_dense_twin_equals_grouped_conv2d_in_float64():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 7, 9, generator=g, dtype=torch.float64)
    w = torch.randn(64, 4, 3, 3, generator=g, dtype=torch.float64)
    twin = expand_ref(w, 16)
    assert twin.shape == (64, 64, 3, 3) and torch.equal(compact_ref(twin, 16), w)
    assert int((twin != 0).sum()) == w.numel()
    y = conv64_grouped(x, w, (1, 1), "half", 16)
    assert float((Fn.conv2d(x, twin.flip(2, 3), padding=1) - y).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- grammar
def test_tokens_parse_to_the_stated_layers():
    m = _build("C[64,3] C.G[64,3,1,4] C.GX[128,2,3,2,1,2] C.GB[128,3,2,128] C.GXB[64,1,5,1,2,2]", (3, H, W))
    c0, a, b, c, d = m.layers[1:6]
    assert all(isinstance(l, ConvLayer) for l in (c0, a, b, c, d))
    assert c0.groups == 1 and not c0.grouped and not c0.direct and c0.pad == 1
    assert a.filter_shape == (64, 16, 3, 3) and a.groups == 4 and a.grouped and a.direct and not a.anisotropic and a.pad == (1, 1)
    assert a.omega.dev_shape == (64, 3, 3, 16) and a.output_shape == (2, 64, H, W) and not a.use_bias
    assert b.filter_shape == (128, 32, 2, 3) and b.groups == 2 and b.stride == (2, 1) and b.omega.dev_shape == (128, 2, 3, 32)
    assert b.pad == (1, 1) and b.output_shape == (2, 128, (H + 2 - 2) // 2 + 1, W)
    assert c.filter_shape == (128, 1, 3, 3) and c.groups == 128 and c.use_bias and c.omega.dev_shape == (128, 3, 3, 1)
    assert c.stride == (2, 2)
    assert d.filter_shape == (64, 64, 1, 5) and d.groups == 2 and d.use_bias and d.stride == (1, 2) and d.omega.dev_shape == (64, 1, 5, 64)
    # the initialisation bound is the filter's own: he-backward R*S*K, he-forward the true fan-in R*S*Cg
    assert a.w_bound == math.sqrt(2.0 / (3 * 3 * 64))
    f = _build("C[64,3] C.G[64,3,1,4]", (3, H, W), wb="he-forward").layers[2]
    assert f.w_bound == math.sqrt(2.0 / (3 * 3 * 16))
    # ... and the numpy.random call sequence is the one of size = filter_shape
    np.random.seed(0)
    np.random.normal(0.0, c0.w_bound, size=c0.filter_shape)
    want = np.random.normal(0.0, a.w_bound, size=(64, 16, 3, 3)).astype(np.float32)
    np.testing.assert_array_equal(a.omega.get_value(), want)
    assert ops.conv_grp_window(64, 64, 4) == (32, 32, 16) and ops.conv_grp_window(64, 128, 2) == (32, 64, 0)
    assert ops.conv_grp_window(128, 128, 128) == (32, 32, 1) and ops.conv_grp_window(192, 192, 2) == (96, 96, 0)


def test_both_block_kinds():
    # a basic block groups both convolutions, a bottleneck its middle one; the 1x1 layers and the projection stay dense
    m = _build("C[64,3] nRSN.O[2,64,3,1,0,1,4] RSN.O[128,3,2,64,1,8] RSN.O[128,1,1,0,1,8]", (3, H, W))
    for blk in m.layers[2:4]:
        convs = [l for l in blk.layers if isinstance(l, ConvLayer)]
        assert isinstance(blk, ResnetLayer) and blk.groups == 4 and blk.dilation == 1 and blk.filter_shape == (64, 64, 3, 3)
        assert [l.filter_shape for l in convs] == [(64, 16, 3, 3)] * 2 and [l.groups for l in convs] == [4, 4]
        assert all(l.direct for l in convs)
    blk = m.layers[4]
    convs = [l for l in blk.layers if isinstance(l, ConvLayer)]
    assert blk.groups == 8 and blk.stride == (2, 2) and blk.output_shape == (2, 128, H // 2, W // 2)
    assert [l.filter_shape for l in convs] == [(64, 64, 1, 1), (64, 8, 3, 3), (128, 64, 1, 1), (128, 64, 1, 1)]
    assert [l.groups for l in convs] == [1, 8, 1, 1] and [l.direct for l in convs] == [False, True, False, False]
    assert [l.stride for l in convs] == [(2, 2), (1, 1), (1, 1), (2, 2)]
    # a block of extent 1 has no convolution to group
    assert all(l.groups == 1 for l in m.layers[5].layers if isinstance(l, ConvLayer)) and m.layers[5].groups == 8
    # the tag decides: without G the extra parameter is no group count
    plain = _build("C[64,3] C[64,3,1,4] nRSN.O[1,64,3]", (3, H, W))
    assert all(l.groups == 1 and not l.grouped for l in walk_layers(plain.layers) if isinstance(l, ConvLayer))
    assert plain.layers[3].groups == 1


@pytest.mark.parametrize("token", ["C.G[64,3,1,4]", "C.GX[128,2,3,2,1,2]", "C.GX[64,1,5,1,2,64]", "C.G[64,3,2,16]", "C.G[64,1,1,2]"])
@pytest.mark.parametrize("border", ["valid", "half", "full", "same"])
def test_output_shape_is_the_dense_layers(token, border):
    nums = [int(v) for v in token[token.index("[") + 1:-1].split(",")]
    if ".GX" in token:
        K, R, S, sh, sw, g = nums
    else:
        K, R, S, sh, sw, g = nums[0], nums[1], nums[1], nums[2], nums[2], nums[3]
    dense = "C.X[%d,%d,%d,%d,%d]" % (K, R, S, sh, sw)
    if border == "same" and (sh, sw) != (1, 1):
        with pytest.raises(AssertionError):          # `same` is defined for stride 1 (as for every other layer)
            _build("C[64,3] " + token, (3, H, W), border)
        return
    l = _build("C[64,3] " + token, (3, H, W), border).layers[2]
    twin = _build("C[64,3] " + dense, (3, H, W), border).layers[2]
    h, w = l.input_shape[2:]
    ph, pw = _padding(border, R, S)
    assert l.groups == g and l.direct and l.pad == (ph, pw) and l.output_shape == twin.output_shape and l.ohw == twin.ohw
    assert l.filter_shape == (K, 64 // g, R, S) and l.omega.dev_shape == (K, R, S, 64 // g)
    y = conv64_grouped(torch.zeros(2, 64, h, w, dtype=torch.float64), torch.zeros(K, 64 // g, R, S, dtype=torch.float64), (sh, sw),
                       border, g)
    assert tuple(y.shape) == l.output_shape
    geom, txt = layer_geometry(l)
    Cw, Kw, slab = ops.conv_grp_window(64, K, g)
    assert geom == (2, h, w, 64, K, Cw, Kw, R, S, S, sh, sw, ph, pw) + l.output_shape[2:] and len(geom) == 16
    assert txt == "%dx%d 64->%d %dx%d/%dx%d g%d" % (h, w, K, R, S, sh, sw, g)


def test_one_group_is_the_untagged_layer():
    a = _build("C[64,3] C.G[64,3,1,1] C.GX[64,3,3,2,2,1] nRSN.O[1,64,3,1,0,1,1]", (3, H, W))
    b = _build("C[64,3] C[64,3,1] C.X[64,3,3,2,2] nRSN.O[1,64,3,1,0,1]", (3, H, W))
    la, lb = [l for l in walk_layers(a.layers) if isinstance(l, ConvLayer)], [l for l in walk_layers(b.layers) if isinstance(l, ConvLayer)]
    assert len(la) == len(lb) == 5
    for x, y in zip(la, lb):
        assert x.groups == 1 and not x.grouped and not x.direct and x.pad == y.pad and type(x.pad) is int
        assert (x.filter_shape, x.stride, x.omega.dev_shape, x.output_shape, x.w_bound) == (
            y.filter_shape, y.stride, y.omega.dev_shape, y.output_shape, y.w_bound)
        np.testing.assert_array_equal(x.omega.get_value(), y.omega.get_value())
        assert "groups" not in x.export_json() and sorted(x.export_json()) == sorted(y.export_json())
        assert len(layer_geometry(x)[0]) == 12
    assert a.layers[4].groups == 1 and "groups" not in a.layers[4].export_json()


# ------------------------------------------------------------------------------------------------- round trips
GROUPED = "C.B[64,3] BN A C.G[64,3,1,4] BN A nRSN.O[1,128,3,2,64,1,8] C.GX[128,3,1,1,1,128] BN A C.G[128,3,1,2] BN A R"


def test_json_and_file_round_trip_keep_the_groups(tmp_path):
    m = _build(GROUPED, (3, 16, 16), batch=4)
    m.class_labels = {"c%i" % i: i for i in range(4)}
    want = [1, 4, 1, 8, 1, 1, 128, 2, 1]
    assert [l.groups for _, l in conv_layers(m)] == want
    js = m.export_json()
    assert [l.get("groups") for l in js["layers"] if l["type"] in ("conv", "resnet")] == [None, 4, 8, 128, 2, None]
    blk = [l for l in js["layers"] if l["type"] == "resnet"][0]
    assert [s.get("groups") for s in blk["layers"] if s["type"] == "conv"] == [None, 8, None, None]
    assert [tuple(l["shape"]) for l in js["layers"] if l["type"] == "conv"][1] == (64, 16, 3, 3)      # "shape" is (K, Cg, R, S)
    assert tuple(blk["shape"]) == (128, 64, 3, 3)                                                      # the block's own
    path = str(tmp_path / "grouped.mdl.gz")
    model_cnn.save_to_file(m, path)
    for other in (model_cnn.load_from_json(js, 4), model_cnn.load_from_file(path, 4)):
        assert [l.output_shape for l in other.layers] == [l.output_shape for l in m.layers]
        assert [l.groups for _, l in conv_layers(other)] == want
        assert [l.groups for l in other.layers if l.type_name == "resnet"] == [8]
        for (_, a), (_, b) in zip(conv_layers(m), conv_layers(other)):
            assert b.pad == a.pad and b.direct == a.direct and b.filter_shape == a.filter_shape
            assert b.omega.dev_shape == a.omega.dev_shape
            np.testing.assert_array_equal(b.omega.get_value(), a.omega.get_value())


def _keys(layers):
    out = []
    for l in layers:
        row = {"type": l["type"], "keys": sorted(l.keys())}
        if l.get("layers"):
            row["layers"] = _keys(l["layers"])
        out.append(row)
    return out


def test_ungrouped_models_export_no_new_key():
    """default models save what they saved before: the key set of every layer is the one recorded in
    tests/golden/undilated_export_keys.json (this project's own record, taken before the `dilation` and `groups` keys existed)"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    np.random.seed(0)
    mixed = model_cnn.ModelCNN()
    mixed.batch_size, mixed.class_num = 4, 4
    mixed.build(MIXED, (3, 16, 24), "relu", "half", ["he-backward"])
    for name, m in (("denet34_skip_128", zoo.denet34(2, "skip", image=128, class_num=5, seed=1)), ("mixed", mixed)):
        j = m.export_json()

        def walk(ls):
            for l in ls:
                assert "groups" not in l, (name, l["type"])
                walk(l.get("layers") or [])
        walk(j["layers"])
        assert {"top": sorted(j.keys()), "layers": _keys(j["layers"])} == golden[name], name
        for l in walk_layers(m.layers):
            if isinstance(l, ConvLayer):
                assert l.groups == 1 and not l.grouped and l.direct == l.anisotropic
            if isinstance(l, ResnetLayer):
                assert l.groups == 1


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("desc,shape,match", [
    ("C[64,3] C.G[64,3,1,0]", (3, H, W), "integer >= 1"),
    ("C[64,3] C.G[64,3,1,-2]", (3, H, W), "integer >= 1"),
    ("C[64,3] C.G[64,3,1,1.5]", (3, H, W), "integer >= 1"),
    ("C[64,3] C.GX[64,3,3,1,1,0]", (3, H, W), "integer >= 1"),
    ("C[64,3] C.G[64,3,1,3]", (3, H, W), "groups 3 does not divide both channel counts"),
    ("C[64,3] C.G[96,3,1,64]", (3, H, W), "groups 64 does not divide both channel counts"),
    ("C[96,3] C.G[96,3,1,4]", (3, H, W), "unsupported group size \\(24 input, 24 output"),          # Cg = 24
    ("C[64,3] C.G[128,3,1,64]", (3, H, W), "unsupported group size \\(1 input, 2 output"),          # a depthwise multiplier
    ("C[64,3] C.G[128,3,1,4]", (3, H, W), "unsupported group size \\(16 input, 32 output"),
    ("C[48,3] C.G[48,3,1,3]", (3, H, W), "no padded channels"),
    ("C[64,3] C.G[48,3,1,4]", (3, H, W), "no padded channels"),
    ("C[64,3] C.G[64,3,3,4]", (3, H, W), "stride 3 of a grouped layer must be a power of two"),
    ("C[64,3] C.GD[64,3,1,2]", (3, H, W), "G tag together with the D tag"),
    ("C[64,3] C.DGX[64,3,3,1,1,2]", (3, H, W), "G tag together with the D tag"),
    ("C.G[63,3,1,3]", (3, H, W), "32 physical input channels"),
    ("C[64,3] RSN.O[64,3,1,0,2,4]", (3, H, W), "grouped block is not dilated"),
    ("C[64,3] nRSN.O[1,128,3,1,64,2,8]", (3, H, W), "grouped block is not dilated"),
    ("C[64,3] RSN.O[64,3,1,0,1,0]", (3, H, W), "integer >= 1"),
    ("C[64,3] RSN.O[64,3,1,0,1,3]", (3, H, W), "groups 3 does not divide both channel counts"),
    ("C[64,3] RSN.O[128,3,1,96,1,4]", (3, H, W), "unsupported group size \\(24 input, 24 output"),
    ("C[64,3] DC.G[32,3,1,2]", (3, H, W), "transposed convolution takes no groups"),
    ("C[64,3] DC.GX[32,3,1,2,1,2]", (3, H, W), "transposed convolution takes no groups"),
])
def test_refusals_name_the_cause(desc, shape, match):
    with pytest.raises(ValueError, match=match):
        _build(desc, shape)


def test_refusals_through_json():
    m = _build("C[64,3] C[64,3] DC[32,3] nRSN.O[1,64,3]", (3, H, W))
    m.class_labels = {"a": 0}
    w = m.layers[2].omega.get_value()

    def edit(index, groups, shape=None, dilation=None):
        js = m.export_json()
        js["layers"][index]["groups"] = groups
        if shape is not None:
            js["layers"][index]["shape"] = shape
            js["layers"][index]["weight"] = np.ascontiguousarray(w[:, :shape[1]])
        if dilation is not None:
            js["layers"][index]["dilation"] = dilation
        return js

    l = model_cnn.load_from_json(edit(1, 4, (64, 16, 3, 3)), 2).layers[2]
    assert l.groups == 4 and l.direct and l.pad == (1, 1) and l.omega.dev_shape == (64, 3, 3, 16)
    np.testing.assert_array_equal(l.omega.get_value(), w[:, :16])
    l = model_cnn.load_from_json(edit(1, 4, (64, 16, 3, 3), dilation=(1, 1)), 2).layers[2]      # dilation (1, 1) is no dilation
    assert l.groups == 4 and not l.dilated
    assert model_cnn.load_from_json(edit(1, 1), 2).layers[2].direct is False                     # one group: the layer it was
    for js, match in ((edit(1, 0), "integer >= 1"), (edit(1, True), "integer >= 1"), (edit(1, 2.0), "integer >= 1"),
                      (edit(1, "4"), "integer >= 1"),
                      (edit(1, 4), "groups 4 does not divide both channel counts"),               # the dense shape with a group count
                      (edit(1, 3, (64, 21, 3, 3)), "groups 3 does not divide both channel counts"),
                      (edit(1, 4, (64, 16, 3, 3), dilation=(2, 2)), "a grouped layer is not dilated"),
                      (edit(2, 2), "transposed convolution takes no groups"),
                      (edit(3, 0), "integer >= 1"), (edit(3, 4, dilation=2), "grouped block is not dilated")):
        with pytest.raises(ValueError, match=match):
            model_cnn.load_from_json(js, 2)
    # a grouped layer on the raw image
    raw = _build("C[63,3]", (3, H, W))
    raw.class_labels = {"a": 0}
    js = raw.export_json()
    js["layers"][0].update(groups=3, shape=(63, 1, 3, 3), weight=np.ascontiguousarray(raw.layers[1].omega.get_value()[:, :1]))
    with pytest.raises(ValueError, match="32 physical input channels"):
        model_cnn.load_from_json(js, 2)


# ------------------------------------------------------------------------------------------------- the paths a grouped layer takes
def test_grouped_layers_stay_off_the_square_path(monkeypatch):
    m = _build(GROUPED, (3, 16, 16), batch=4)
    rows = conv_layers(m)
    assert [l.grouped for _, l in rows] == [False, True, False, True, False, False, True, True, False]
    assert [l.direct for _, l in rows][:8] == [False, True, False, True, False, False, True, True]
    for _, l in rows:
        if l.grouped:
            assert not l._bf16_train_eligible()
            g, txt = layer_geometry(l)
            assert len(g) == 16 and txt.endswith(" g%d" % l.groups)
            fwd, dgrad, wgrad, kw = l._direct_calls()
            assert fwd is ops.conv_grp_fwd and wgrad is ops.conv_grp_wgrad and dgrad.func is ops.conv_grp_dgrad
            assert dgrad.keywords["cache"] is l._cache() and kw["groups"] == l.groups and "dilation" not in kw
    # an ungrouped 3x3 layer of the same shape is eligible for the bf16 kernels; the groups alone take it off them
    plain = _build("C[64,3] C[64,3]", (3, 12, 16)).layers[2]
    assert plain._bf16_train_eligible() and not plain.direct
    # a grouped 3x3 stride-1 layer asks for no tuned decision, and no tuned table is read for it
    three = _build("C[64,3] C.G[64,3,1,4] C[64,3]", (3, 12, 16))
    looked = []
    real = ops.conv_geom
    monkeypatch.setattr(ops, "conv_geom", lambda *a, **k: looked.append(a) or real(*a, **k))
    missing = decisions_cover(three)
    assert all(name != "2.conv" for name, _, _ in missing)
    assert all(a[1] != three.layers[2].omega.dev_shape for a in looked)            # its geometry never reaches the square path's
    from denet_amd.layer import groups_log_lines
    lines = groups_log_lines(m)
    assert len(lines) == 4 and "4 groups" in lines[0] and "g4" in lines[0] and "128 groups" in lines[2]
    assert groups_log_lines(_build("C[64,3] C[64,3]", (3, 12, 16))) == []


# ------------------------------------------------------------------------------------------------- recipes
def _trained(m):
    """trained parameters, K * Cg * R * S per filter: the reference-layout values, no device padding"""
    return sum(int(np.prod(p.value.shape)) for l in m.layers for p in l.weights() + l.biases())


def test_parameter_counts():
    """ResNeXt-50 32x4d: the published 25 028 904 plus the 64 biases of this grammar's `C.B` stem; the ResNet-50 desc by the same
    count: 25 557 032 + 64"""
    m = zoo.resnext50(2)
    assert _trained(m) == 25028968
    grouped = [l for _, l in conv_layers(m) if l.grouped]
    assert len(grouped) == 16 and all(l.groups == 32 and l.filter_shape[2:] == (3, 3) for l in grouped)
    assert sorted({l.filter_shape[1] for l in grouped}) == [4, 8, 16, 32]
    np.random.seed(1)
    r = model_cnn.ModelCNN()
    r.batch_size, r.class_num = 2, 1000
    r.build(RESNET50_DESC, (3, 224, 224), "relu", "half", ["he-backward"])
    assert _trained(r) == 25557096


def test_denet_on_resnext101_builds():
    m = zoo.denet101(2, "skip", backbone_desc=zoo.RESNEXT101_DESC)
    grouped = [l for _, l in conv_layers(m) if l.grouped]
    assert len(grouped) == 33 and all(l.groups == 32 for l in grouped)
    plain = zoo.denet101(2, "skip")
    assert [l.type_name for l in m.layers] == [l.type_name for l in plain.layers]
    assert [l.output_shape for l in m.layers] == [l.output_shape for l in plain.layers]


# ------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_refuse_before_any_device_work():
    """argument validation happens before any HIP call: callable without a device (the pointers are never dereferenced)"""
    L = dlib.load()
    p = ctypes.c_void_p(4096)
    names = ("N", "H", "W", "C", "K", "Cw", "Kw", "R", "S", "Sr", "sh", "sw", "ph", "pw", "OH", "OW")
    ok = (2, 12, 12, 64, 128, 32, 64, 3, 3, 3, 1, 1, 1, 1, 12, 12)

    def geom(**kw):
        g = dict(zip(names, ok))
        g.update(kw)
        return [g[n] for n in names]

    cases = [(dict(Cw=16), b"window Cw (16) must be a positive multiple of 32"), (dict(Kw=48), b"window Kw (48) must be a positive"),
             (dict(Cw=0), b"window Cw (0)"), (dict(C=96, Cw=64), b"window Cw (64) does not divide C (96)"),
             (dict(K=96, Kw=64), b"window Kw (64) does not divide K (96)"), (dict(Kw=32), b"2 input windows"),
             (dict(Cw=64, Kw=64), b"1 input windows"), (dict(sh=3, OH=4), b"row stride sh must be a power of two"),
             (dict(sw=3, OW=4), b"column stride sw must be a power of two"), (dict(Sr=2), b"S_real (2) != S (3)"),
             (dict(C=48, Cw=48), b"physical C (48) must be a multiple of 32"), (dict(OH=13), b"OH=13 inconsistent")]
    for kw, word in cases:
        g = geom(**kw)
        for who, call in (("conv_grp_fwd", lambda: L.denet_conv_grp_fwd(p, p, None, None, p, 0, *g, None)),
                          ("conv_grp_dgrad", lambda: L.denet_conv_grp_dgrad(p, p, None, p, *g, None)),
                          ("conv_grp_wgrad", lambda: L.denet_conv_grp_wgrad(p, p, p, p, 1 << 30, *g, None))):
            rc = call()
            msg = L.denet_last_error()
            assert rc == -1000, (who, kw, rc)
            assert msg.startswith(who.encode() + b":") and word in msg[len(who) + 1:], (who, kw, msg)
    g = geom()
    for who, call in (("conv_grp_fwd", lambda: L.denet_conv_grp_fwd(None, p, None, None, p, 0, *g, None)),
                      ("conv_grp_dgrad", lambda: L.denet_conv_grp_dgrad(p, None, None, p, *g, None)),
                      ("conv_grp_wgrad", lambda: L.denet_conv_grp_wgrad(p, p, None, p, 1 << 30, *g, None))):
        assert call() == -1000 and L.denet_last_error() == who.encode() + b": null tensor", who
    # the slices of the pixel reduction need their workspace: 2 x 56 x 56 pixels are 196 chunks, more than one slice
    big = geom(H=56, W=56, OH=56, OW=56)
    need = L.denet_conv_grp_wgrad_workspace_bytes(2, 64, 128, 32, 64, 3, 3, 56, 56)
    assert need > 0 and need % (128 * 3 * 3 * 32 * 4) == 0
    assert need == 2 * L.denet_conv_rect_wgrad_workspace_bytes(2, 32, 64, 3, 3, 56, 56)      # the window's slices, for both windows
    assert L.denet_conv_grp_wgrad_workspace_bytes(2, 64, 128, 64, 128, 3, 3, 56, 56) == L.denet_conv_rect_wgrad_workspace_bytes(
        2, 64, 128, 3, 3, 56, 56)
    assert L.denet_conv_grp_wgrad_workspace_bytes(2, 64, 128, 0, 64, 3, 3, 56, 56) == 0
    for ws, nbytes in ((None, need), (p, need - 4)):
        assert L.denet_conv_grp_wgrad(p, p, p, ws, nbytes, *big, None) == -1000
        assert b"conv_grp_wgrad: workspace of" in L.denet_last_error() and b"denet_conv_grp_wgrad_workspace_bytes" in L.denet_last_error()
    # expand / compact
    for who, fn in (("conv_grp_expand", L.denet_conv_grp_expand), ("conv_grp_compact", L.denet_conv_grp_compact)):
        for args, word in (((p, p, 64, 3, 3, 3), b"Cg must be 1, 2, 4, 8 or 16 (got 3)"), ((p, p, 64, 3, 3, 32), b"(got 32)"),
                           ((p, p, 64, 3, 3, 0), b"(got 0)"), ((p, p, 48, 3, 3, 4), b"K (48) must be a positive multiple of 32"),
                           ((p, p, 64, 0, 3, 4), b"non-positive filter extent"), ((None, p, 64, 3, 3, 4), b"null tensor"),
                           ((p, None, 64, 3, 3, 4), b"null tensor")):
            assert fn(*args, None) == -1000, (who, args)
            msg = L.denet_last_error()
            assert msg.startswith(who.encode() + b":") and word in msg, (who, args, msg)
    # the rectangular twins keep their signatures
    assert L.denet_conv_rect_fwd(p, p, None, None, p, 0, 2, 12, 12, 32, 32, 3, 3, 3, 3, 1, 1, 1, 4, 12, None) == -1000
    assert b"conv_rect_fwd: row stride sh must be a power of two" in L.denet_last_error()


def test_window_rules_of_the_python_side():
    for args, match in (((64, 64, 0), "integer >= 1"), ((64, 64, 2.0), "integer >= 1"), ((64, 64, 3), "does not divide"),
                        ((96, 96, 4), "unsupported group size"), ((64, 128, 64), "unsupported group size"),
                        ((48, 48, 3), "multiples of 32")):
        with pytest.raises(ValueError, match=match):
            ops.conv_grp_window(*args)
    g, slab = ops.conv_grp_geom((2, 7, 9, 64), (64, 3, 3, 4), 16, (2, 1), (1, 1))
    assert g == (2, 7, 9, 64, 64, 32, 32, 3, 3, 3, 2, 1, 1, 1, 4, 9) and slab == 4


def test_profile_record_names_the_grouped_kernel():
    assert ops.kernel_symbol(26, 1, 128, 64) == "conv_grp_kernel<1, 128, 64>"
    assert ops.kernel_symbol(25, 1, 128, 64) == "conv_dil_kernel<1, 128, 64>"
    assert ops.kernel_symbol(20, 1, 128, 64) == "conv_rect_kernel<1, 128, 64>"


def test_no_new_translation_unit():
    assert "conv_rect.hip" in hip_build.SOURCES and not [s for s in hip_build.SOURCES if "grp" in s or "group" in s]
    with open(os.path.join(hip_build.CSRC, "conv_rect.hip")) as f:
        text = f.read()
    assert "conv_grp_kernel" in text and "grp_expand_kernel" in text and "grp_compact_kernel" in text
