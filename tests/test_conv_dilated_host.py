"""Dilated convolutions on the host: `C.D[k, size, stride, d]`, `C.DX[k, kh, kw, sh, sw, dh, dw]` and the dilated residual blocks
`RSN[k, size, stride, bottleneck, d]` / `nRSN[n, k, size, stride, bottleneck, d]` ("Dilated convolutions": this
build's own contract, the reference has no such parameter) parse, report the shapes of the effective extent ke = (k - 1) * d + 1,
survive the JSON / .mdl.gz round trip, are refused where the contract says so, and leave every undilated model exactly as it was.
No GPU needed."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from denet_amd import lib as dlib, ops
from denet_amd.layer.convolution import ConvLayer
from denet_amd.layer.resnet import ResnetLayer
from denet_amd.model import model_cnn, modify, zoo
from denet_amd.model.audit import conv_layers, decisions_cover, layer_geometry
from denet_amd.model.model_cnn import walk_layers

H, W = 19, 38
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undilated_export_keys.json")
MIXED = "C.B[32,3] BN A C.X[64,1,7] BN A C.X[64,7,1,2,1] BN A DC.X[32,3,1,2,1] C.X[32,3,3,1,2] BN A R"     # test_conv_rect_gpu.py's


def _build(desc, shape, border="half", batch=2):
    np.random.seed(0)
    m = model_cnn.ModelCNN()
    m.batch_size, m.class_num = batch, 4
    m.build(desc, shape, "relu", border, ["he-backward"])
    return m


def _padding(border, keh, kew):
    if isinstance(border, tuple):
        return border
    return {"valid": (0, 0), "half": (keh // 2, kew // 2), "full": (keh - 1, kew - 1), "same": (keh // 2, kew // 2)}[border]


# ------------------------------------------------------------------------------------------------- grammar
def test_tokens_parse_to_the_stated_layers():
    m = _build("C[32,3] C.D[32,3,1,2] C.DX[32,3,5,1,1,2,3] C.DB[64,3,1,4] C.DXB[32,2,3,1,1,3,2] nRSN.O[2,32,3,1,0,2]", (3, H, W))
    c0, a, b, c, d = m.layers[1:6]
    assert all(isinstance(l, ConvLayer) for l in (c0, a, b, c, d))
    assert c0.dilation == (1, 1) and not c0.dilated and not c0.direct and c0.pad == 1
    assert a.filter_shape == (32, 32, 3, 3) and a.stride == (1, 1) and a.dilation == (2, 2) and a.dilated and a.direct
    assert not a.anisotropic and a.pad == (2, 2) and not a.use_bias and a.output_shape == (2, 32, H, W)
    assert b.filter_shape == (32, 32, 3, 5) and b.stride == (1, 1) and b.dilation == (2, 3) and b.pad == (2, 6)
    assert b.output_shape == (2, 32, H, W)
    assert c.filter_shape == (64, 32, 3, 3) and c.dilation == (4, 4) and c.use_bias and c.pad == (4, 4)
    assert d.filter_shape == (32, 64, 2, 3) and d.dilation == (3, 2) and d.use_bias and d.pad == (2, 2)      # ke = 4 x 5
    assert d.output_shape == (2, 32, H + 4 - 4 + 1, W)
    # the filter and its initialisation bound do not know the dilation: a trained filter loads as it is
    assert a.omega.dev_shape == (32, 3, 3, 32) and a.w_bound == math.sqrt(2.0 / (3 * 3 * 32))
    blocks = m.layers[6:8]
    assert all(isinstance(l, ResnetLayer) and l.dilation == 2 and l.stride == (1, 1) for l in blocks)
    for blk in blocks:
        convs = [l for l in blk.layers if isinstance(l, ConvLayer)]
        assert len(convs) == 2 and all(l.dilation == (2, 2) and l.pad == (2, 2) and l.filter_shape[2:] == (3, 3) for l in convs)
        assert blk.output_shape == (2, 32, d.output_shape[2], W)
    # RSN: param 4; a bottleneck block dilates its middle convolution only, the projection shortcut stays as it is
    n = _build("C[32,3] RSN.O[64,3,1,32,3]", (3, H, W))
    blk = n.layers[2]
    convs = [l for l in blk.layers if isinstance(l, ConvLayer)]
    assert blk.dilation == 3 and [l.filter_shape[2:] for l in convs] == [(1, 1), (3, 3), (1, 1), (1, 1)]
    assert [l.dilation for l in convs] == [(1, 1), (3, 3), (1, 1), (1, 1)] and [l.direct for l in convs] == [False, True, False, False]
    assert [l.pad for l in convs] == [0, (3, 3), 0, 0]
    # the tag decides: without D the extra parameters are not a dilation
    plain = _build("C[32,3] C[32,3,1,2] nRSN.O[1,32,3]", (3, H, W))
    assert all(l.dilation == (1, 1) and not l.direct for l in walk_layers(plain.layers) if isinstance(l, ConvLayer))
    assert plain.layers[3].dilation == 1


@pytest.mark.parametrize("token", ["C.D[32,3,1,2]", "C.DX[32,3,5,1,1,2,3]", "C.DX[32,2,3,1,1,3,1]", "C.DX[32,1,5,2,1,1,2]",
                                   "C.D[32,3,1,4]"])
@pytest.mark.parametrize("border", ["valid", "half", "full", "same", (1, 1)])
def test_output_shape_on_the_effective_extent(token, border):
    nums = [int(v) for v in token[token.index("[") + 1:-1].split(",")]
    if ".DX" in token:
        K, R, S, sh, sw, dh, dw = nums
    else:
        K, R, S, sh, sw, dh, dw = nums[0], nums[1], nums[1], nums[2], nums[2], nums[3], nums[3]
    if border == "same" and (sh, sw) != (1, 1):
        with pytest.raises(AssertionError):          # `same` is defined for stride 1 (as for every other layer)
            _build("C[32,3] " + token, (3, H, W), border)
        return
    l = _build("C[32,3] " + token, (3, H, W), border).layers[2]
    h, w = l.input_shape[2:]
    keh, kew = (R - 1) * dh + 1, (S - 1) * dw + 1
    ph, pw = _padding(border, keh, kew)
    oh, ow = int(math.ceil((h + 2 * ph - keh + 1) / sh)), int(math.ceil((w + 2 * pw - kew + 1) / sw))
    if border == "same":
        oh, ow = h, w
    assert l.dilation == (dh, dw) and l.pad == (ph, pw) and l.output_shape == (2, K, oh, ow)
    y = Fn.conv2d(torch.zeros(2, 32, h, w, dtype=torch.float64), torch.zeros(K, 32, R, S, dtype=torch.float64), stride=(sh, sw),
                  padding=(ph, pw), dilation=(dh, dw))
    if border == "same":
        y = y[:, :, :h, :w]
    assert tuple(y.shape) == l.output_shape
    g, txt = layer_geometry(l)
    assert g == ops.conv_dil_geom((2, h, w, 32), (32, R, S, 32), (sh, sw), (ph, pw), (dh, dw), S, l.ohw)
    assert g == (2, h, w, 32, 32, R, S, S, sh, sw, ph, pw, dh, dw, oh, ow) and len(g) == 16
    assert txt == "%dx%d 32->%d %dx%d/%dx%d d%dx%d" % (h, w, K, R, S, sh, sw, dh, dw)


def test_dilation_on_an_extent_one_axis_reads_one():
    m = _build("C[32,3] C.DX[32,1,1,1,1,3,2] C.DX[32,1,3,2,1,5,1] C.D[32,1,2,4] C.DX[32,3,1,1,2,2,7]", (3, H, W))
    a, b, c, d = m.layers[2:6]
    assert a.dilation == (1, 1) and not a.dilated and not a.direct and a.pad == 0          # a 1x1 layer never leaves the square path
    assert len(layer_geometry(a)[0]) == 12
    assert b.dilation == (1, 1) and not b.dilated and b.anisotropic and b.direct           # rectangular for its own reasons
    assert len(layer_geometry(b)[0]) == 14
    assert c.dilation == (1, 1) and not c.direct and c.stride == (2, 2)                    # (the stride rule has nothing to refuse)
    assert d.dilation == (2, 1) and d.dilated and d.stride == (1, 2) and d.pad == (2, 0)
    for l in (a, b, c):
        assert "dilation" not in l.export_json()
    assert d.export_json()["dilation"] == (2, 1)


# ------------------------------------------------------------------------------------------------- round trips
DILATED = "C.B[32,3] BN A C.D[32,3,1,2] BN A nRSN.O[1,32,3,1,0,2] C.DX[64,3,3,1,1,1,2] BN A R"


def test_json_and_file_round_trip_keep_the_dilation(tmp_path):
    m = _build(DILATED, (3, 12, 16), batch=4)
    m.class_labels = {"c%i" % i: i for i in range(4)}
    want = [(1, 1), (2, 2), (2, 2), (2, 2), (1, 2), (1, 1)]
    assert [l.dilation for _, l in conv_layers(m)] == want
    js = m.export_json()
    assert [l.get("dilation") for l in js["layers"] if l["type"] in ("conv", "resnet")] == [None, (2, 2), 2, (1, 2), None]
    blk = [l for l in js["layers"] if l["type"] == "resnet"][0]
    assert [s.get("dilation") for s in blk["layers"] if s["type"] == "conv"] == [(2, 2), (2, 2)]
    path = str(tmp_path / "dilated.mdl.gz")
    model_cnn.save_to_file(m, path)
    for other in (model_cnn.load_from_json(js, 4), model_cnn.load_from_file(path, 4)):
        assert [l.output_shape for l in other.layers] == [l.output_shape for l in m.layers]
        assert [l.dilation for _, l in conv_layers(other)] == want
        assert [l.dilation for l in other.layers if l.type_name == "resnet"] == [2]
        for (_, a), (_, b) in zip(conv_layers(m), conv_layers(other)):
            assert b.pad == a.pad and b.direct == a.direct and b.ohw == a.ohw
            np.testing.assert_array_equal(b.omega.get_value(), a.omega.get_value())


def _keys(layers):
    out = []
    for l in layers:
        row = {"type": l["type"], "keys": sorted(l.keys())}
        if l.get("layers"):
            row["layers"] = _keys(l["layers"])
        out.append(row)
    return out


def test_undilated_models_export_no_new_key():
    """default models save what they saved before: no `dilation` key in any layer, and the key set of every layer is the one
    recorded before the key existed. tests/golden/undilated_export_keys.json is this project's own record, no reference involved:
    per layer (nested ones included) the type and the sorted keys of export_json() of the two models below, taken at the commit
    before this one"""
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
                assert "dilation" not in l, (name, l["type"])
                walk(l.get("layers") or [])
        walk(j["layers"])
        assert {"top": sorted(j.keys()), "layers": _keys(j["layers"])} == golden[name], name
        for l in walk_layers(m.layers):
            if isinstance(l, ConvLayer):
                assert l.dilation == (1, 1) and not l.dilated and l.direct == l.anisotropic
            if isinstance(l, ResnetLayer):
                assert l.dilation == 1


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("desc,shape,border,match", [
    ("C[32,3] C.D[32,3,1,0]", (3, H, W), "half", "integer >= 1"),
    ("C[32,3] C.D[32,3,1,-2]", (3, H, W), "half", "integer >= 1"),
    ("C[32,3] C.D[32,3,1,1.5]", (3, H, W), "half", "integer >= 1"),
    ("C[32,3] C.DX[32,3,3,1,1,2,0]", (3, H, W), "half", "integer >= 1"),
    ("C[32,3] C.D[32,3,2,2]", (3, H, W), "half", "stride 2.*stride 1 only"),
    ("C[32,3] C.DX[32,3,3,1,2,1,2]", (3, H, W), "half", "column dilation 2 with column stride 2"),
    ("C[32,3] C.DX[32,3,3,2,1,3,1]", (3, H, W), "half", "row dilation 3 with row stride 2"),
    ("C.D[32,3,1,2]", (3, H, W), "half", "32 physical input channels"),
    ("C[32,3] C.D[32,3,1,4]", (3, 9, 11), "valid", "effective filter extent 9 .*larger than the padded map's 7 rows"),
    ("C[32,3] C.DX[32,1,3,1,1,1,5]", (3, 9, 11), "valid", "effective filter extent 11 .*larger than the padded map's 9 columns"),
    ("C[32,3] nRSN.O[1,32,3,2,0,2]", (3, H, W), "half", "stride"),
    ("C[32,3] RSN.O[64,3,2,32,2]", (3, H, W), "half", "stride"),
    ("C[32,3] RSN.O[32,3,1,0,0]", (3, H, W), "half", "integer >= 1"),
    ("C[32,3] DC.D[16,3,1,2]", (3, H, W), "half", "transposed convolution takes no dilation"),
    ("C[32,3] DC.DX[16,3,1,2,1,2,2]", (3, H, W), "half", "transposed convolution takes no dilation"),
])
def test_refusals_name_the_cause(desc, shape, border, match):
    with pytest.raises(ValueError, match=match):
        _build(desc, shape, border)


def test_refusals_through_json():
    m = _build("C[32,3] C[32,3] DC[32,3]", (3, H, W))
    m.class_labels = {"a": 0}
    for index, value, match in ((1, (2, 2), None), (1, 0, "integer >= 1"), (1, [2, 2.5], "integer >= 1"), (1, (1, 2, 3), "pair"),
                                (1, True, "integer >= 1"), (0, 2, "32 physical input channels"),
                                (2, (2, 2), "transposed convolution takes no dilation")):
        js = m.export_json()
        js["layers"][index]["dilation"] = value
        if match is None:
            l = model_cnn.load_from_json(js, 2).layers[2]
            assert l.dilation == (2, 2) and l.direct and l.pad == (2, 2)
            np.testing.assert_array_equal(l.omega.get_value(), m.layers[2].omega.get_value())      # a trained filter loads as it is
        else:
            with pytest.raises(ValueError, match=match):
                model_cnn.load_from_json(js, 2)


# ------------------------------------------------------------------------------------------------- the paths a dilated layer takes
def test_dilated_layers_stay_off_the_square_path():
    m = _build(DILATED, (3, 12, 16), batch=4)
    rows = conv_layers(m)
    assert [l.direct for _, l in rows] == [False, True, True, True, True, True]           # (the head: a 12 x 16 `valid` filter)
    assert [l.dilated for _, l in rows] == [False, True, True, True, True, False]
    for _, l in rows:
        if l.dilated:
            assert not l._bf16_train_eligible()
            g, txt = layer_geometry(l)
            assert len(g) == 16 and g[12:14] == l.dilation and txt.endswith(" d%dx%d" % l.dilation)
            fwd, dgrad, wgrad, kw = l._direct_calls()
            assert (fwd, dgrad, wgrad) == (ops.conv_dil_fwd, ops.conv_dil_dgrad, ops.conv_dil_wgrad) and kw["dilation"] == l.dilation
    head = rows[-1][1]
    assert head._direct_calls()[:3] == (ops.conv_rect_fwd, ops.conv_rect_dgrad, ops.conv_rect_wgrad)
    assert "dilation" not in head._direct_calls()[3]
    # an undilated 3x3 layer of the same shape is eligible for the bf16 kernels; the dilation alone takes it off them
    plain = _build("C[32,3] C[32,3]", (3, 12, 16)).layers[2]
    assert plain._bf16_train_eligible() and not plain.direct
    # a dilated 3x3 stride-1 layer asks for no tuned decision
    three = _build("C[32,3] C.D[32,3,1,2] C[32,3]", (3, 12, 16))
    missing = decisions_cover(three)
    assert all(name != "2.conv" for name, _, _ in missing)
    # the drivers' start-up lines: one per dilated convolution, the nested ones included
    from denet_amd.layer import dilation_log_lines
    lines = dilation_log_lines(m)
    assert len(lines) == 4 and "dilation (2, 2)" in lines[0] and "d2x2" in lines[0] and "dilation (1, 2)" in lines[3]
    assert dilation_log_lines(_build("C[32,3] C[32,3]", (3, 12, 16))) == []


def test_modify_layer_sets_a_dilation():
    """--modify-layer conv dilation=...: the pair-typed attribute parses (`2` -> (2, 2), `2,3`), the edit goes through the JSON key"""
    stem = _build("C[32,3] C[32,3] BN A R", (3, 12, 16))
    stem.class_labels = {"c%i" % i: i for i in range(4)}
    with pytest.raises(ValueError, match="32 physical input channels"):        # the FIRST layer of the type: the one on the raw image
        modify.modify_layer(stem, "conv", ["dilation=2"])
    for text, want in (("dilation=2", (2, 2)), ("dilation=2,3", (2, 3))):
        m = _build("C[32,3] BN A R", (32, 12, 16))                             # a 32-channel input
        m.class_labels = {"c%i" % i: i for i in range(4)}
        w = m.layers[1].omega.get_value().copy()
        e = modify.modify_layer(m, "conv", [text])
        l = e.layers[1]
        assert l.dilation == want and l.pad == want and l.output_shape == m.layers[1].output_shape
        assert e.export_json()["layers"][0]["dilation"] == want
        np.testing.assert_array_equal(l.omega.get_value(), w)
    m = _build("C[32,3] BN A R", (32, 12, 16))
    m.class_labels = {"c%i" % i: i for i in range(4)}
    e = modify.modify_layer(m, "conv", ["stride=2"])                           # the other pair-typed attribute
    assert e.layers[1].stride == (2, 2)


# ------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_refuse_before_any_device_work():
    """argument validation happens before any HIP call: callable without a device (the pointers are never dereferenced)"""
    L = dlib.load()
    p = ctypes.c_void_p(4096)
    #            N  H   W   C   K   R  S  Sr sh sw ph pw dh dw OH  OW
    ok = (2, 12, 12, 32, 32, 3, 3, 3, 1, 1, 2, 2, 2, 2, 12, 12)
    cases = [(dict(dh=0), b"dh"), (dict(dw=-1), b"dw"), (dict(sh=2, OH=6), b"sh"), (dict(C=4, S=8), b"C"), (dict(OH=13), b"OH"),
             (dict(sw=2, OW=6), b"sw"), (dict(OW=13), b"OW")]
    names = ("N", "H", "W", "C", "K", "R", "S", "Sr", "sh", "sw", "ph", "pw", "dh", "dw", "OH", "OW")

    def geom(**kw):
        g = dict(zip(names, ok))
        g.update(kw)
        return [g[n] for n in names]

    for kw, word in cases:
        g = geom(**kw)
        for who, call in (("conv_dil_fwd", lambda: L.denet_conv_dil_fwd(p, p, None, None, p, 0, *g, None)),
                          ("conv_dil_dgrad", lambda: L.denet_conv_dil_dgrad(p, p, None, p, *g, None)),
                          ("conv_dil_wgrad", lambda: L.denet_conv_dil_wgrad(p, p, p, p, 1 << 30, *g, None))):
            rc = call()
            msg = L.denet_last_error()
            assert rc == -1000, (who, kw, rc)
            assert msg.startswith(who.encode() + b":") and word in msg[len(who) + 1:], (who, kw, msg)
    # the stride rule, the channel rule and the extent are named for what they are
    assert L.denet_conv_dil_fwd(p, p, None, None, p, 0, *geom(sh=2, OH=6), None) == -1000
    assert b"row stride sh must be 1 on a dilated axis" in L.denet_last_error()
    assert L.denet_conv_dil_fwd(p, p, None, None, p, 0, *geom(C=4, S=8), None) == -1000
    assert b"dilated filter needs physical C (4)" in L.denet_last_error()
    assert L.denet_conv_dil_fwd(p, p, None, None, p, 0, *geom(OH=13), None) == -1000
    assert b"OH=13 inconsistent" in L.denet_last_error()
    # ke = 9 on a 7-row map without padding
    assert L.denet_conv_dil_fwd(p, p, None, None, p, 0, *geom(H=7, ph=0, dh=4, OH=1), None) == -1000
    assert b"OH=1 inconsistent" in L.denet_last_error()
    # the rectangular twins keep their signatures: 14 geometry arguments, no dilation
    assert L.denet_conv_rect_fwd(p, p, None, None, p, 0, 2, 12, 12, 32, 32, 3, 3, 3, 3, 1, 1, 1, 4, 12, None) == -1000
    assert b"conv_rect_fwd: row stride sh must be a power of two" in L.denet_last_error()


def test_profile_record_names_the_dilated_kernel():
    assert ops.kernel_symbol(25, 1, 128, 64) == "conv_dil_kernel<1, 128, 64>"
    assert ops.kernel_symbol(20, 1, 128, 64) == "conv_rect_kernel<1, 128, 64>"


def test_geometry_refuses_an_extent_beyond_the_padded_map():
    with pytest.raises(ValueError, match="larger than the padded map"):
        ops.conv_dil_geom((2, 7, 9, 32), (32, 3, 3, 32), (1, 1), (0, 0), (4, 4))
    assert ops.conv_dil_geom((2, 7, 9, 32), (32, 3, 3, 32), (1, 1), (4, 4), (4, 4))[14:] == (7, 9)
