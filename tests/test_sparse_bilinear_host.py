"""Opt-in bilinear RoI sampling of the DNS layer (tapRule 2, `DNS.I`; csrc/sparse_bilinear.hip), the part
that needs no GPU: the desc tag, the JSON key, model-modify, the C-ABI surface and the refusals of the entry points."""

import pytest

import cabi
from denet_amd import lib as dlib, ops
from denet_amd.layer import denet_sparse as DS
from denet_amd.model import model_cnn, modify

NAMES = ("denet_sparse_bilinear_fwd", "denet_sparse_bilinear_workspace_bytes", "denet_sparse_bilinear_sort",
         "denet_sparse_bilinear_bwd")


def _model(dns="DNS[3,4,0.01,0.1]"):
    import numpy
    numpy.random.seed(0)
    model = model_cnn.ModelCNN()
    model.batch_size, model.class_num = 2, 3
    model.build("C[32,3] DNC[8,10] %s C[32,1] DND[0.5,1,1]" % dns, (3, 16, 16), "relu", "half", ["he-backward"])
    return model


def _dns(model):
    return [l for l in model.layers if l.type_name == "denet-sparse"][0]


def _dns_json(model):
    return [l for l in model.export_json()["layers"] if l["type"] == "denet-sparse"][0]


def test_desc_tag_I_sets_rule_2():
    assert DS.TAP_BILINEAR == 2
    plain, inter, gi, g = (_dns(_model(d)) for d in ("DNS[3,4,0.01,0.1]", "DNS.I[3,4,0.01,0.1]", "DNS.GI[3,4,0.01,0.1]", "DNS.G[3,4,0.01,0.1]"))
    assert plain.tap_rule == 0 and plain.sample_gt
    assert inter.tap_rule == 2 and inter.sample_gt
    assert gi.tap_rule == 2 and not gi.sample_gt
    assert g.tap_rule == 0 and not g.sample_gt
    assert (inter.grid_size, inter.sample_num, inter.corner_threshold, inter.random_sample) == (3, 4, 0.01, 0.1)


def test_default_layer_exports_no_tap_rule_key():
    j = _dns_json(_model())
    assert "tapRule" not in j
    assert {"gridSize", "sampleNum", "sampleGT", "localMax", "cornerThreshold", "randomSample", "nmsThreshold", "version"} <= set(j)


@pytest.mark.parametrize("rule", [1, 2])
def test_json_rule_survives_export_and_reload(rule):
    model = _model()
    j = model.export_json()
    [l for l in j["layers"] if l["type"] == "denet-sparse"][0]["tapRule"] = rule
    loaded = model_cnn.load_from_json(j, 2)
    assert _dns(loaded).tap_rule == rule
    assert _dns_json(loaded)["tapRule"] == rule
    again = model_cnn.load_from_json(loaded.export_json(), 2)
    assert _dns(again).tap_rule == rule


@pytest.mark.parametrize("bad", [3, -1, 2.5, "2", True])
def test_unknown_rule_is_refused_when_the_layer_is_built(bad):
    j = _model().export_json()
    [l for l in j["layers"] if l["type"] == "denet-sparse"][0]["tapRule"] = bad
    with pytest.raises(ValueError, match="tapRule"):
        model_cnn.load_from_json(j, 2)


def test_model_modify_sets_the_rule_and_takes_it_back():
    model = _model()
    default_json = _dns_json(model)
    on = modify.modify_layer(model, "denet-sparse", ["tap_rule=2"])
    assert _dns(on).tap_rule == 2 and _dns_json(on)["tapRule"] == 2
    off = modify.modify_layer(on, "denet-sparse", ["tap_rule=0"])
    assert _dns(off).tap_rule == 0 and _dns_json(off) == default_json
    with pytest.raises(ValueError, match="tapRule"):
        modify.modify_layer(off, "denet-sparse", ["tap_rule=3"])


def test_cabi_declares_and_binds_the_four_entries():
    """include/denet_hip.h and lib.SIGNATURES agree argument by argument, the library exports the symbols, every declaration says that
    the reference has no counterpart and names section 16, and ops carries the three host functions and the two launch names"""
    L = dlib.load()
    for name in NAMES:
        text, restype, declared = cabi.declaration(name)
        assert "no counterpart" in text and "section 16" in text, name
        res, args = dlib.SIGNATURES[name]
        assert res is restype, name
        assert declared == list(args), (name, declared, args)
        assert hasattr(L, name), name
    for fn in ("sparse_bilinear_fwd", "sparse_bilinear_sort_async", "sparse_bilinear_bwd"):
        assert callable(getattr(ops, fn)), fn
    assert ops.kernel_symbol(60, 0, 0, 0) == "sparse_bilinear_fwd_kernel"
    assert ops.kernel_symbol(61, 0, 0, 0) == "sparse_bilinear_bwd_kernel"
    from denet_amd import build
    assert "sparse_bilinear.hip" in build.SOURCES and "sparse_bilinear.hip" in build.NO_CONTRACT


def test_entry_points_refuse_before_any_device_work():
    """called with null pointers on a CPU-only box: each limit answers with its own message"""
    L = dlib.load()

    def bwd(B=1, H=8, W=8, CP=32, coff=4, F=8, rois=4, gs=3, KP=96, zero_from=None):
        return L.denet_sparse_bilinear_bwd(None, None, None, None, 0, None, B, H, W, CP, coff, F, rois, gs, KP,
                                           coff + F if zero_from is None else zero_from, None)

    assert bwd(F=6, KP=64) == -1000
    err = L.denet_last_error()
    assert b"sparse_bilinear_bwd" in err and b"F (6)" in err and b"multiple of 4" in err
    assert bwd(F=260, CP=288, KP=2368) == -1000
    err = L.denet_last_error()
    assert b"sparse_bilinear_bwd" in err and b"F (260)" in err and b"256" in err
    assert bwd(CP=34) == -1000
    assert b"CP (34)" in L.denet_last_error()
    assert bwd(H=256, W=129) == -1000
    err = L.denet_last_error()
    assert b"sparse_bilinear_bwd" in err and b"256 x 129" in err and b"32768" in err
    assert bwd(zero_from=40) == -1000
    assert b"zero_from" in L.denet_last_error()
    assert bwd() == -1000
    assert b"null" in L.denet_last_error()
    # the grouping: the same cell limit, and no workspace for a refused geometry
    assert L.denet_sparse_bilinear_sort(None, None, 0, 1, 256, 129, 4, 3, None) == -1000
    err = L.denet_last_error()
    assert b"sparse_bilinear_sort" in err and b"32768" in err
    assert L.denet_sparse_bilinear_sort(None, None, 0, 1, 8, 8, 4, 3, None) == -1000
    assert b"null" in L.denet_last_error()
    assert L.denet_sparse_bilinear_workspace_bytes(1, 256, 129, 4, 3) == 0
    # ... which is the nearest rules' workspace for four times the slots
    assert L.denet_sparse_bilinear_workspace_bytes(2, 8, 8, 4, 3) == L.denet_sparse_sort_workspace_bytes(2, 8, 8, 16, 3) > 0
    assert L.denet_sparse_bilinear_workspace_bytes(2, 8, 8, 4, 3) > L.denet_sparse_sort_workspace_bytes(2, 8, 8, 4, 3)
    # the gather: a layout it cannot serve, a missing pointer, one of the two training arrays without the other
    assert L.denet_sparse_bilinear_fwd(None, None, None, None, None, 1, 8, 8, 32, 28, 8, 4, 3, 96, None) == -1000
    assert b"channel layout" in L.denet_last_error()
    assert L.denet_sparse_bilinear_fwd(None, None, None, None, None, 1, 8, 8, 32, 4, 8, 4, 1, 96, None) == -1000
    assert b"grid size 1" in L.denet_last_error()
    assert L.denet_sparse_bilinear_fwd(None, None, None, None, None, 1, 8, 8, 32, 4, 8, 4, 3, 96, None) == -1000
    assert b"null" in L.denet_last_error()
    one = 1
    assert L.denet_sparse_bilinear_fwd(one, one, one, one, None, 1, 8, 8, 32, 4, 8, 4, 3, 96, None) == -1000
    assert b"together" in L.denet_last_error()
    # the nearest rules' entry keeps its own rules: rule 2 is not one of them
    assert L.denet_sparse_fwd(one, one, one, None, 1, 8, 8, 32, 4, 8, 4, 3, 96, 2, None) == -1000
    assert b"tap_rule" in L.denet_last_error()
