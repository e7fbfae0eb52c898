"""Opt-in focal cost of the corner map and the detection head (focalGamma; csrc/focal.hip), the part that needs
no GPU: the float64 reference checked against central differences of its own costs, the desc grammar, the JSON key, model-modify,
the refusals and the C-ABI surface."""
import math

import numpy as np
import pytest

import cabi
import focal_reference as FR
from denet_amd import lib as dlib, ops
from denet_amd.model import model_cnn, modify

NAMES = ("denet_corner_loss_focal", "denet_detect_loss_focal")
GAMMAS = [1.0, 2.0, 3.5]


# ---- the reference against central differences of its own costs ----------------------------------------------------------------

def _corner_inputs():
    rng = np.random.RandomState(3)
    x = 3.0 * rng.randn(2, 4, 5, 6)
    x.reshape(-1)[:6] = [12.0, -12.0, 14.0, -14.0, 9.0, -9.0]            # saturated cells: one probability ~ 1e-11 ... 1e-12
    t0, t1 = rng.rand(*x.shape) / x.size, rng.rand(*x.shape) / x.size
    drop = rng.rand(*x.shape) < 0.25
    t0[drop] = t1[drop] = 0.0
    return x, t0, t1


def _detect_inputs():
    rng = np.random.RandomState(4)
    M, ncls = 10, 7
    z = rng.randn(M, ncls)
    t = np.zeros((M, ncls))
    cls = rng.randint(0, ncls, M)
    t[np.arange(M), cls] = 1.0
    t[::5, 3] = 1.0
    t = t / t.sum(1, keepdims=True) / 5.0
    z[1, cls[1]] += 28.0                                                   # the target is certain: q ~ 1e-12
    z[2, (cls[2] + 1) % ncls] += 28.0                                      # another class is certain: p ~ 1e-12
    return z, t


def _central(f, x, h=1e-5):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = f(x)
        flat[i] = keep - h
        dn = f(x)
        flat[i] = keep
        gf[i] = (up - dn) / (2 * h)
    return g


@pytest.mark.parametrize("gamma", GAMMAS)
def test_reference_corner_gradient_is_the_derivative_of_its_cost(gamma):
    x, t0, t1 = _corner_inputs()
    cost = lambda v: FR.corner_focal(*FR.corner_logpr(v), t0, t1, gamma, 100.0, 2)[0]
    _, grad = FR.corner_focal(*FR.corner_logpr(x), t0, t1, gamma, 100.0, 2)
    num = _central(cost, x.copy())
    err = np.abs(num - grad).max() / np.abs(grad).max()
    print("focal reference, corner, gamma %g: central differences differ by %.2e of the largest gradient" % (gamma, err))
    assert err < 1e-7, err
    assert not grad[(t0 == 0) & (t1 == 0)].any()


@pytest.mark.parametrize("gamma", GAMMAS)
def test_reference_detect_gradient_is_the_derivative_of_its_cost(gamma):
    z, t = _detect_inputs()
    cost = lambda v: FR.detect_focal(v, t, gamma, 1.5, 2)[0]
    _, grad = FR.detect_focal(z, t, gamma, 1.5, 2)
    num = _central(cost, z.copy())
    err = np.abs(num - grad).max() / np.abs(grad).max()
    print("focal reference, detect, gamma %g: central differences differ by %.2e of the largest gradient" % (gamma, err))
    assert err < 1e-7, err


def test_reference_at_gamma_0_is_the_plain_cost():
    x, t0, t1 = _corner_inputs()
    l0, l1 = FR.corner_logpr(x)
    c, g = FR.corner_focal(l0, l1, t0, t1, 0.0, 100.0, 2)
    cp, gp = FR.corner_plain(l0, l1, t0, t1, 100.0, 2)
    assert abs(c - cp) <= 1e-14 * abs(cp) and np.abs(g - gp).max() <= 1e-14 * np.abs(gp).max()
    z, t = _detect_inputs()
    c, g = FR.detect_focal(z, t, 0.0, 1.5, 2)
    cp, gp = FR.detect_plain(z, t, 1.5, 2)
    assert abs(c - cp) <= 1e-14 * abs(cp) and np.abs(g - gp).max() <= 1e-14 * np.abs(gp).max()


def test_reference_softmax_keeps_the_small_side():
    """class_logpr: q of a certain row is the others' mass, not 1 - p rounded"""
    z = np.zeros((1, 5))
    z[0, 2] = 30.0
    lp, p, q = FR.class_logpr(z)
    assert abs(q[0, 2] / (4 * math.exp(-30.0)) - 1) < 1e-12 and abs(lp[0, 2] / -q[0, 2] - 1) < 1e-12
    assert abs(lp[0, 0] + 30.0) < 1e-12 and abs(q[0, 0] - 1.0) < 1e-12


# ---- grammar, JSON, model-modify ----------------------------------------------------------------------------------------------

def _model(dnc="DNC[8,10]", dnd="DND[0.5,1,1]"):
    np.random.seed(0)
    model = model_cnn.ModelCNN()
    model.batch_size, model.class_num = 2, 3
    model.build("C[32,3] %s DNS[3,4,0.01,0.1] C[32,1] %s" % (dnc, dnd), (3, 16, 16), "relu", "half", ["he-backward"])
    return model


def _layer(model, type_name):
    return [l for l in model.layers if l.type_name == type_name][0]


def _json(model, type_name):
    """the layer's own keys (its nested convolution, with the weight arrays, left out)"""
    j = [l for l in model.export_json()["layers"] if l["type"] == type_name][0]
    return {k: v for k, v in j.items() if k not in ("layers", "conv")}


def test_desc_parameters_set_gamma():
    model = _model("DNC[96,100,0,2]", "DND[0.5,1,1,0,2]")
    dnc, dnd = _layer(model, "denet-corner"), _layer(model, "denet-detect")
    assert dnc.focal_gamma == 2.0 and type(dnc.focal_gamma) is float
    assert dnd.focal_gamma == 2.0 and type(dnd.focal_gamma) is float
    assert (dnc.sample_feat, dnc.cost_factor, dnc.dropout) == (96, 100, 0)
    assert (dnd.overlap_threshold, dnd.cost_factor, dnd.bbox_factor, dnd.indfit_factor) == (0.5, 1, 1, 0)
    assert _json(model, "denet-corner")["focalGamma"] == 2.0 and _json(model, "denet-detect")["focalGamma"] == 2.0
    frac = _model("DNC.C[96,100,0.1,3.5]", "DND.B[0.5,1,1,0,1]")
    assert _layer(frac, "denet-corner").focal_gamma == 3.5 and _layer(frac, "denet-corner").use_center
    assert _layer(frac, "denet-detect").focal_gamma == 1.0 and _layer(frac, "denet-detect").use_bounded_iou


def test_default_layers_have_gamma_0_and_export_no_key():
    model = _model("DNC[96,100]", "DND[0.5,1,1]")
    for type_name, keys in (("denet-corner", {"sampleFeat", "useCenter", "costFactor", "dropout"}),
                            ("denet-detect", {"costFactor", "bboxFactor", "fitnessFactor", "useJointFitness", "useBoundedIoU",
                                              "classNum", "overlapThreshold"})):
        layer = _layer(model, type_name)
        assert layer.focal_gamma == 0.0 and type(layer.focal_gamma) is float
        j = _json(model, type_name)
        assert "focalGamma" not in j and keys <= set(j)
    assert _json(_model("DNC[96,100,0,0]"), "denet-corner") == _json(model, "denet-corner")      # an explicit 0 is the default


def test_json_key_survives_export_and_reload():
    j = _model().export_json()
    [l for l in j["layers"] if l["type"] == "denet-corner"][0]["focalGamma"] = 2
    [l for l in j["layers"] if l["type"] == "denet-detect"][0]["focalGamma"] = 3.5
    loaded = model_cnn.load_from_json(j, 2)
    assert _layer(loaded, "denet-corner").focal_gamma == 2.0 and _layer(loaded, "denet-detect").focal_gamma == 3.5
    again = model_cnn.load_from_json(loaded.export_json(), 2)
    assert _json(again, "denet-corner")["focalGamma"] == 2.0 and _json(again, "denet-detect")["focalGamma"] == 3.5
    assert _layer(again, "denet-corner").focal_gamma == 2.0 and _layer(again, "denet-detect").focal_gamma == 3.5


@pytest.mark.parametrize("type_name", ["denet-corner", "denet-detect"])
def test_model_modify_sets_gamma_and_takes_it_back(type_name):
    model = _model()
    default_json = _json(model, type_name)
    on = modify.modify_layer(model, type_name, ["focal_gamma=2"])
    assert _layer(on, type_name).focal_gamma == 2.0 and _json(on, type_name)["focalGamma"] == 2.0
    other = "denet-detect" if type_name == "denet-corner" else "denet-corner"
    assert _layer(on, other).focal_gamma == 0.0
    off = modify.modify_layer(on, type_name, ["focal_gamma=0"])
    assert _layer(off, type_name).focal_gamma == 0.0 and _json(off, type_name) == default_json
    with pytest.raises(ValueError, match="focalGamma"):
        modify.modify_layer(off, type_name, ["focal_gamma=0.5"])


@pytest.mark.parametrize("bad", [-1, 0.5, float("nan"), float("inf"), "2", True])
@pytest.mark.parametrize("type_name", ["denet-corner", "denet-detect"])
def test_bad_gamma_is_refused_when_the_layer_is_built(type_name, bad):
    j = _model().export_json()
    [l for l in j["layers"] if l["type"] == type_name][0]["focalGamma"] = bad
    with pytest.raises(ValueError, match="%s: focalGamma must be 0" % type_name):
        model_cnn.load_from_json(j, 2)


@pytest.mark.parametrize("desc", [("DNC[8,10,0,-1]", "DND[0.5,1,1]"), ("DNC[8,10,0,0.5]", "DND[0.5,1,1]"),
                                  ("DNC[8,10]", "DND[0.5,1,1,0,-1]"), ("DNC[8,10]", "DND[0.5,1,1,0,0.5]")])
def test_bad_gamma_in_a_desc_is_refused(desc):
    with pytest.raises(ValueError, match="focalGamma"):
        _model(*desc)


def test_drivers_log_gamma_per_cost_layer():
    from denet_amd.layer import focal_log_lines
    assert focal_log_lines(_model()) == []
    lines = focal_log_lines(_model("DNC[8,10,0,2]", "DND[0.5,1,1,0,3.5]"))
    assert len(lines) == 2
    assert "denet-corner" in lines[0] and "focal gamma 2" in lines[0]
    assert "denet-detect" in lines[1] and "focal gamma 3.5" in lines[1]
    assert len(focal_log_lines(_model("DNC[8,10]", "DND[0.5,1,1,0,2]"))) == 1


# ---- C ABI --------------------------------------------------------------------------------------------------------------------

def test_cabi_declares_and_binds_the_two_entries():
    """include/denet_hip.h and lib.SIGNATURES agree argument by argument, the library exports the symbols, each declaration names
    the reference lines it extends, says that the reference has no such mode and names section 17"""
    L = dlib.load()
    extends = {"denet_corner_loss_focal": "denet_corner.py:126-134", "denet_detect_loss_focal": "denet_detect.py:238-313"}
    for name in NAMES:
        text, restype, declared = cabi.declaration(name)
        assert "no such mode" in text and "section 17" in text and extends[name] in text, name
        res, args = dlib.SIGNATURES[name]
        assert res is restype, name
        assert declared == list(args), (name, declared, args)
        assert hasattr(L, name), name
        # the arguments of the plain entry plus `float gamma` in front of the stream
        plain = dlib.SIGNATURES[name[:-len("_focal")]][1]
        assert list(args) == list(plain[:-1]) + [dlib.F, dlib.P], name
    assert callable(ops.corner_loss_focal) and callable(ops.detect_loss_focal)
    assert ops.kernel_symbol(70, 0, 0, 0) == "corner_focal_loss_kernel"
    assert ops.kernel_symbol(71, 0, 0, 0) == "detect_focal_loss_kernel"
    from denet_amd import build
    assert "focal.hip" in build.SOURCES and "focal.hip" in build.NO_CONTRACT


def test_entry_points_refuse_before_any_device_work():
    """called without a device: a gamma outside the domain and null pointers answer with their own messages"""
    L = dlib.load()
    one = 1

    def corner(gamma, p=one, B=2, Cn=4):
        return L.denet_corner_loss_focal(p, p, p, p, p, B, 8, 8, 32, Cn, 100.0, gamma, None)

    def detect(gamma, p=one, nreg=0, ncls=21, CP=32, valid=None):
        return L.denet_detect_loss_focal(p, p, valid, valid, None, None, p, p, p, 18, 2, CP, ncls, nreg, 0, 1.0, 1.0, 0.0, 0,
                                         gamma, None)

    for call, who in ((corner, b"corner_loss_focal"), (detect, b"detect_loss_focal")):
        for bad in (-1.0, 0.5, float("nan"), float("inf"), -0.25, 0.999):
            assert call(bad) == -1000, (who, bad)
            err = L.denet_last_error()
            assert who in err and b"gamma" in err, err
        assert call(2.0, p=None) == -1000
        err = L.denet_last_error()
        assert who in err and b"null" in err, err
        assert call(0.0, p=None) == -1000                                      # gamma 0 is inside the domain: the pointers are next
        assert b"null" in L.denet_last_error()
    assert corner(2.0, Cn=0) == -1000 and b"bad shape" in L.denet_last_error()
    assert corner(2.0, Cn=40) == -1000 and b"bad shape" in L.denet_last_error()
    assert detect(2.0, nreg=3) == -1000 and b"nreg" in L.denet_last_error()
    assert detect(2.0, nreg=4) == -1000 and b"bbox targets missing" in L.denet_last_error()
    assert detect(2.0, ncls=40) == -1000 and b"CP too small" in L.denet_last_error()
