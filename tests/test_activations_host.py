"""The sigmoid / tanh / elu / softplus activations, host side: construction, the desc grammar, the JSON round trip, model surgery
and the names that are refused (no device needed)."""
import copy

import numpy as np
import pytest

from denet_amd.layer import Act, InitialLayer
from denet_amd.layer.activation import ActivationLayer
from denet_amd.layer.batch_norm import BatchNormLayer
from denet_amd.layer.resnet import ResnetLayer
from denet_amd.model import model_cnn, modify

SMOOTH = ["sigmoid", "tanh", "elu", "softplus"]
DESC = "C.B[32,3] BN A P[2] nRSN.O[2,64,3,2] nRSN[2,64,3,1] nRSN.O[2,128,3,2,32] nRSN[2,128,3,1,32] R.C"


def _initial(shape=(2, 32, 8, 8)):
    return [InitialLayer(Act(shape), shape)]


def _model(activation, desc=DESC, batch=2, size=16, class_num=5, seed=3):
    np.random.seed(seed)
    m = model_cnn.ModelCNN()
    m.batch_size = batch
    m.class_num = class_num
    m.build(desc, (3, size, size), activation, "half", ["he-backward"])
    return m


def _strip(j, drop=("activation", "date", "user")):
    """a model's JSON without the activation names (and the time stamp), arrays as lists"""
    if isinstance(j, dict):
        return {k: _strip(v, drop) for k, v in j.items() if k not in drop}
    if isinstance(j, (list, tuple)):
        return [_strip(v, drop) for v in j]
    if isinstance(j, np.ndarray):
        return j.tolist()
    return j


def _activation_names(j):
    """every `activation` value of the activation / resnet layers of a model's JSON, nested sub-layers included"""
    out = []
    for l in j["layers"] if isinstance(j, dict) and "classNum" in j else j:
        if l["type"] in ("activation", "resnet"):
            out.append(l["activation"])
        out += _activation_names(l.get("layers", []))
    return out


@pytest.mark.parametrize("name", SMOOTH)
def test_layers_construct(name):
    a = ActivationLayer(_initial(), name)
    assert a.activation == name and a.output is not a.input and a.output.cp == a.input.cp
    assert a.export_json()["activation"] == name
    for version in ("original", "pre-activation"):
        for bottleneck in (0, 32):
            for stride in (1, 2):
                r = ResnetLayer(_initial(), (64, 32, 3, 3), (stride, stride), bottleneck, name, version)
                assert r.activation == name and r.export_json()["activation"] == name
                acts = [l for l in r.layers if l.type_name == "activation"]
                assert acts and all(l.activation == name and l.fused_into is None for l in acts)
                assert not any(l.type_name == "batchnorm-relu" for l in r.layers)
                assert r._fold_plan() is None                      # inference takes the unfolded path
                assert r.output_shape == (2, 64, 8 // stride, 8 // stride)


def test_fused_into_only_for_relu():
    for name, fused in (("sigmoid", False), ("relu", True), ("relu-safe", True), ("tanh", False)):
        ls = _initial()
        ls.append(BatchNormLayer(ls))
        a = ActivationLayer(ls, name)
        assert (a.fused_into is ls[-1]) == fused, name
        assert (getattr(ls[-1], "act_behind", None) is a) == fused, name


def test_parse_desc_same_layers_as_relu():
    relu, tanh = _model("relu"), _model("tanh")
    assert [l.type_name for l in relu.layers] == [l.type_name for l in tanh.layers]
    for a, b in zip(model_cnn.walk_layers(relu.layers), model_cnn.walk_layers(tanh.layers)):
        assert a.type_name == b.type_name and a.output_shape == b.output_shape
    jr, jt = relu.export_json(), tanh.export_json()
    assert _strip(jr) == _strip(jt)                                # same keys, shapes and (same seed) initial values
    assert set(_activation_names(jr)) == {"relu"} and set(_activation_names(jt)) == {"tanh"}
    assert len(_activation_names(jt)) == len(_activation_names(jr)) > 8
    # the top-level `A` token and the block exits
    assert [l.activation for l in tanh.layers if l.type_name in ("activation", "resnet")] == ["tanh"] * 9


@pytest.mark.parametrize("name", SMOOTH)
def test_json_round_trip(name):
    m = _model(name)
    for l in model_cnn.walk_layers(m.layers):                      # distinguishable batch-norm state
        if l.type_name == "batchnorm" and l.enabled:
            l.mean.set_value(np.random.normal(size=l.mean.value.shape))
            l.stdinv.set_value(np.random.uniform(0.5, 2.0, size=l.stdinv.value.shape))
    j = m.export_json()
    m2 = model_cnn.load_from_json(copy.deepcopy(j), 2)
    j2 = m2.export_json()
    assert _strip(j, ("date", "user")) == _strip(j2, ("date", "user"))
    assert set(_activation_names(j2)) == {name}


@pytest.mark.parametrize("name", SMOOTH + ["relu-safe", "none"])
def test_set_activation_then_load(name, tmp_path):
    m = _model("relu")
    m2 = modify.set_activation(m, name)
    j = m2.export_json()
    assert set(_activation_names(j)) == {name}
    assert _strip(j) == _strip(m.export_json())                    # nothing else moved: parameters, shapes, versions
    f = str(tmp_path / "m.mdl.gz")
    model_cnn.save_to_file(m2, f)
    m3 = model_cnn.load_from_file(f, 2)
    assert set(_activation_names(m3.export_json())) == {name}
    # and back
    assert set(_activation_names(modify.set_activation(m3, "relu").export_json())) == {"relu"}


def test_set_activation_cli(tmp_path):
    src, dst = str(tmp_path / "a.mdl.gz"), str(tmp_path / "b.mdl.gz")
    model_cnn.save_to_file(_model("relu"), src)
    assert modify.main(["--input", src, "--output", dst, "--activation", "softplus"]) == 0
    assert set(_activation_names(model_cnn.load_from_file(dst, 2).export_json())) == {"softplus"}


def test_set_activation_refuses_converted_blocks():
    m = modify.convert_bn_relu(_model("relu"))
    assert any("bnrelu" in l.version for l in m.layers if l.type_name == "resnet")
    for name in SMOOTH:
        with pytest.raises(ValueError) as e:
            modify.set_activation(m, name)
        assert name in str(e.value) and "convert-bn-relu" in str(e.value) and "bnrelu" in str(e.value)
    assert modify.set_activation(m, "relu") is m                   # nothing to change: the model as it is


@pytest.mark.parametrize("name", ["softmax", "leaky-relu", "bogus"])
def test_refused_names_fail_at_construction(name):
    with pytest.raises((NotImplementedError, ValueError)) as e:
        ActivationLayer(_initial(), name)
    assert name in str(e.value)
    with pytest.raises((NotImplementedError, ValueError)) as e:
        ActivationLayer(_initial(), "relu", json_param={"activation": name})
    assert name in str(e.value)
    for version in ("original", "pre-activation"):
        with pytest.raises((NotImplementedError, ValueError)) as e:
            ResnetLayer(_initial(), (32, 32, 3, 3), (1, 1), 0, name, version)
        assert name in str(e.value)
    with pytest.raises((NotImplementedError, ValueError)) as e:
        _model(name, "C[32,3] A")
    assert name in str(e.value)
    with pytest.raises((NotImplementedError, ValueError)) as e:
        modify.set_activation(_model("relu", "C[32,3] A"), name)
    assert name in str(e.value)
    if name == "softmax":
        assert "2-D" in str(e.value)                               # says why


def test_relu_models_build_as_before():
    """relu / relu-safe / none: the fused sub-layers, the fold plan and the JSON of a converted block are what they were"""
    m = modify.convert_bn_relu(_model("relu"))
    blocks = [l for l in m.layers if l.type_name == "resnet"]
    assert all(any(s.type_name == "batchnorm-relu" for s in b.layers) for b in blocks)
    assert all(b._fold_plan() is not None for b in blocks if "original" in b.version)
    assert all(not b._smooth_exit() for b in blocks)
    for name in ("relu-safe", "none"):
        assert all(not b._smooth_exit() for b in _model(name).layers if b.type_name == "resnet")
