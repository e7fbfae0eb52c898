"""Batch renormalisation, host side (no device work): the `BN[m, eps, r, d, it]` grammar and the JSON keys renormMaxR / renormMaxD /
renormMaxIt of `batchnorm`, `batchnorm-relu` and the bnParam of `resnet` layers, the ramp of the limits over the epochs (the
reference's commented-out block, denet/layer/batch_norm.py:65-73), the refusals, and `model-modify --modify-bn-renorm R D IT`."""
import math

import numpy as np
import pytest

from denet_amd.layer import batch_norm
from denet_amd.model import model_cnn, modify

KEYS = ("renormMaxR", "renormMaxD", "renormMaxIt")
DESC = "C.B[32,3] BN A C[32,3] BNA nRSN.O[2,32,3] P.A[8] R"


def _build(desc=DESC, seed=3):
    np.random.seed(seed)
    m = model_cnn.ModelCNN()
    m.batch_size = 2
    m.class_num = 10
    m.build(desc, (3, 8, 8), "relu", "half", ["he-backward"])
    return m


def _plain(j):
    """an exported model with arrays and tuples as lists, without the wall-clock `date` export_json() stamps: comparable with =="""
    if isinstance(j, dict):
        return {k: _plain(v) for k, v in j.items() if k != "date"}
    if isinstance(j, (list, tuple)):
        return [_plain(v) for v in j]
    if isinstance(j, np.ndarray):
        return j.tolist()
    if isinstance(j, np.generic):
        return j.item()
    return j


def _bns(model):
    return [l for l in model_cnn.walk_layers(model.layers) if isinstance(l, batch_norm.BatchNormLayer)]


def test_desc_parsing():
    m = _build("C.B[32,3] BN[0.9,1e-5,3,5,10] A BN P.A[8] R")
    bn, plain = m.layers[2], m.layers[4]
    assert bn.type_name == "batchnorm" and (bn.momentum, bn.eps) == (0.9, 1e-5)
    assert (bn.renorm_max_r, bn.renorm_max_d, bn.renorm_max_it) == (3, 5, 10) and bn.renorm_active
    assert (plain.renorm_max_r, plain.renorm_max_d, plain.renorm_max_it) == (1, 0, 0) and not plain.renorm_active
    # either limit alone switches it on (batch_norm.py:66)
    assert _build("C.B[32,3] BN[0.9,1e-5,2] P.A[8] R").layers[2].renorm_active
    assert _build("C.B[32,3] BN[0.9,1e-5,1,0.5] P.A[8] R").layers[2].renorm_active
    # a renorm-active layer takes part in no fusion
    assert bn.stats_final(bn.input) is None and bn.sums_request(bn.output) is None


def test_json_round_trip_batchnorm():
    m = _build("C.B[32,3] BN[0.9,1e-5,3,5,10] A P.A[8] R")
    j = m.export_json()
    assert [j["layers"][1][k] for k in KEYS] == [3, 5, 10]
    m2 = model_cnn.load_from_json(j, 2)
    bn = m2.layers[2]
    assert (bn.renorm_max_r, bn.renorm_max_d, bn.renorm_max_it) == (3, 5, 10) and bn.renorm_active
    assert _plain(m2.export_json()) == _plain(j)


def test_json_round_trip_batchnorm_relu():
    m = _build()
    j = m.export_json()
    bna = [l for l in j["layers"] if l["type"] == "batchnorm-relu"]
    assert len(bna) == 1 and not any(k in bna[0] for k in KEYS)          # inactive: the fused layer's export has no such keys
    bna[0].update({"renormMaxR": 3.0, "renormMaxD": 5.0, "renormMaxIt": 10})
    m2 = model_cnn.load_from_json(j, 2)
    layer = [l for l in m2.layers if l.type_name == "batchnorm-relu"][0]
    assert (layer.renorm_max_r, layer.renorm_max_d, layer.renorm_max_it) == (3.0, 5.0, 10) and layer.renorm_active
    j2 = m2.export_json()
    out = [l for l in j2["layers"] if l["type"] == "batchnorm-relu"][0]
    assert [out[k] for k in KEYS] == [3.0, 5.0, 10]
    assert _plain(j2) == _plain(j)
    # --convert-bn-relu keeps an active layer active, and writes no key for an inactive one
    act = modify.convert_bn_relu(_build("C.B[32,3] BN[0.9,1e-5,3,5,10] A C[32,3] BN A P.A[8] R"))
    fused = [l for l in act.layers if l.type_name == "batchnorm-relu"]
    assert [l.renorm_active for l in fused] == [True, False]
    assert [[k in l.export_json() for k in KEYS] for l in fused] == [[True] * 3, [False] * 3]


def test_json_round_trip_resnet():
    m = _build()
    j = m.export_json()
    blocks = [l for l in j["layers"] if l["type"] == "resnet"]
    assert len(blocks) == 2 and all(b["bnParam"] == {"enabled": True} for b in blocks)
    blocks[0]["bnParam"] = dict(blocks[0]["bnParam"], renormMaxR=3.0, renormMaxD=5.0, renormMaxIt=10)
    m2 = model_cnn.load_from_json(j, 2)
    r0, r1 = [l for l in m2.layers if l.type_name == "resnet"]
    inner0 = [l for l in r0.layers if isinstance(l, batch_norm.BatchNormLayer)]
    inner1 = [l for l in r1.layers if isinstance(l, batch_norm.BatchNormLayer)]
    assert len(inner0) == 2 and all(l.renorm_active and (l.renorm_max_r, l.renorm_max_d, l.renorm_max_it) == (3.0, 5.0, 10)
                                    for l in inner0)
    assert len(inner1) == 2 and not any(l.renorm_active for l in inner1)
    j2 = m2.export_json()
    assert j2["layers"][[l["type"] for l in j2["layers"]].index("resnet")]["bnParam"] == blocks[0]["bnParam"]
    assert _plain(model_cnn.load_from_json(j2, 2).export_json()) == _plain(j2)
    # the fused blocks of the DeNet / ResNet models (`bnrelu`): the keys reach their batchnorm-relu sub-layers
    m3 = modify.convert_bn_relu(m2)
    r0 = [l for l in m3.layers if l.type_name == "resnet"][0]
    assert "bnrelu" in r0.version
    subs = [l for l in r0.layers if isinstance(l, batch_norm.BatchNormLayer)]
    assert [l.type_name for l in subs] == ["batchnorm-relu", "batchnorm"] and all(l.renorm_active for l in subs)
    assert all(k in subs[0].export_json() for k in KEYS)


def _formula(R, D, it, epoch):
    """the issue's definition, restated"""
    if it > 0:
        return min(R, math.exp(epoch * math.log(R) / it)), min(D, math.exp(epoch * math.log(D + 1) / it) - 1)
    return R, D


@pytest.mark.parametrize("R,D,it", [(3.0, 5.0, 10), (2.0, 0.0, 4), (1.0, 0.5, 6), (3.0, 5.0, 0)])
def test_ramp(R, D, it):
    for epoch in (0, it / 2, it, 2 * it, 1, 7):
        r_max, d_max = batch_norm.renorm_limits(R, D, it, epoch)
        fr, fd = _formula(R, D, it, epoch)
        assert r_max == pytest.approx(fr, rel=1e-12, abs=1e-15) and d_max == pytest.approx(fd, rel=1e-12, abs=1e-15)
        assert 1.0 <= r_max <= R and 0.0 <= d_max <= D
    if it > 0:
        assert batch_norm.renorm_limits(R, D, it, 0) == (1.0, 0.0)          # closed: plain batch norm
        assert batch_norm.renorm_limits(R, D, it, it) == pytest.approx((R, D), rel=1e-12)
        assert batch_norm.renorm_limits(R, D, it, 2 * it) == (R, D)
        r_half, d_half = batch_norm.renorm_limits(R, D, it, it / 2)
        assert r_half == pytest.approx(math.sqrt(R), rel=1e-12) and d_half == pytest.approx(math.sqrt(D + 1) - 1, rel=1e-12, abs=1e-15)
    else:
        assert all(batch_norm.renorm_limits(R, D, it, e) == (R, D) for e in (0, 1, 50))      # `it` = 0: no ramp, no division


@pytest.mark.parametrize("args,word", [
    ((0.5, 0.0, 0), "renormMaxR must be >= 1"),
    ((3.0, -1.0, 0), "renormMaxD must be >= 0"),
    ((3.0, 5.0, -2), "renormMaxIt must be >= 0"),
    ((float("nan"), 0.0, 0), "renormMaxR must be a finite number"),
    ((3.0, float("inf"), 0), "renormMaxD must be a finite number"),
    ((3.0, 5.0, float("nan")), "renormMaxIt must be a finite number"),
])
def test_refusals(args, word):
    with pytest.raises(ValueError, match=word):
        batch_norm.renorm_check(*args)
    if all(math.isfinite(a) for a in args):
        with pytest.raises(ValueError, match=word):          # when the layer is built from the grammar
            _build("C.B[32,3] BN[0.9,1e-5,%r,%r,%r] P.A[8] R" % args)
    # the same through JSON, for both layer kinds and a block's bnParam
    j = _build().export_json()
    upd = dict(zip(KEYS, args))
    for pick in ("batchnorm", "batchnorm-relu", "resnet"):
        jj = _plain(j)
        l = [x for x in jj["layers"] if x["type"] == pick][0]
        (l["bnParam"] if pick == "resnet" else l).update(upd)
        with pytest.raises(ValueError, match=word):
            model_cnn.load_from_json(jj, 2)
    with pytest.raises(ValueError, match=word):
        modify.modify_bn_renorm(_build(), *args)


def test_modify_bn_renorm_traversal(tmp_path):
    m = _build()
    before = _plain(m.export_json())
    on = modify.modify_bn_renorm(m, 3, 5, 10)
    bns = _bns(on)
    assert len(bns) == 2 + 2 * 2 and {l.type_name for l in bns} == {"batchnorm", "batchnorm-relu"}
    assert all(l.renorm_active and (l.renorm_max_r, l.renorm_max_d, l.renorm_max_it) == (3.0, 5.0, 10) for l in bns)
    j = on.export_json()
    for l in j["layers"]:
        if l["type"] in ("batchnorm", "batchnorm-relu"):
            assert [l[k] for k in KEYS] == [3.0, 5.0, 10]
        if l["type"] == "resnet":
            assert [l["bnParam"][k] for k in KEYS] == [3.0, 5.0, 10] and l["bnParam"]["enabled"] is True
    # nothing but the keys moved
    for a, b in zip(model_cnn.walk_layers(m.layers), model_cnn.walk_layers(on.layers)):
        assert a.type_name == b.type_name
        for pa, pb in zip(a.params(), b.params()):
            np.testing.assert_array_equal(pa.value, pb.value)
    # the fused blocks too
    fused = modify.modify_bn_renorm(modify.convert_bn_relu(m), 3, 5, 0)
    assert all(l.renorm_active and l.renorm_max_it == 0 for l in _bns(fused))
    assert sum(l.type_name == "batchnorm-relu" for l in _bns(fused)) == 4
    # 1 0 0 switches it off: the export is the original's
    off = modify.modify_bn_renorm(on, 1, 0, 0)
    assert not any(l.renorm_active for l in _bns(off))
    assert _plain(off.export_json()) == before
    # a top-level batchnorm always exports the keys: switched off it carries the values as given (renormMaxIt 0), also where a
    # file carried the constructor's 10 - the one place where `1 0 0` does not give the original back (stated in the help)
    j10 = _plain(m.export_json())
    j10["layers"][1]["renormMaxIt"] = 10
    off10 = modify.modify_bn_renorm(model_cnn.load_from_json(j10, 2), 1, 0, 0)
    assert [off10.export_json()["layers"][1][k] for k in KEYS] == [1.0, 0.0, 0] and not off10.layers[2].renorm_active
    assert "renormMaxIt 0" in " ".join(modify.build_parser().format_help().split())
    # --modify-bn keeps its meaning and the renorm keys
    kept = modify.modify_bn(on, 1, 0.8, 1e-4)
    assert all(l.renorm_active and l.momentum == 0.8 for l in _bns(kept) if l.type_name == "batchnorm")
    # the command line
    src, dst, back = (str(tmp_path / n) for n in ("a.mdl.gz", "b.mdl.gz", "c.mdl.gz"))
    model_cnn.save_to_file(m, src)
    assert modify.main(["--input", src, "--output", dst, "--modify-bn-renorm", "3", "5", "10"]) == 0
    assert _plain(model_cnn.load_from_file(dst, 2).export_json()) == _plain(j)
    assert modify.main(["--input", dst, "--output", back, "--modify-bn-renorm", "1", "0", "0"]) == 0
    assert _plain(model_cnn.load_from_file(back, 2).export_json()) == before
    assert "--modify-bn-renorm" in modify.build_parser().format_help()
    with pytest.raises(ValueError, match="renormMaxR must be >= 1"):
        modify.main(["--input", src, "--output", dst, "--modify-bn-renorm", "0.5", "0", "0"])


def test_default_model_export_is_unchanged():
    """the keys a default model writes are those it wrote before the feature existed: `batchnorm` carries the three keys with the
    grammar's defaults (as the reference's export does), `batchnorm-relu` and bnParam carry none"""
    m = _build()
    j = m.export_json()
    bn = j["layers"][1]
    assert set(bn.keys()) == {"type", "layers", "momentum", "eps", "mean", "std", "gamma", "bias", "renormMaxR", "renormMaxD",
                              "renormMaxIt", "enabled"}
    assert [bn[k] for k in KEYS] == [1, 0, 0]
    bna = [l for l in j["layers"] if l["type"] == "batchnorm-relu"][0]
    assert set(bna.keys()) == {"type", "layers", "momentum", "eps", "mean", "std", "gamma", "bias"}
    for blk in (l for l in j["layers"] if l["type"] == "resnet"):
        assert blk["bnParam"] == {"enabled": True}
        inner = [s for s in blk["layers"] if s["type"] == "batchnorm"]
        assert inner and all([s[k] for k in KEYS] == [1.0, 0.0, 10] for s in inner)
    # and a reload from that JSON, made before any renorm key was touched, exports the same again
    assert _plain(model_cnn.load_from_json(j, 2).export_json()) == _plain(j)
    assert batch_norm.renorm_log_line(m, 0) is None
    on = modify.modify_bn_renorm(m, 3, 5, 10)
    assert batch_norm.renorm_log_line(on, 0) == "batch renorm: 6 active layers, epoch 0 limits r_max=1 d_max=0"
    assert batch_norm.renorm_log_line(on, 5) == "batch renorm: 6 active layers, epoch 5 limits r_max=%.6g d_max=%.6g" % (
        math.sqrt(3.0), math.sqrt(6.0) - 1.0)
