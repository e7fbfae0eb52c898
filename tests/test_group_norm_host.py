"""Group normalisation, host side (no device work): the `BN.G[g, eps]` / `BNA.G[g, eps]` grammar, the JSON key normGroups of
`batchnorm`, `batchnorm-relu` and the bnParam of `resnet` layers, `model-modify --modify-bn-groups G`, the zoo argument, the
refusals, model-update-bn's layer selection, and the closed-form backward the kernels implement against autograd (DESIGN.md
section 21)."""
import numpy as np
import pytest
import torch

from denet_amd.layer import batch_norm
from denet_amd.model import model_cnn, modify, update_bn
from group_norm_reference import gn_closed_form, gn_ref64

DESC = "C.B[32,3] BN A C[32,3] BNA nRSN.O[2,32,3] P.A[8] R"
DESC_G = "C.B[32,3] BN.G[8] A C[32,3] BNA.G nRSN.O[2,32,3] P.A[8] R"


def _build(desc=DESC, seed=3):
    np.random.seed(seed)
    m = model_cnn.ModelCNN()
    m.batch_size = 2
    m.class_num = 10
    m.build(desc, (3, 8, 8), "relu", "half", ["he-backward"])
    return m


def _plain(j):
    """an exported model with arrays and tuples as lists, without the wall-clock `date`: comparable with =="""
    if isinstance(j, dict):
        return {k: _plain(v) for k, v in j.items() if k != "date"}
    if isinstance(j, (list, tuple)):
        return [_plain(v) for v in j]
    if isinstance(j, np.ndarray):
        return j.tolist()
    if isinstance(j, np.generic):
        return j.item()
    return j


def _keys(j):
    """the key structure of an exported model: every dict's key set, arrays and scalars dropped"""
    if isinstance(j, dict):
        return {k: _keys(v) for k, v in j.items()}
    if isinstance(j, (list, tuple)) and any(isinstance(v, dict) for v in j):
        return [_keys(v) for v in j]
    return None


def _bns(model):
    return [l for l in model_cnn.walk_layers(model.layers) if isinstance(l, batch_norm.BatchNormLayer)]


def test_desc_grammar_and_defaults():
    m = _build("C.B[32,3] BN.G[8,1e-4] A C[64,3] BNA.G BN.G BNA.G[16] BN[0.8] BNA P.A[8] R")
    bn, bna, bn_d, bna16, plain, plain_a = m.layers[2], m.layers[5], m.layers[6], m.layers[7], m.layers[8], m.layers[9]
    assert (bn.type_name, bn.norm_groups, bn.eps, bn.momentum) == ("batchnorm", 8, 1e-4, 0.9)
    assert (bna.type_name, bna.norm_groups, bna.eps) == ("batchnorm-relu", 32, 1e-5)
    assert (bn_d.norm_groups, bn_d.eps) == (32, 1e-5) and (bna16.norm_groups, bna16.fused_relu) == (16, True)
    assert all(isinstance(l.norm_groups, int) for l in (bn, bna, bn_d, bna16))
    # the untagged tokens mean what they always meant
    assert (plain.norm_groups, plain.momentum, plain.eps) == (0, 0.8, 1e-5) and (plain_a.norm_groups, plain_a.momentum) == (0, 0.9)
    assert not bn.renorm_active
    # a group-mode layer takes part in no batch-norm fusion: no statistics asked of the producer, nothing handed to it
    assert not getattr(bn.input, "want_stats", False) and getattr(bn.input, "stats_bn", None) is None
    assert bn.stats_final(bn.input) is None and bn.sums_request(bn.output) is None
    assert getattr(plain.input, "want_stats", False) and plain.input.stats_bn is plain
    # gamma / beta stay biases; mean / std stay parameters (layout, packing and EMA untouched)
    assert bn.biases() == [bn.omega, bn.beta] and bn.params() == [bn.omega, bn.beta, bn.mean, bn.stdinv]
    assert bn.updates() == [bn.mean, bn.stdinv] and bn.weights() == []
    assert batch_norm.group_norm_log_line(m) == "group norm: 4 layers, groups 8 16 32"
    assert batch_norm.group_norm_log_line(_build()) is None


def test_key_round_trip_and_default_export_unchanged():
    plain, grouped = _build(), _build(DESC_G)
    jp, jg = plain.export_json(), grouped.export_json()
    # a default model writes the keys it always wrote: no normGroups anywhere
    assert "normGroups" not in repr(_keys(jp))
    assert set(jp["layers"][1].keys()) == {"type", "layers", "momentum", "eps", "mean", "std", "gamma", "bias", "renormMaxR",
                                           "renormMaxD", "renormMaxIt", "enabled"}
    assert set(jp["layers"][4].keys()) == {"type", "layers", "momentum", "eps", "mean", "std", "gamma", "bias"}
    assert all(l["bnParam"] == {"enabled": True} for l in jp["layers"] if l["type"] == "resnet")
    # the grouped model: the same key sets plus normGroups on the two tagged layers, nowhere else
    kp, kg = _keys(jp), _keys(jg)
    assert jg["layers"][1]["normGroups"] == 8 and jg["layers"][4]["normGroups"] == 32
    for i in (1, 4):
        assert kg["layers"][i].pop("normGroups", 0) is None
    assert kg == kp
    # mean / std stay in the file
    assert np.asarray(jg["layers"][1]["mean"]).shape == (32,) and np.asarray(jg["layers"][1]["std"]).shape == (32,)
    m2 = model_cnn.load_from_json(jg, 2)
    assert [l.norm_groups for l in _bns(m2)] == [8, 32, 0, 0, 0, 0]
    assert _plain(m2.export_json()) == _plain(jg)
    # normGroups 0 in a file is batch norm, and is not written back
    j0 = _plain(jp)
    j0["layers"][1]["normGroups"] = 0
    m0 = model_cnn.load_from_json(j0, 2)
    assert m0.layers[2].norm_groups == 0 and "normGroups" not in m0.export_json()["layers"][1]
    # --convert-bn-relu carries the key over
    fused = modify.convert_bn_relu(grouped)
    f = [l for l in fused.layers if l.type_name == "batchnorm-relu"]
    assert [l.norm_groups for l in f] == [8, 32] and f[0].export_json()["normGroups"] == 8


def test_bn_param_reaches_every_norm_of_a_block():
    j = _plain(_build("C.B[32,3] BN A RSN.O[64,3,2] RSN[64,3] P.A[4] R").export_json())
    blocks = [l for l in j["layers"] if l["type"] == "resnet"]
    assert len(blocks) == 2
    blocks[0]["bnParam"] = dict(blocks[0]["bnParam"], normGroups=16)
    m = model_cnn.load_from_json(j, 2)
    r0, r1 = [l for l in m.layers if l.type_name == "resnet"]
    inner0 = [l for l in r0.layers if isinstance(l, batch_norm.BatchNormLayer)]
    assert len(r0.layers) > r0.n_main and len(inner0) == 3                  # the projection's norm included
    assert all(l.norm_groups == 16 for l in inner0)
    assert not any(l.norm_groups for l in r1.layers if isinstance(l, batch_norm.BatchNormLayer))
    j2 = m.export_json()
    out = [l for l in j2["layers"] if l["type"] == "resnet"]
    assert out[0]["bnParam"] == {"enabled": True, "normGroups": 16} and out[1]["bnParam"] == {"enabled": True}
    assert _plain(model_cnn.load_from_json(j2, 2).export_json()) == _plain(j2)
    # the fused blocks (`bnrelu`): the key reaches their batchnorm-relu sub-layers
    m3 = modify.convert_bn_relu(m)
    subs = [l for l in [b for b in m3.layers if b.type_name == "resnet"][0].layers if isinstance(l, batch_norm.BatchNormLayer)]
    assert [l.type_name for l in subs] == ["batchnorm-relu", "batchnorm", "batchnorm"] and all(l.norm_groups == 16 for l in subs)
    # no fold plan for a block with group-mode norms; the plain block keeps its own
    blk = [b for b in m3.layers if b.type_name == "resnet"]
    assert blk[0]._fold_plan() is None


def test_modify_bn_groups_forth_and_back(tmp_path):
    m = _build()
    before = _plain(m.export_json())
    on = modify.modify_bn_groups(m, 8)
    bns = _bns(on)
    assert len(bns) == 2 + 2 * 2 and all(l.norm_groups == 8 for l in bns)
    j = on.export_json()
    for l in j["layers"]:
        if l["type"] in ("batchnorm", "batchnorm-relu"):
            assert l["normGroups"] == 8
        if l["type"] == "resnet":
            assert l["bnParam"] == {"enabled": True, "normGroups": 8}
    for a, b in zip(model_cnn.walk_layers(m.layers), model_cnn.walk_layers(on.layers)):
        assert a.type_name == b.type_name
        for pa, pb in zip(a.params(), b.params()):
            np.testing.assert_array_equal(pa.value, pb.value)
    off = modify.modify_bn_groups(on, 0)
    assert not any(l.norm_groups for l in _bns(off))
    assert _plain(off.export_json()) == before
    # the refusal names the layer
    with pytest.raises(ValueError, match=r"layer 2 \(batchnorm\) has 32 channels, which 5 does not divide"):
        modify.modify_bn_groups(m, 5)
    wide = _build("C.B[64,3] BN A C[96,3] BNA P.A[8] R")
    with pytest.raises(ValueError, match=r"layer 5 \(batchnorm-relu\) has 96 channels, which 64 does not divide"):
        modify.modify_bn_groups(wide, 64)
    with pytest.raises(ValueError, match="normGroups must be an integer >= 1"):
        modify.modify_bn_groups(m, -2)
    # the command line
    src, dst, back = (str(tmp_path / n) for n in ("a.mdl.gz", "b.mdl.gz", "c.mdl.gz"))
    model_cnn.save_to_file(m, src)
    assert modify.main(["--input", src, "--output", dst, "--modify-bn-groups", "8"]) == 0
    assert _plain(model_cnn.load_from_file(dst, 2).export_json()) == _plain(j)
    assert modify.main(["--input", dst, "--output", back, "--modify-bn-groups", "0"]) == 0
    assert _plain(model_cnn.load_from_file(back, 2).export_json()) == before
    assert "--modify-bn-groups" in modify.build_parser().format_help()
    with pytest.raises(ValueError, match="which 5 does not divide"):
        modify.main(["--input", src, "--output", dst, "--modify-bn-groups", "5"])
    # --convert-bn-relu on the same command line keeps the mode
    assert modify.main(["--input", src, "--output", dst, "--modify-bn-groups", "8", "--convert-bn-relu"]) == 0
    assert all(l.norm_groups == 8 for l in _bns(model_cnn.load_from_file(dst, 2)))


@pytest.mark.parametrize("groups,word", [(0.5, "normGroups must be an integer >= 1"), (-1, "normGroups must be an integer >= 1"),
                                         (True, "normGroups must be an integer >= 1"), ("8", "normGroups must be an integer >= 1"),
                                         (5, "normGroups 5 does not divide the layer's 32 channels"),
                                         (64, "normGroups 64 does not divide the layer's 32 channels")])
def test_refusals_of_the_group_count(groups, word):
    if isinstance(groups, (int, float)) and not isinstance(groups, bool):
        with pytest.raises(ValueError, match=word):          # when the layer is built from the grammar
            _build("C.B[32,3] BN.G[%r] P.A[8] R" % (groups,))
        with pytest.raises(ValueError, match=word):
            _build("C.B[32,3] BNA.G[%r] P.A[8] R" % (groups,))
    j = _build().export_json()
    for pick in ("batchnorm", "batchnorm-relu", "resnet"):
        jj = _plain(j)
        l = [x for x in jj["layers"] if x["type"] == pick][0]
        (l["bnParam"] if pick == "resnet" else l)["normGroups"] = groups
        with pytest.raises(ValueError, match=word):
            model_cnn.load_from_json(jj, 2)


def test_zero_is_off_in_a_file_and_refused_in_a_token():
    for tok in ("BN.G[0]", "BNA.G[0]"):
        with pytest.raises(ValueError, match="normGroups must be an integer >= 1"):
            _build("C.B[32,3] %s P.A[8] R" % tok)


def test_refusal_with_active_renorm_and_with_enabled_false():
    j = _plain(_build().export_json())
    for pick in ("batchnorm", "batchnorm-relu", "resnet"):
        for upd, word in (({"renormMaxR": 3.0}, "together with an active batch renormalisation"),
                          ({"renormMaxD": 0.5}, "together with an active batch renormalisation"),
                          ({"enabled": False}, "enabled false")):
            if pick == "batchnorm-relu" and "enabled" in upd:
                continue                     # (the fused layer has no `enabled` switch: the key is ignored there)
            jj = _plain(j)
            l = [x for x in jj["layers"] if x["type"] == pick][0]
            d = l["bnParam"] if pick == "resnet" else l
            d.update(upd, normGroups=8)
            with pytest.raises(ValueError, match=word):
                model_cnn.load_from_json(jj, 2)
            d["normGroups"] = 0              # without the mode the same file loads
            model_cnn.load_from_json(jj, 2)
    with pytest.raises(ValueError, match="together with an active batch renormalisation"):
        modify.modify_bn_groups(modify.modify_bn_renorm(_build(), 3, 5, 0), 8)
    with pytest.raises(ValueError, match="together with an active batch renormalisation"):
        modify.modify_bn_renorm(modify.modify_bn_groups(_build(), 8), 3, 5, 0)


def test_update_bn_selection_skips_group_mode_layers():
    m = _build(DESC_G)
    j = _plain(m.export_json())
    blocks = [l for l in j["layers"] if l["type"] == "resnet"]
    blocks[1]["bnParam"] = dict(blocks[1]["bnParam"], normGroups=4)
    m = model_cnn.load_from_json(j, 2)
    chosen = update_bn.select_bn_layers(m)
    r0, r1 = [l for l in m.layers if l.type_name == "resnet"]
    assert chosen == [l for l in r0.layers if isinstance(l, batch_norm.BatchNormLayer)] and len(chosen) == 2
    _, skipped = update_bn._select(m)
    assert sorted(l.norm_groups for l in skipped) == [4, 4, 8, 32]
    # nothing else to do: said so, nothing touched (no device work: the function returns before it packs the model)
    allg = modify.modify_bn_groups(_build(), 8)
    lines = []
    assert update_bn.update_bn(allg, [np.zeros((2, 3, 8, 8), np.float32)], log=lines.append) == []
    assert sum("group norm, 8 groups" in s for s in lines) == 6 and any("nothing to estimate" in s for s in lines)
    assert len(update_bn.select_bn_layers(_build())) == 6


def test_zoo_argument(monkeypatch):
    """the three builders take norm_groups = 0 by default; resnext50's own code path runs on a small stand-in for its desc (the
    real backbones take a minute to initialise on the host), the other two share its last line (zoo._norm_groups)"""
    import inspect
    from denet_amd.model import zoo
    for f in (zoo.denet34, zoo.denet101, zoo.resnext50):
        assert inspect.signature(f).parameters["norm_groups"].default == 0
        assert "return _norm_groups(m, norm_groups)" in inspect.getsource(f)
    monkeypatch.setattr(zoo, "RESNEXT50_DESC", "C.B[32,7,8] BN A RSN.O[64,3,4] nRSN.O[1,64,3,1,32,1,4] P.A[7] R")
    a, b = zoo.resnext50(1, image=64, class_num=10), zoo.resnext50(1, image=64, class_num=10, norm_groups=0)
    assert _plain(a.export_json()) == _plain(b.export_json()) and not batch_norm.group_norm_layers(a)
    g = zoo.resnext50(1, image=64, class_num=10, norm_groups=32)
    n = len(_bns(g))
    assert n == 7 and len(batch_norm.group_norm_layers(g)) == n and all(l.norm_groups == 32 for l in _bns(g))
    for x, y in zip(model_cnn.walk_layers(a.layers), model_cnn.walk_layers(g.layers)):
        for pa, pb in zip(x.params(), y.params()):
            np.testing.assert_array_equal(pa.value, pb.value)


@pytest.mark.parametrize("shape,groups", [((2, 7, 9, 64), 32), ((3, 5, 7, 96), 2), ((2, 4, 4, 32), 1), ((2, 6, 6, 64), 64),
                                          ((1, 1, 1, 32), 32)])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_closed_form_backward_equals_autograd(shape, groups, relu, res):
    """the formulas of the contract (numpy float64) against autograd through F.group_norm: <= 1e-12 relative (of max |ref|)"""
    g = torch.Generator().manual_seed(7 + shape[-1] + groups)
    C = shape[-1]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * (torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
         + torch.randn(C, generator=g, dtype=torch.float64))
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    rs = torch.randn(shape, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    eps = 1e-5
    m_one = shape[1] * shape[2] * (C // groups) == 1
    ref = gn_ref64(x, gamma, beta, groups, eps, relu, rs, dy)
    got = gn_closed_form(x.numpy(), gamma.numpy(), beta.numpy(), groups, eps, relu, rs.numpy() if res else None, dy.numpy())
    for k in ("y", "mu", "inv", "dx", "dgamma", "dbeta") + (("dres",) if res else ()):
        a, b = torch.from_numpy(np.asarray(got[k])), ref[k]
        scale = float(b.abs().max())
        if k == "dx" and m_one:
            # the exact dx is 0 there: autograd leaves the rounding of its terms inv * gamma * g (inv = eps ** -0.5), the scale
            scale = float(ref["inv"].max() * gamma.abs().max() * dy.abs().max())
        if k == "dgamma" and m_one:
            # likewise 0 exactly (xhat = 0): the scale is that of a term g * (x - mu) * inv
            scale = float(ref["inv"].max() * x.abs().max() * dy.abs().max())
        err = float((a - b).abs().max())
        assert err <= 1e-12 * max(scale, 1e-300) or (scale == 0.0 and err == 0.0), (k, err, scale)
    if m_one:
        # m = 1: var = 0, y = beta (+ res, relu), dx = 0
        want = beta.numpy()[None, None, None, :] + (rs.numpy() if res else 0.0)
        assert np.array_equal(got["y"], np.maximum(want, 0.0) if relu else want) and not got["dx"].any()
