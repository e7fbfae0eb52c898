"""Border-keeping pooling (`P.B` / `P.AB`, ignoreBorder false) on the host: the layer builds, carries the shape of the tensor
pool_2d(..., ignore_border=False) returns, refuses what the reference cannot mean, survives the JSON round trip, and
`model-modify --use-cudnn-pool` performs the reference's edit (denet/model/modify.py:62-68). No device work."""
import ctypes
import math

import numpy as np
import pytest

from denet_amd import lib as dlib
from denet_amd import ops
from denet_amd.model import model_cnn, modify


def _build(desc, data_shape, B=2, cls=10):
    m = model_cnn.ModelCNN()
    m.batch_size, m.class_num = B, cls
    m.build(desc, data_shape, "relu", "half", ["he-backward"])
    return m


def _border_out(r, k, s):
    """the rule as the issue states it, restated here (not imported from the code under test)"""
    return (r - 1) // s + 1 if s >= k else max(0, (r - 1 - k + s) // s) + 1


# (r, k, s, expected): s > k, s == k, s < k, even and odd maps, an input smaller than the window
SHAPES = [(32, 3, 2, 16), (112, 3, 2, 56), (6, 3, 2, 3), (2, 3, 2, 1),        # s < k (even maps; 2 < 3: smaller than the window)
          (7, 2, 2, 4), (8, 2, 2, 4), (15, 2, 2, 8), (1, 2, 2, 1), (2, 3, 3, 1), (9, 3, 3, 3), (10, 3, 3, 4),      # s == k
          (9, 2, 3, 3), (10, 2, 3, 4), (10, 2, 4, 3), (11, 1, 2, 6), (3, 2, 5, 1)]                                  # s > k


@pytest.mark.parametrize("r,k,s,out", SHAPES)
@pytest.mark.parametrize("tag", ["B", "AB"])
def test_border_pool_builds_with_the_tensor_shape(r, k, s, out, tag):
    assert _border_out(r, k, s) == out == ops.pool_border_out(r, k, s) == int(math.ceil(r / s))
    m = _build("P.%s[%i,%i]" % (tag, k, s), (32, r, r))
    pool = m.layers[-1]
    assert pool.type_name == "pool" and pool.ignore_border is False and tuple(pool.pad) == (0, 0)
    assert pool.mode == ("average_inc_pad" if "A" in tag else "max")
    assert pool.size == (k, k) and pool.stride == (s, s)
    assert pool.output_shape == (2, 32, out, out)


def test_border_pool_default_stride_and_non_square_map():
    m = _build("P.AB[2]", (32, 7, 12))
    assert m.layers[-1].stride == (2, 2) and m.layers[-1].output_shape == (2, 32, 4, 6)
    m = _build("P.B[3,2]", (64, 14, 20))
    assert m.layers[-1].output_shape == (2, 64, 7, 10)


def test_output_size_rule_against_torch_ceil_mode_and_the_reference_line():
    """the rule equals torch's ceil_mode output size wherever the input is at least as large as the window; against the
    reference's own ceil(r / s) (pool.py:32-33) it differs 584 times for k, s in 1..7, r in 1..39, always with s < k"""
    import torch
    import torch.nn.functional as Fn
    differ = 0
    for k in range(1, 8):
        for s in range(1, 8):
            for r in range(1, 40):
                own = ops.pool_border_out(r, k, s)
                assert own == _border_out(r, k, s)
                if r >= k:
                    t = Fn.max_pool2d(torch.zeros(1, 1, r, r, dtype=torch.float64), k, s, padding=0, ceil_mode=True)
                    assert tuple(t.shape[2:]) == (own, own), (r, k, s)
                if own != int(math.ceil(r / s)):
                    differ += 1
                    assert s < k
    assert differ == 584


def test_refusals_carry_a_message():
    # padding with the B tag: Theano refuses padding != (0, 0) with ignore_border=False
    with pytest.raises(ValueError, match="pad .* with ignoreBorder false"):
        _build("P.B[3,2,1]", (32, 32, 32))
    with pytest.raises(ValueError, match="pad .* with ignoreBorder false"):
        _build("P.AB[3,2,1]", (32, 32, 32))
    # k = 3, s = 2 on an odd map: the tensor has 16 rows, the reference's layer declares 17; both sizes are named
    with pytest.raises(ValueError, match=r"yields 16 x 16.*17 x 17"):
        _build("P.B[3,2]", (32, 33, 33))
    with pytest.raises(ValueError, match=r"yields 3 x 3.*5 x 5"):
        _build("P.AB[3,1]", (32, 5, 5))
    # one axis is enough
    with pytest.raises(ValueError, match=r"yields 16 x 16.*16 x 17"):
        _build("P.B[3,2]", (32, 32, 33))


def _pool_json(model):
    j = model.export_json()
    index = [i for i, l in enumerate(j["layers"]) if l["type"] == "pool"][0]
    return j, j["layers"][index]


def test_unequal_pairs_run_border_keeping_only():
    """a model file whose pool size / stride differ per axis: built in border-keeping mode, refused with a message in cuDNN mode"""
    j, p = _pool_json(_build("C.B[32,3] P.B[2]", (3, 16, 15)))
    p["size"], p["stride"] = (3, 2), (2, 2)
    m = model_cnn.load_from_json(j, 2)
    pool = [l for l in m.layers if l.type_name == "pool"][0]
    assert pool.size == (3, 2) and pool.stride == (2, 2) and pool.output_shape == (2, 32, 8, 8)
    p["ignoreBorder"] = True
    with pytest.raises(ValueError, match="differ per axis"):
        model_cnn.load_from_json(j, 2)
    p["size"], p["stride"], p["pad"] = (2, 2), (2, 1), (0, 0)
    with pytest.raises(ValueError, match="differ per axis"):
        model_cnn.load_from_json(j, 2)
    # padding in the JSON form of a border-keeping layer
    p["size"], p["stride"], p["pad"], p["ignoreBorder"] = (3, 3), (2, 2), (1, 1), False
    with pytest.raises(ValueError, match="pad .* with ignoreBorder false"):
        model_cnn.load_from_json(j, 2)


def test_json_round_trip_keeps_the_border_mode(tmp_path):
    np.random.seed(2)
    m = _build("C.B[32,7,2] BN A P.B[3,2] C[32,3] BN A P.AB[2] R", (3, 60, 64))
    fname = str(tmp_path / "border.mdl.gz")
    model_cnn.save_to_file(m, fname)
    again = model_cnn.load_from_file(fname, 2)
    pools = [l for l in m.layers if l.type_name == "pool"]
    pools2 = [l for l in again.layers if l.type_name == "pool"]
    assert [(p.mode, p.size, p.stride, p.pad, p.ignore_border) for p in pools] == \
        [("max", (3, 3), (2, 2), (0, 0), False), ("average_inc_pad", (2, 2), (2, 2), (0, 0), False)]
    assert [p.output_shape for p in pools] == [(2, 32, 15, 16), (2, 32, 8, 8)]
    for a, b in zip(pools, pools2):
        assert (a.mode, a.size, a.stride, a.pad, a.ignore_border, a.output_shape) == \
            (b.mode, b.size, b.stride, b.pad, b.ignore_border, b.output_shape)
        assert b.ignore_border is False
    assert [l.output_shape for l in again.layers] == [l.output_shape for l in m.layers]
    assert [l["ignoreBorder"] for l in again.export_json()["layers"] if l["type"] == "pool"] == [False, False]


def test_fused_stem_link_skips_a_border_keeping_pool():
    """ModelCNN.build_train_func links BN + ReLU + max pool into one pass for the cuDNN mode only (skip_build: no device)"""
    for desc, linked in (("C.B[32,7,2] BN A P.B[3,2] R", False), ("C.B[32,7,2] BN A P[3,2,1] R", True),
                         ("C.B[32,7,2] BNA P.B[3,2] R", False), ("C.B[32,7,2] BNA P[3,2,1] R", True)):
        m = _build(desc, (3, 32, 32))
        m.build_train_func("sgd", skip_build=True)
        pools = [l for l in m.layers if getattr(l, "pool_behind", None) is not None]
        assert (len(pools) == 1) == linked, desc


STEM_DESC = "C.B[32,7,2] BN A %s nRSN.O[2,32,3] nRSN.O[2,64,3,2] nRSN.O[2,128,3,2] P.A[2] R.TB"


def _params_of(model):
    return [p.value.copy() for l in model_cnn.walk_layers(model.layers) for p in l.params()]


def test_use_cudnn_pool_converts_a_border_keeping_stem(tmp_path, capsys):
    np.random.seed(4)
    m = _build(STEM_DESC % "P.B[3,2]", (3, 64, 64))
    src, out, kept = str(tmp_path / "cls.mdl.gz"), str(tmp_path / "cudnn.mdl.gz"), str(tmp_path / "kept.mdl.gz")
    model_cnn.save_to_file(m, src)
    assert modify.main(["--input", src, "--output", out, "--use-cudnn-pool"]) == 0
    got = model_cnn.load_from_file(out, 2)
    before = [l for l in m.layers if l.type_name == "pool"]
    after = [l for l in got.layers if l.type_name == "pool"]
    assert before[0].ignore_border is False and before[0].pad == (0, 0)
    assert after[0].pad == (1, 1) and after[0].ignore_border is True
    assert after[0].size == (3, 3) and after[0].stride == (2, 2) and after[0].mode == "max"
    assert after[0].output_shape == before[0].output_shape == (2, 32, 16, 16)
    assert [l.type_name for l in got.layers] == [l.type_name for l in m.layers]
    assert [l.output_shape for l in got.layers] == [l.output_shape for l in m.layers]
    a, b = _params_of(m), _params_of(got)
    assert len(a) == len(b) > 0
    for pa, pb in zip(a, b):
        np.testing.assert_array_equal(pa, pb)
    # without the flag the pool layer is kept as it was
    assert modify.main(["--input", src, "--output", kept]) == 0
    same = model_cnn.load_from_file(kept, 2)
    pool = [l for l in same.layers if l.type_name == "pool"][0]
    assert pool.ignore_border is False and pool.pad == (0, 0) and pool.size == (3, 3) and pool.stride == (2, 2)
    assert [l["ignoreBorder"] for l in same.export_json()["layers"] if l["type"] == "pool"] == [False, True]
    assert "--use-cudnn-pool" in modify.build_parser().format_help()
    assert "accepted for the recipes" not in modify.build_parser().format_help()


def test_use_cudnn_pool_leaves_a_cudnn_model_as_it_is(tmp_path):
    """a model without a border-keeping pool comes out of --use-cudnn-pool as it comes out without the flag"""
    np.random.seed(5)
    m = _build(STEM_DESC % "P[3,2,1]", (3, 64, 64))
    src, a, b = str(tmp_path / "cls.mdl.gz"), str(tmp_path / "a.mdl.gz"), str(tmp_path / "b.mdl.gz")
    model_cnn.save_to_file(m, src)
    assert modify.main(["--input", src, "--output", a, "--use-cudnn-pool"]) == 0
    assert modify.main(["--input", src, "--output", b]) == 0
    import gzip
    import re
    stamp = re.compile(rb'"date": "[^"]*"')          # the file carries the second it was written in
    ta, tb = [stamp.sub(b"", gzip.open(f).read()) for f in (a, b)]
    assert ta == tb and len(stamp.findall(gzip.open(a).read())) == 1
    assert modify.use_cudnn_pool(m) is m


def test_denet_recipe_replays_from_a_border_keeping_stem(tmp_path):
    """the two model-modify commands of examples/denet34.sh (skip variant) on a classifier whose stem pool is `P.B[3,2]`, as the
    published base models': the result equals the one from the same classifier written with `P[3,2,1]`"""
    head = "PI[2] C[64,3] SKIP[1] BNA PI[2] C[32,3] SKIP[0] BNA DNC[16,100] DNS[3,4,0.01,0.1] C.B[64,1] BNA DND[0.5,1,1]"
    models = {}
    for name, pool in (("border", "P.B[3,2]"), ("cudnn", "P[3,2,1]")):
        np.random.seed(4)
        m = _build(STEM_DESC % pool, (3, 64, 64))
        src, mid, dst = [str(tmp_path / (name + s)) for s in ("_cls.mdl.gz", "_skipsrc.mdl.gz", "_initial.mdl.gz")]
        model_cnn.save_to_file(m, src)
        assert modify.main(["--input", src, "--output", mid, "--modify-bn", "1", "0.9", "1e-5", "--convert-bn-relu",
                            "--use-cudnn-pool", "--class-num", "20", "--image-size", "128", "128", "--layer-remove", "3",
                            "--layer-insert", "6:SKIPSRC.X[0]", "7:SKIPSRC.X[1]"]) == 0
        assert modify.main(["--input", mid, "--output", dst, "--layer-append"] + head.split()) == 0
        models[name] = model_cnn.load_from_file(dst, 2)
    got, ref = models["border"], models["cudnn"]
    assert got.layers[-1].type_name == "denet-detect" and got.class_num == 20 and tuple(got.data_shape) == (3, 128, 128)
    assert [l.type_name for l in got.layers] == [l.type_name for l in ref.layers]
    assert [l.output_shape for l in got.layers] == [l.output_shape for l in ref.layers]
    pool = [l for l in got.layers if l.type_name == "pool"][0]
    assert pool.pad == (1, 1) and pool.ignore_border is True and pool.output_shape == (2, 32, 32, 32)
    a, b = _params_of(got), _params_of(ref)
    assert len(a) == len(b) > 0
    for pa, pb in zip(a, b):
        np.testing.assert_array_equal(pa, pb)


def test_entry_points_check_their_arguments_before_any_device_work():
    """argument validation happens before any launch: callable without a device"""
    L = dlib.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused
    for fn in (L.denet_maxpool_border_fwd, L.denet_avgpool_border_fwd, L.denet_avgpool_border_bwd):
        assert fn(None, None, 2, 16, 16, 32, 8, 8, 3, 3, 2, 2, None) == -1000
        assert b"null pointer" in L.denet_last_error()
        assert fn(p, p, 2, 16, 16, 30, 8, 8, 3, 3, 2, 2, None) == -1000          # C % 4
        assert b"multiple of 4" in L.denet_last_error()
        assert fn(p, p, 2, 16, 16, 32, 9, 8, 3, 3, 2, 2, None) == -1000          # window 8 would start at row 16 of 16
        assert b"start inside the map" in L.denet_last_error()
        assert fn(p, p, 2, 16, 16, 32, 8, 9, 3, 3, 2, 2, None) == -1000
        assert fn(p, p, 2, 16, 16, 32, 8, 8, 0, 3, 2, 2, None) == -1000
        assert fn(p, p, 2, 16, 16, 32, 8, 8, 3, 3, 2, 0, None) == -1000
    assert L.denet_maxpool_border_bwd(p, p, None, p, 2, 16, 16, 32, 8, 8, 3, 3, 2, 2, None) == -1000
    assert b"null pointer" in L.denet_last_error()
    assert L.denet_maxpool_border_bwd(p, p, p, p, 2, 16, 16, 32, 9, 8, 3, 3, 2, 2, None) == -1000
    assert b"start inside the map" in L.denet_last_error()
