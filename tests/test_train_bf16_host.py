"""Opt-in bf16 training (ops.TRAIN_PRECISION, csrc/conv_bf16_train.hip): the switch, the context manager, the driver flags, the
kernel names and the argument validation of the C entry points - everything that needs no GPU."""
import pytest

from denet_amd import lib as dlib
from denet_amd import ops, switches
from denet_amd.model import model_cnn, train, train_multi


@pytest.mark.parametrize("build_parser", [train.build_parser, train_multi.build_parser], ids=["model-train", "model-train-multi"])
def test_training_parsers_take_the_precision_flag(build_parser):
    parser = build_parser()
    assert parser.parse_args([]).precision == "fp32"
    assert parser.parse_args(["--precision", "bf16"]).precision == "bf16"
    assert parser.parse_args(["--precision", "fp32"]).precision == "fp32"
    with pytest.raises(SystemExit):
        parser.parse_args(["--precision", "fp16"])


def test_train_precision_rejects_unknown_names():
    with pytest.raises(ValueError):
        with ops.train_precision("fp16"):
            pass
    assert ops.TRAIN_PRECISION == "fp32"


def test_train_precision_restores_the_previous_value():
    assert ops.TRAIN_PRECISION == "fp32"
    with ops.train_precision("bf16"):
        assert ops.TRAIN_PRECISION == "bf16" and ops.train_bf16()
        with ops.train_precision("fp32"):
            assert ops.TRAIN_PRECISION == "fp32" and not ops.train_bf16()
        assert ops.TRAIN_PRECISION == "bf16"
    assert ops.TRAIN_PRECISION == "fp32"
    with pytest.raises(RuntimeError):
        with ops.train_precision("bf16"):
            raise RuntimeError("inside")
    assert ops.TRAIN_PRECISION == "fp32"


def test_the_two_precision_switches_are_independent():
    with ops.train_precision("bf16"):
        assert ops.INFER_PRECISION == "fp32"
        with ops.infer_precision("bf16"):
            assert ops.TRAIN_PRECISION == "bf16"
        assert ops.INFER_PRECISION == "fp32"
    with ops.infer_precision("bf16"):
        assert ops.TRAIN_PRECISION == "fp32"


def test_switch_is_listed_with_default_off():
    default, kind, _ = switches.SWITCHES["DENET_TRAIN_BF16"]
    assert default == "0" and kind == "kernels"
    assert switches.changes_kernels({"DENET_TRAIN_BF16": "1"})


def test_kernel_symbols_of_the_new_launches():
    assert ops.kernel_symbol(22, 64, 128, 0) == "conv_bf16_wgrad_kernel<64, 128>"
    assert ops.kernel_symbol(23, 0, 0, 0) == "conv_bf16_wgrad_reduce_kernel"
    assert ops.kernel_symbol(24, 0, 0, 0) == "filter_to_bf16_dgrad_kernel"
    assert ops.kernel_symbol(21, 128, 64, 0) == "conv_bf16_kernel<128, 64>"


def test_entry_points_validate_before_any_device_work():
    """callable on a CPU-only box: every rule is reported with null tensors (the pattern of test_host.py's C-ABI test)"""
    lib = dlib.load()
    ok = (1, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8)              # N H W C K R S S_real stride pad OH OW

    def geom(**kw):
        names = ("N", "H", "W", "C", "K", "R", "S", "S_real", "stride", "pad", "OH", "OW")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    # the filter gradient
    assert lib.denet_conv_wgrad_bf16(None, None, None, None, 0, *geom(C=33), None) == -1000
    err = lib.denet_last_error()
    assert b"conv_wgrad_bf16" in err and b"multiple of 32" in err and b"C (33)" in err
    assert lib.denet_conv_wgrad_bf16(None, None, None, None, 0, *geom(S=4), None) == -1000
    assert b"square" in lib.denet_last_error()
    assert lib.denet_conv_wgrad_bf16(None, None, None, None, 0, *geom(stride=3), None) == -1000
    assert b"power of two" in lib.denet_last_error()
    assert lib.denet_conv_wgrad_bf16(None, None, None, None, 0, *geom(OH=9), None) == -1000
    assert b"OH=9" in lib.denet_last_error()
    assert lib.denet_conv_wgrad_bf16(None, None, None, None, 0, *ok, None) == -1000
    assert b"null" in lib.denet_last_error()
    # the data gradient: stride 1, pad <= R - 1, an uncut output
    assert lib.denet_conv_dgrad_bf16(None, None, None, None, *geom(K=48), None) == -1000
    assert b"conv_dgrad_bf16" in lib.denet_last_error() and b"K (48)" in lib.denet_last_error()
    assert lib.denet_conv_dgrad_bf16(None, None, None, None, *geom(stride=2, OH=4, OW=4), None) == -1000
    assert b"stride 1 only" in lib.denet_last_error()
    assert lib.denet_conv_dgrad_bf16(None, None, None, None, *geom(pad=3, OH=12, OW=12), None) == -1000
    assert b"R - 1" in lib.denet_last_error()
    assert lib.denet_conv_dgrad_bf16(None, None, None, None, *geom(OH=7, OW=7), None) == -1000
    assert b"cut output" in lib.denet_last_error()
    assert lib.denet_conv_dgrad_bf16(None, None, None, None, *ok, None) == -1000
    assert b"null" in lib.denet_last_error()
    # the rotated filter copy
    assert lib.denet_filter_to_bf16_dgrad(None, None, 32, 3, 3, 16, None) == -1000
    assert b"C (16)" in lib.denet_last_error()
    assert lib.denet_filter_to_bf16_dgrad(None, None, 32, 3, 3, 32, None) == -1000
    assert b"null" in lib.denet_last_error()


def test_slicing_rule_depends_on_the_geometry_only():
    """at most 128 slices, at least 4 chunks of 32 pixels each, none empty; no workspace for one slice"""
    lib = dlib.load()
    assert lib.denet_conv_wgrad_bf16_slices(1, 32, 32, 1, 1, 1, 1) == 1
    assert lib.denet_conv_wgrad_bf16_workspace_bytes(1, 32, 32, 1, 1, 1, 1) == 0
    # 2 x 15 x 14 = 420 pixels = 14 chunks (the last one ragged), one tile: 3 slices of 5 + 5 + 4 chunks
    assert lib.denet_conv_wgrad_bf16_slices(2, 32, 32, 1, 1, 15, 14) == 3
    assert lib.denet_conv_wgrad_bf16_workspace_bytes(2, 32, 32, 1, 1, 15, 14) == 3 * 32 * 32 * 4
    assert lib.denet_conv_wgrad_bf16_slices(32, 64, 64, 3, 3, 128, 128) == 102       # 512 // 5 tiles = 102 asked, 161 chunks each
    assert lib.denet_conv_wgrad_bf16_slices(64, 32, 32, 1, 1, 512, 512) == 128
    assert lib.denet_conv_wgrad_bf16_slices(0, 32, 32, 1, 1, 8, 8) == 0


def test_head_bf16x3_and_bf16_training_are_not_mixed(monkeypatch):
    monkeypatch.setattr(ops, "HEAD_BF16X3", True)
    model = model_cnn.ModelCNN()
    with ops.train_precision("bf16"):
        with pytest.raises(ValueError):
            model.build_train_func("nesterov", skip_build=True)


def test_eligibility_follows_the_rules_of_the_kernels():
    """a layer the bf16 kernels refuse is not eligible (it runs what it runs in fp32 mode): here the stride rule and the stem"""
    import numpy
    numpy.random.seed(0)
    model = model_cnn.ModelCNN()
    model.batch_size, model.class_num = 2, 10
    model.build("C[32,3] C[64,3] C[64,3,2] C[64,3,3] C[64,1,4] P.A[2] R", (3, 48, 48), "relu", "half", ["he-backward"])
    convs = [l for l in model_cnn.walk_layers(model.layers) if l.type_name == "conv"]
    assert [l.stride[0] for l in convs[:5]] == [1, 1, 2, 3, 4]
    assert [l._bf16_train_eligible() for l in convs] == [False, True, True, False, True, False]
    lib = dlib.load()
    assert lib.denet_conv_fwd_bf16(None, None, None, None, None, 0, 2, 24, 24, 64, 64, 3, 3, 3, 3, 1, 8, 8, None) == -1000
    assert b"power of two" in lib.denet_last_error()
