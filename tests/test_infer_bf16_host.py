"""Opt-in bf16 inference (ops.INFER_PRECISION, csrc/conv_bf16.hip): the switch, the context manager, the driver flag and the
argument validation of the C entry points - everything that needs no GPU."""
import pytest

from denet_amd import lib as dlib
from denet_amd import ops, switches
from denet_amd.model import predict


def test_predict_parser_takes_the_precision_flag():
    base = ["--model", "m", "--input", "i"]
    parser = predict.build_parser()
    assert parser.parse_args(base).precision == "fp32"
    assert parser.parse_args(base + ["--precision", "bf16"]).precision == "bf16"
    assert parser.parse_args(base + ["--precision", "fp32"]).precision == "fp32"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--precision", "fp16"])


def test_infer_precision_rejects_unknown_names():
    with pytest.raises(ValueError):
        with ops.infer_precision("fp16"):
            pass
    assert ops.INFER_PRECISION == "fp32"


def test_infer_precision_restores_the_previous_value():
    assert ops.INFER_PRECISION == "fp32"
    with ops.infer_precision("bf16"):
        assert ops.INFER_PRECISION == "bf16"
        with ops.infer_precision("fp32"):
            assert ops.INFER_PRECISION == "fp32"
        assert ops.INFER_PRECISION == "bf16"
    assert ops.INFER_PRECISION == "fp32"
    with pytest.raises(RuntimeError):
        with ops.infer_precision("bf16"):
            raise RuntimeError("inside")
    assert ops.INFER_PRECISION == "fp32"


def test_a_wrong_module_value_raises_where_it_is_read(monkeypatch):
    """ops.INFER_PRECISION assigned directly: the inference branch of conv_fwd refuses anything but the two names before it
    touches a tensor"""
    monkeypatch.setattr(ops, "INFER_PRECISION", "fp16")
    with pytest.raises(ValueError):
        ops.conv_fwd(None, None, cache={"infer": True, "train": False})


def test_switch_is_listed_with_default_off():
    default, kind, _ = switches.SWITCHES["DENET_INFER_BF16"]
    assert default == "0" and kind == "kernels"
    assert switches.changes_kernels({"DENET_INFER_BF16": "1"})


def test_kernel_symbol_of_the_bf16_launches():
    assert ops.kernel_symbol(21, 128, 64, 0) == "conv_bf16_kernel<128, 64>"


def test_entry_points_validate_before_any_device_work():
    """callable on a CPU-only box: the channel rule is reported with null tensors (the pattern of test_host.py's C-ABI test)"""
    lib = dlib.load()
    assert lib.denet_conv_fwd_bf16(None, None, None, None, None, 0, 1, 8, 8, 33, 32, 3, 3, 3, 1, 1, 8, 8, None) == -1000
    err = lib.denet_last_error()
    assert b"multiple of 32" in err and b"C (33)" in err
    # the stem's 4 channels and a padded tap row are not this kernel's: errors, not a quiet other path
    assert lib.denet_conv_fwd_bf16(None, None, None, None, None, 0, 1, 8, 8, 4, 32, 3, 3, 3, 1, 1, 8, 8, None) == -1000
    assert lib.denet_conv_fwd_bf16(None, None, None, None, None, 0, 1, 8, 8, 32, 32, 3, 4, 3, 1, 1, 8, 8, None) == -1000
    assert b"square" in lib.denet_last_error()
    # a valid geometry with null tensors
    assert lib.denet_conv_fwd_bf16(None, None, None, None, None, 0, 1, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8, None) == -1000
    assert b"null" in lib.denet_last_error()
    assert lib.denet_filter_to_bf16(None, None, 64, None) == -1000
    assert lib.denet_filter_to_bf16(None, None, 0, None) == -1000
    assert lib.denet_abi_version() == 1
