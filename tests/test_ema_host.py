"""The exponential moving average of the weights (csrc/ema.hip), the part that needs no GPU: the decay
schedule, the validation of `ema_decay`, the driver flag, the naming of the average's files against find_restart, the C-ABI surface
with its refusals, and the recurrence restated in numpy float64. tests/test_ema_gpu.py imports `om_at`, `ema64`, `U` and `bound`."""
import math
import os

import numpy as np
import pytest

import cabi
from denet_amd import lib as dlib, ops
from denet_amd.model import model_cnn
from denet_amd.model.model_cnn import ema_decay_at

U = 2.0 ** -24            # unit roundoff of float32


def om_at(t, d):
    """om_t of the contract: 1 - d_t in double, rounded to float32 once; returned as the double the kernel's float holds"""
    return float(np.float32(1.0 - min(float(d), (1.0 + t) / (10.0 + t))))


def ema64(e, p, om):
    """one update of the recurrence in float64: e + om * (p - e)"""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + np.float64(om) * (p - e)


def bound(n_updates, a_max):
    """the derived bound on |device - float64| after n chained updates. One update errs by at most 3 u A with A = max(|e|, |p|):
    u |p - e| <= 2 u A from the subtraction (times om <= 1), u |result| <= u A from the fused rounding (the result lies between e
    and p). An error already in e is carried with the factor (1 - om) <= 1, so n updates err by at most 3 n u A_max"""
    return 3.0 * n_updates * U * float(a_max)


# ------------------------------------------------------------------------------------------------- the schedule
def test_decay_schedule():
    assert ema_decay_at(0, 0.999) == 0.1 and ema_decay_at(0, 0.5) == 0.1
    assert ema_decay_at(0, 0.05) == 0.05                                # a decay below the warm-up's start is used as it is
    for d in (0.5, 0.9, 0.999, 0.9999):
        seq = [ema_decay_at(t, d) for t in range(0, 20000)]
        assert all(a <= b for a, b in zip(seq[:-1], seq[1:])), d        # monotone
        assert all(0.0 < v <= d for v in seq)
        first = next(t for t in range(200000) if (1 + t) / (10 + t) >= d)
        assert ema_decay_at(first, d) == d and ema_decay_at(first + 1, d) == d and ema_decay_at(10 ** 9, d) == d
        if first > 0:
            assert ema_decay_at(first - 1, d) < d
    assert next(t for t in range(200000) if (1 + t) / (10 + t) >= 0.999) == 8990
    assert ema_decay_at(8990, 0.999) == 0.999 and ema_decay_at(8989, 0.999) == 8990 / 8999 < 0.999
    assert ema_decay_at(3, 0.9) == 4 / 13
    # om_t: formed in double, rounded once
    assert om_at(0, 0.999) == float(np.float32(0.9)) and om_at(8990, 0.999) == float(np.float32(1.0 - 0.999))
    assert om_at(5, 0.9) == float(np.float32(1.0 - ema_decay_at(5, 0.9)))


def test_recurrence_in_float64():
    rng = np.random.RandomState(0)
    e, p = rng.normal(size=100), rng.normal(size=100)
    assert np.array_equal(ema64(e, e, 0.3), e)                          # p == e: the entry keeps its value
    assert np.array_equal(ema64(e, p, 1.0), e + (p - e)) and np.array_equal(ema64(e, p, 0.0), e)
    out = ema64(e, p, 0.25)
    assert np.all(out >= np.minimum(e, p)) and np.all(out <= np.maximum(e, p))          # a convex combination
    assert np.allclose(out, 0.75 * e + 0.25 * p, rtol=0, atol=1e-15)
    # a constant sequence of parameters: after the warm-up the average has forgotten its start
    avg = np.zeros(3)
    for t in range(200):
        avg = ema64(avg, np.ones(3), om_at(t, 0.9))
    assert np.all(np.abs(avg - 1.0) < 1e-6)
    assert bound(5, 2.0) == 30 * U


# ------------------------------------------------------------------------------------------------- the model's argument
def _small_model():
    np.random.seed(3)
    m = model_cnn.ModelCNN()
    m.batch_size = 2
    m.class_num = 10
    m.build("C[32,3] BN A P[2] C[20,3] A R", (3, 32, 32), "relu", "half", ["he-backward"])
    return m


def test_decay_is_accepted_or_refused():
    m = _small_model()
    assert m.ema_decay == 0.0 and m.ema_auto is True and m.ema_updates == 0
    for ok in (0, 0.0, 0.5):
        m.ema_decay = ok
        m.build_train_func("sgd", skip_build=True)
        assert "train_step" in m.func
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        m.ema_decay = bad
        with pytest.raises(ValueError):
            m.build_train_func("sgd", skip_build=True)


def test_drivers_parse_the_flag():
    from denet_amd.model import train, train_multi
    for mod in (train, train_multi):
        parser = mod.build_parser()
        assert parser.parse_args(["--train", "x"]).ema == 0.0, mod.__name__
        args = parser.parse_args(["--train", "x", "--ema", "0.999"])
        assert args.ema == 0.999, mod.__name__
    m = model_cnn.ModelCNN()
    lines = []
    train.set_ema_args(m, args, lines.append)
    assert m.ema_decay == 0.999 and len(lines) == 1 and "0.999" in lines[0] and "(1 + t) / (10 + t)" in lines[0]
    args.model = "some.mdl.gz"
    lines = []
    train.set_ema_args(m, args, lines.append)
    assert len(lines) == 2 and "not resumed" in lines[1]
    m = model_cnn.ModelCNN()
    lines = []
    train.set_ema_args(m, parser.parse_args(["--train", "x"]), lines.append)
    assert m.ema_decay == 0.0 and lines == []


def test_file_names_and_restart(tmp_path):
    """the average's files carry `_ema` in front of `_epoch`: find_restart's glob `<prefix>_epoch*.mdl.gz` keeps ignoring them"""
    from denet_amd.model import train, train_multi
    assert train.ema_name("out/x_epoch003.mdl.gz") == "out/x_ema_epoch003.mdl.gz"
    assert train.ema_name("out/x_epoch003_final.mdl.gz") == "out/x_ema_epoch003_final.mdl.gz"
    assert train.ema_name("x_epoch001_subset004.mdl.gz") == "x_ema_epoch001_subset004.mdl.gz"
    assert train.ema_name("run_epoch9/x_epoch000.test") == "run_epoch9/x_ema_epoch000.test"
    for name in ("x_epoch001_final.mdl.gz", "x_ema_epoch002_final.mdl.gz"):
        (tmp_path / name).write_bytes(b"")
    fname, epoch, subset = train_multi.find_restart(str(tmp_path / "x"))
    assert os.path.basename(fname) == "x_epoch001_final.mdl.gz" and (epoch, subset) == (2, 0)


# ------------------------------------------------------------------------------------------------- the C ABI
NEW_ENTRIES = ("denet_ema_update", "denet_swap")


def test_cabi_declares_the_new_entries():
    """include/denet_hip.h and lib.SIGNATURES agree argument by argument, the library exports the symbols, the header says that
    neither has a reference counterpart, and the profile kinds have names"""
    hdr = open(cabi.HEADER).read()
    L = dlib.load()
    for name in NEW_ENTRIES:
        _, restype, declared = cabi.declaration(name)
        res, args = dlib.SIGNATURES[name]
        assert res is restype, name
        assert declared == list(args), (name, declared, args)
        assert hasattr(L, name)
    block = hdr[hdr.index("csrc/ema.hip"):hdr.index("int denet_swap")]
    assert block.count("No reference counterpart") >= 2
    assert ops.kernel_symbol(54, 0, 0, 0) == "ema_update_kernel" and ops.kernel_symbol(55, 0, 0, 0) == "swap_kernel"
    assert ops.EMA_KERNELS == ("ema_update_kernel", "swap_kernel")
    assert ops.kernel_symbol(52, 0, 0, 0) == "solver_coef_kernel" and ops.kernel_symbol(60, 0, 0, 0) == "sparse_bilinear_fwd_kernel"


def test_refusals_answer_without_a_device():
    L = dlib.load()
    a, b = 1 << 20, 1 << 21          # non-null, aligned, far apart: every call below is refused before a pointer is touched

    def last():
        return L.denet_last_error()

    assert L.denet_ema_update(None, b, 8, 0.1, None) == -1000 and b"null pointer" in last()
    assert L.denet_ema_update(a, None, 8, 0.1, None) == -1000 and b"null pointer" in last()
    assert L.denet_ema_update(a, b, 0, 0.1, None) == -1000 and b"n = 0" in last()
    assert L.denet_ema_update(a + 2, b, 8, 0.1, None) == -1000 and b"4-byte aligned" in last()
    assert L.denet_ema_update(a, a + 16, 8, 0.1, None) == -1000 and b"overlap" in last()
    for om in (-0.1, 1.5, float("nan")):
        assert L.denet_ema_update(a, b, 8, om, None) == -1000 and b"om" in last()
    assert L.denet_swap(None, b, 8, None) == -1000 and b"null pointer" in last()
    assert L.denet_swap(a, None, 8, None) == -1000 and b"null pointer" in last()
    assert L.denet_swap(a, b, -3, None) == -1000 and b"n = -3" in last()
    assert L.denet_swap(a, b + 1, 8, None) == -1000 and b"4-byte aligned" in last()
    assert L.denet_swap(a, a, 8, None) == -1000 and b"overlap" in last()
    assert L.denet_swap(a + 32, a, 9, None) == -1000 and b"overlap" in last()


def test_model_refuses_misuse_without_a_device():
    m = _small_model()
    with pytest.raises(RuntimeError, match="before the first update"):
        with m.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="the average is off"):
        m.ema_step()
    assert math.isfinite(ema_decay_at(0, 0.5))
