"""Global-norm gradient clipping and on-device gradient norms (csrc/grad_norm.hip), the part that needs no
GPU: the driver flags, the limit's validation, the chunk table of the reduction, the C-ABI surface with its refusals, and the
contract's coefficient restated in numpy float64. tests/test_grad_clip_gpu.py imports RANGES, `laid_out` and `coef64`."""
import math

import numpy as np
import pytest

import cabi
from denet_amd import lib as dlib, ops
from denet_amd.model import model_cnn

CH = ops.NORM_CHUNK
# 64, 192, exactly one chunk, one chunk + 64, five chunks + 192 floats
LENGTHS = (64, 192, CH, CH + 64, 5 * CH + 192)
GAP = 64          # floats between two ranges that no chunk may cover


def laid_out(lengths=LENGTHS, gap=GAP):
    """[(offset, length)] of the ranges with `gap` floats in front of, between and behind them, and the buffer's size"""
    ranges, off = [], gap
    for n in lengths:
        ranges.append((off, n))
        off += n + gap
    return ranges, off


RANGES, TOTAL = laid_out()


def coef64(norm, c):
    """the contract: coef = c / norm if norm > c else 1 (NaN: 1, inf: 0)"""
    norm, c = np.float64(norm), np.float64(c)
    return c / norm if norm > c else np.float64(1.0)


def test_drivers_parse_the_flags():
    from denet_amd.model import train, train_multi
    for mod in (train, train_multi):
        parser = mod.build_parser()
        args = parser.parse_args(["--train", "x"])
        assert args.gradient_clip == 0.0 and args.gradient_norms is False, mod.__name__
        args = parser.parse_args(["--train", "x", "--gradient-clip", "2.5", "--gradient-norms"])
        assert args.gradient_clip == 2.5 and args.gradient_norms is True, mod.__name__
    m = model_cnn.ModelCNN()
    train.set_gradient_norm_args(m, args)
    assert m.gradient_clip == 2.5 and m.track_grad_norm is True
    assert model_cnn.ModelCNN().gradient_clip == 0.0 and model_cnn.ModelCNN().track_grad_norm is False


def _small_model():
    np.random.seed(3)
    m = model_cnn.ModelCNN()
    m.batch_size = 2
    m.class_num = 10
    m.build("C[32,3] BN A P[2] C[20,3] A R", (3, 32, 32), "relu", "half", ["he-backward"])
    return m


def test_limit_is_accepted_or_refused():
    m = _small_model()
    m.gradient_clip = 0.5
    m.build_train_func("sgd", skip_build=True)             # (raised NotImplementedError before clipping existed)
    assert "train_step" in m.func
    m.gradient_clip = 0.0
    m.build_train_func("sgd", skip_build=True)
    for bad in (-1.0, float("nan"), float("inf")):
        m.gradient_clip = bad
        with pytest.raises(ValueError):
            m.build_train_func("sgd", skip_build=True)


def test_chunk_table_covers_every_range_once():
    table, first = ops.norm_chunks(RANGES)
    covered = np.zeros(TOTAL, dtype=np.int64)
    for off, n, seg in table:
        assert n % 4 == 0 and off % 4 == 0 and 0 < n <= CH
        lo, length = RANGES[seg]
        assert lo <= off and off + n <= lo + length, "a chunk crosses its range"
        covered[off:off + n] += 1
    expect = np.zeros(TOTAL, dtype=np.int64)
    for lo, length in RANGES:
        expect[lo:lo + length] = 1
    assert np.array_equal(covered, expect)                  # every float of every range exactly once, nothing outside
    assert len(first) == len(RANGES) + 1 and first[0] == 0 and first[-1] == len(table)
    assert [b - a for a, b in zip(first[:-1], first[1:])] == [1, 1, 1, 2, 6]
    for seg, (lo, length) in enumerate(RANGES):              # a segment's chunks: consecutive, in order, end to end
        chunks = table[first[seg]:first[seg + 1]]
        assert all(c[2] == seg for c in chunks)
        assert chunks[0][0] == lo and chunks[-1][0] + chunks[-1][1] == lo + length
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks[:-1], chunks[1:]))
    assert [c[2] for c in table] == sorted(c[2] for c in table)
    with pytest.raises(AssertionError):
        ops.norm_chunks([(0, 60)])
    with pytest.raises(AssertionError):
        ops.norm_chunks([(0, 128), (64, 64)])


NEW_ENTRIES = ("denet_grad_norm_chunk_len", "denet_grad_norm_check_table", "denet_grad_norm_workspace_bytes", "denet_grad_norm",
               "denet_solver_step_coef", "denet_solver_adam_coef")


def test_cabi_declares_the_new_entries():
    """include/denet_hip.h and lib.SIGNATURES agree on the new entries, argument by argument; the coef solvers are the plain
    signatures plus one pointer"""
    for name in NEW_ENTRIES:
        _, restype, declared = cabi.declaration(name)
        res, args = dlib.SIGNATURES[name]
        assert res is restype, name
        assert declared == list(args), (name, declared, args)
    for plain in ("denet_solver_step", "denet_solver_adam"):
        a, b = dlib.SIGNATURES[plain][1], dlib.SIGNATURES[plain + "_coef"][1]
        assert list(b) == list(a[:-1]) + [dlib.P, dlib.P]


def test_refusals_answer_without_a_device():
    L = dlib.load()
    assert L.denet_grad_norm_chunk_len() == CH and CH % 64 == 0
    assert L.denet_grad_norm_workspace_bytes(0, 1) == 0 and L.denet_grad_norm_workspace_bytes(10, 3) >= 10 * 8 + 2 * 3 * 4
    one = 64          # a non-null, 16-byte aligned "pointer": every call below is refused before it is touched

    def last():
        return L.denet_last_error()

    assert L.denet_grad_norm(None, one, 1, 1, 1.0, 0.0, one, one, one, None, None) == -1000 and b"null pointer" in last()
    assert L.denet_grad_norm(one, None, 1, 1, 1.0, 0.0, one, one, one, None, None) == -1000 and b"null pointer" in last()
    assert L.denet_grad_norm(one, one, 1, 1, 1.0, 0.0, None, one, one, None, None) == -1000 and b"null pointer" in last()
    assert L.denet_grad_norm(one, one, 1, 1, 1.0, 0.0, one, None, one, None, None) == -1000 and b"null pointer" in last()
    assert L.denet_grad_norm(one, one, 1, 1, 1.0, 0.0, one, one, None, None, None) == -1000 and b"null pointer" in last()
    assert L.denet_grad_norm(one, one, 0, 1, 1.0, 0.0, one, one, one, None, None) == -1000 and b"n_chunks" in last()
    assert L.denet_grad_norm(one, one, 4, 0, 1.0, 0.0, one, one, one, None, None) == -1000 and b"segments" in last()
    assert L.denet_grad_norm(one, one, 4, 5, 1.0, 0.0, one, one, one, None, None) == -1000 and b"segments" in last()
    assert L.denet_grad_norm(one + 4, one, 1, 1, 1.0, 0.0, one, one, one, None, None) == -1000 and b"aligned" in last()
    assert L.denet_grad_norm(one, one, 1, 1, float("nan"), 0.0, one, one, one, None, None) == -1000 and b"scale" in last()
    assert L.denet_solver_step_coef(one, one, one, 8, 4, 0.1, 0.9, 0, 0.0, 1.0, 0, None, None) == -1000 and b"solver_step_coef" in last()
    assert L.denet_solver_step_coef(one, one, one, 8, 4, 0.1, 0.9, 0, 0.0, 1.0, 2, one, None) == -1000 and b"mode" in last()
    assert L.denet_solver_adam_coef(one, one, one, one, 8, 4, 0.1, 0.9, 0.999, 0, 0.0, 1.0, None, None) == -1000 and b"solver_adam_coef" in last()
    assert L.denet_solver_adam_coef(one, one, one, one, 8, 4, 0.1, 1.0, 0.999, 0, 0.0, 1.0, one, None) == -1000 and b"betas" in last()

    # the table's rules, checked on the host copy
    table, _ = ops.norm_chunks(RANGES)

    def check(rows, n_seg=len(RANGES), n=TOTAL):
        t = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 3))
        return L.denet_grad_norm_check_table(t.ctypes.data, len(rows), n_seg, n)

    assert check(table) == 0
    assert L.denet_grad_norm_check_table(None, 1, 1, 64) == -1000 and b"null pointer" in last()
    assert check(table[:1], 1, 0) == -1000                                          # leaves the buffer
    too_long = [(0, CH + 64, 0)]
    assert check(too_long, 1, 4 * CH) == -1000 and b"floats long" in last()
    assert check([(2, 64, 0)], 1, 4 * CH) == -1000 and b"misaligned" in last()
    assert check([(0, 62, 0)], 1, 4 * CH) == -1000 and b"misaligned" in last()
    assert check([(0, 64, 0), (32, 64, 0)], 1, 4 * CH) == -1000 and b"overlaps" in last()
    assert check([(0, 64, 0), (64, 64, 2), (128, 64, 2)], 3, 4 * CH) == -1000 and b"behind segment" in last()
    assert check([(0, 64, 0), (64, 64, 0), (128, 64, 1)], 3, 4 * CH) == -1000 and b"the chunks name" in last()
    assert check(table, len(RANGES), TOTAL - GAP - 4) == -1000 and b"leaves" in last()


def test_contract_in_float64():
    c = 2.0
    assert coef64(1.5, c) == 1.0
    assert coef64(2.0, c) == 1.0                                        # norm == c: exactly 1
    assert coef64(np.nextafter(2.0, 3.0), c) < 1.0
    assert coef64(8.0, c) == 0.25
    assert coef64(float("nan"), c) == 1.0                               # NaN is not rescued: the step poisons the weights as before
    assert coef64(float("inf"), c) == 0.0 and math.isnan(0.0 * float("inf"))
    rng = np.random.RandomState(0)
    g = rng.normal(size=1000)
    norm = np.sqrt((g * g).sum())
    clipped = coef64(norm, norm / 2) * g
    assert abs(np.sqrt((clipped * clipped).sum()) - norm / 2) <= 1e-12 * norm
    assert np.array_equal(coef64(norm, 2 * norm) * g, g)
