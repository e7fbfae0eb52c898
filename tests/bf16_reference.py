"""The numerics contract of the opt-in bf16 convolutions ("bf16 inference" and "bf16 training"), as a checker shared by
tests/test_infer_bf16_gpu.py and tests/test_train_bf16_gpu.py. A helper module: it holds no test.

An eligible convolution computes
    y  = epilogue( sum bf16(x) * bf16(w) ),      dx = sum bf16(dy) * bf16(w) (+ add),      dw = sum over pixels bf16(dy) * bf16(x),
operands rounded to nearest-even, accumulated in fp32. The product of two bf16 values is exact in fp32, so a kernel differs from the
same sum in fp64 ON THE ROUNDED OPERANDS only by its fp32 additions:
    |err| <= n * 2^-23 * T + 4 * 2^-24 * |ref|,      T = the same sum over absolute values,
    n = R*S*C (forward), R*S*K (data gradient), N*OH*OW + the number of slices (filter gradient)
(twice the worst case of n fp32 additions, plus the fp32 additions of the epilogue). The bound is derived, not measured: a dropped
tap, a wrong channel or pixel, or truncation instead of RNE on an operand misses it by orders of magnitude. The checkers always
round the very fp32 values the kernel rounds, so no value can fall on the other side of a rounding boundary."""
import numpy as np
import torch
import torch.nn.functional as F


def _r64(t):
    return t.detach().cpu().bfloat16().float().double()


def assert_bound(got, ref, T, n, what, nonzero=True):
    """prints the figures, then asserts the bound -> whether the reference holds anything but zeros"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = n * 2.0 ** -23 * T + 4 * 2.0 ** -24 * ref.abs()
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: n = %d, max |err| = %.3e, max |ref| = %.3e, largest error / bound = %.3e"
          % (what, n, float(err.max()), float(ref.abs().max()), worst))
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), (what, worst)
    assert float(ref.abs().max()) > 0 or not nonzero
    return float(ref.abs().max()) > 0


def conv64(x, w, stride, pad, ohw=None):
    """NHWC x [N][H][W][C], KRSC w (correlation taps, as the device stores them) -> NHWC float64"""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if ohw is not None:
        y = y[:, :ohw[0], :ohw[1]]
    return y.contiguous()


def check_fwd(y, x, w, bias=None, add=None, relu=False, stride=1, pad=0, ohw=None, what=""):
    """y (device result) against fp64 on the operands the kernel really multiplies"""
    xr, wr = _r64(x), _r64(w)
    ref, T = conv64(xr, wr, stride, pad, ohw), conv64(xr.abs(), wr.abs(), stride, pad, ohw)
    if bias is not None:
        ref = ref + bias.detach().cpu().double()
    if add is not None:
        ref = ref + add.detach().cpu().double()
    if relu:
        ref = ref.clamp_min(0.0)
    assert_bound(y, ref, T, w.shape[1] * w.shape[2] * w.shape[3], what)


def dgrad64(dy, w, x_shape, stride, pad):
    N, H, W, C = x_shape
    R = w.shape[1]
    oph, opw = H - ((dy.shape[1] - 1) * stride - 2 * pad + R), W - ((dy.shape[2] - 1) * stride - 2 * pad + R)
    dx = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad, output_padding=(oph, opw))
    return dx.permute(0, 2, 3, 1).contiguous()


def check_dgrad(dx, dy, w, x_shape, add=None, stride=1, pad=0, what="", nonzero=True):
    dyr, wr = _r64(dy), _r64(w)
    ref, T = dgrad64(dyr, wr, x_shape, stride, pad), dgrad64(dyr.abs(), wr.abs(), x_shape, stride, pad)
    if add is not None:
        ref = ref + add.detach().cpu().double()
    return assert_bound(dx, ref, T, w.shape[0] * w.shape[1] * w.shape[2], what, nonzero)


def wgrad64(x, dy, w_shape, stride, pad):
    w0 = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    y = conv64(x, w0, stride, pad)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    y.backward(dy)
    return w0.grad.detach()


def check_wgrad(dw, x, dy, stride=1, pad=0, slices=1, what="", nonzero=True):
    xr, dyr = _r64(x), _r64(dy)
    ref, T = wgrad64(xr, dyr, tuple(dw.shape), stride, pad), wgrad64(xr.abs(), dyr.abs(), tuple(dw.shape), stride, pad)
    return assert_bound(dw, ref, T, dy.shape[0] * dy.shape[1] * dy.shape[2] + slices, what, nonzero)


def draw(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def ties():
    """values exactly halfway between two bf16 neighbours (ties go to the even mantissa), one fp32 ulp either side, both signs"""
    halfway = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]
    vals = []
    for t in halfway:
        t32 = np.float32(t)
        assert float(t32) == t
        vals += [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(4))]
    # the reference itself rounds ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert float(torch.tensor(halfway[0]).bfloat16()) == 1.0 and float(torch.tensor(halfway[1]).bfloat16()) == 1.0 + 2.0 ** -6
    return np.array(vals + [-v for v in vals], dtype=np.float32)
