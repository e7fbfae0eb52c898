"""GPU parity of the individual HIP kernels against plain torch fp32 references of the same op.
(The end-to-end / layer-level parity against the oracle lives in test_parity_gpu.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from igemm_matrix import _TunedTable, _igemm_pass, _igemm_tensors

pytestmark = pytest.mark.gpu


def _nhwc(t):  # NCHW -> NHWC contiguous
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _close(a, b, rtol=1e-3, atol=None):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    if atol is None:
        atol = 1e-4 * float(b.abs().max()) + 1e-7
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), "max err %.3e (tol %.3e), %d/%d bad" % (float(err.max()), float(tol.min()), int(bad.sum()), bad.numel())


CONV_CASES = [
    # N, H, W, C, K, R, stride, pad
    (2, 16, 16, 64, 64, 3, 1, 1),
    (2, 16, 16, 64, 128, 3, 2, 1),
    (2, 16, 16, 128, 256, 1, 2, 0),
    (1, 12, 12, 128, 128, 3, 1, 1),     # M not a multiple of 128
    (2, 8, 8, 256, 96, 1, 1, 0),        # K not a multiple of the N tile
    (3, 24, 24, 32, 160, 3, 1, 1),
    (2, 10, 14, 64, 64, 3, 1, 1),       # non-square
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_dgrad_wgrad(hip, case):
    from denet_amd import ops
    N, H, W, C, K, R, stride, pad = case
    g = torch.Generator(device="cpu").manual_seed(hash(case) & 0xFFFF)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, R, R, generator=g) * 0.1).cuda()
    bias = torch.randn(K, generator=g).cuda()
    x.requires_grad_(True)
    w.requires_grad_(True)
    y_ref = Fn.conv2d(x, w, bias, stride=stride, padding=pad)
    dy = torch.randn(y_ref.shape, generator=g).cuda()
    y_ref.backward(dy)

    xn, wn = _nhwc(x.detach()), w.detach().permute(0, 2, 3, 1).contiguous()
    y = ops.conv_fwd(xn, wn, bias=bias, stride=stride, pad=pad)
    _close(_nchw(y), y_ref)
    dyn = _nhwc(dy)
    dx = ops.conv_dgrad(dyn, wn, tuple(xn.shape), stride=stride, pad=pad)
    _close(_nchw(dx), x.grad)
    dw = ops.conv_wgrad(xn, dyn, tuple(wn.shape), stride=stride, pad=pad)
    _close(dw.permute(0, 3, 1, 2), w.grad)
    # epilogue add
    addt = torch.randn(y.shape, generator=g).cuda()
    y2 = ops.conv_fwd(xn, wn, bias=bias, add=addt, stride=stride, pad=pad)
    _close(y2, y + addt)
    addx = torch.randn(xn.shape, generator=g).cuda()
    dx2 = ops.conv_dgrad(dyn, wn, tuple(xn.shape), add=addx, stride=stride, pad=pad)
    _close(dx2, dx + addx)


@pytest.mark.parametrize("ratio", [0.0, 3.0, 30.0])
def test_conv_epilogue_statistics_with_a_large_channel_offset(hip, ratio):
    """ADVICE r2 / VERDICT r3 item 9: the statistics from the convolution epilogues used to accumulate sum and sum of squares
    of 128-256 values in fp32 before they were widened, and var = E[x^2] - mean^2 cancels: with a channel whose |mean| / std is
    `ratio` the inverse standard deviation carried ~3e-7 x ratio^2 relative error (3e-4 at ratio 30). The implicit-GEMM
    epilogue, the Winograd output transforms and the fused F(4x4) kernel now keep at most 4 values in fp32 (the fused F(2x2)
    kernel 8, the first layer none) and sum in doubles from there (the stand-alone pass sums every element in fp64; the
    reference's cuDNN is two-pass): <= 1e-5 at ratio 30 for all five producers.
    DeNet's own convolution outputs in front of a batch norm have ratios of 0-3 (no bias in front of a BN: resnet.py:60-90)."""
    from denet_amd import ops
    N, H, C, K = 4, 32, 64, 64
    g = torch.Generator(device="cpu").manual_seed(int(ratio))
    x = torch.randn(N, H, H, C, generator=g).cuda()
    w = (torch.randn(K, 3, 3, C, generator=g) * 0.04).cuda()
    gamma, beta = torch.ones(K).cuda(), torch.zeros(K).cuda()
    y0 = ops.conv_fwd(x, w, stride=1, pad=1)
    bias = (float(ratio) * y0.std()).item() * torch.ones(K).cuda()
    with ops.algorithms() as wino:
        worst = 0.0
        for force in (0, 2, 4, 22):
            geom = ops.conv_geom(x.shape, w.shape, 1, 1, None)
            wino.clear()
            wino[(0, geom)] = force
            cache = {"train": True}
            y = ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, cache=cache, bn_stats=True)
            st = cache.get("bn_stats")
            assert st is not None
            rm, rs = torch.zeros(K).cuda(), torch.ones(K).cuda()
            _, _, si = ops.bn_fwd_train(y, gamma, beta, rm, rs, pre=st)
            ref = 1.0 / torch.sqrt(y.double().reshape(-1, K).var(0, unbiased=False) + 1e-5)
            err = float(((si.double() - ref) / ref).abs().max())
            print("ratio %g, algorithm %d: %.2e" % (ratio, force, err))
            worst = max(worst, err)
    # the first layer (7x7 / 2 from the planar batch, the only biased convolution in front of a batch norm: C.B[64,7,2] BN)
    xs = torch.rand(2, 3, 128, 128, generator=g).cuda()
    ws = torch.zeros(64, 7, 8, 4)
    ws[:, :, :7, :3] = torch.randn(64, 7, 7, 3, generator=g) * 0.05
    ws = ws.cuda()
    if ops.conv_stem_ok(xs, tuple(ws.shape), 2, 3, 7):
        y0 = ops.conv_stem_fwd(xs, ws, torch.zeros(64).cuda(), {}, False)
        bias = (float(ratio) * y0.std()).item() * torch.ones(64).cuda()
        cache = {"train": True}
        y = ops.conv_stem_fwd(xs, ws, bias, cache, True)
        _, _, si = ops.bn_fwd_train(y, torch.ones(64).cuda(), torch.zeros(64).cuda(), torch.zeros(64).cuda(), torch.ones(64).cuda(),
                                    pre=cache["bn_stats"])
        ref = 1.0 / torch.sqrt(y.double().reshape(-1, 64).var(0, unbiased=False) + 1e-5)
        err = float(((si.double() - ref) / ref).abs().max())
        print("ratio %g, first layer: %.2e" % (ratio, err))
        worst = max(worst, err)
    print("ratio %g: worst relative error of the inverse standard deviation %.2e" % (ratio, worst))
    assert worst < 1e-5, (ratio, worst)


@pytest.mark.parametrize("case", [(2, 16, 16, 64, 64, 3, 1, 1), (3, 20, 12, 32, 160, 1, 1, 0), (2, 16, 16, 64, 128, 3, 2, 1),
                                  (1, 12, 12, 128, 128, 3, 1, 1), (2, 24, 24, 64, 96, 3, 1, 1)])
def test_conv_epilogue_batch_norm_sums(hip, case):
    """the convolution's epilogue (direct kernel and Winograd output transform) also writes the per-channel sum / sum of squares
    of its output - the statistics of the batch norm behind it (denet/layer/batch_norm.py:50-53) - and bn_fwd_train(pre=...)
    normalises with them: same result as the stand-alone statistics pass"""
    from denet_amd import ops
    N, H, W, C, K, R, stride, pad = case
    g = torch.Generator(device="cpu").manual_seed(sum(case))
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, R, R, C, generator=g) * 0.1).cuda()
    bias = torch.randn(K, generator=g).cuda()
    OH = (H + 2 * pad - R) // stride + 1
    addt = torch.randn(N, OH, OH if H == W else (W + 2 * pad - R) // stride + 1, K, generator=g).cuda()
    gamma, beta = torch.rand(K, generator=g).cuda() + 0.5, torch.randn(K, generator=g).cuda()
    with ops.algorithms() as wino:
        for force_wino in (0, 2, 4):
            geom = ops.conv_geom(x.shape, w.shape, stride, pad, None)
            if force_wino and not ops.conv_wino_ok(geom, force_wino):
                continue
            wino.clear()
            wino[(0, geom)] = force_wino
            cache = {"train": True}
            y = ops.conv_fwd(x, w, bias=bias, add=addt, stride=stride, pad=pad, cache=cache, bn_stats=True)
            st = cache.get("bn_stats")
            if force_wino and K // 4 not in (8, 16, 32, 64, 128, 256):
                assert st is None                     # 256 % (K/4) != 0: the batch norm computes its own statistics
                continue
            assert st is not None
            buf, rows = st
            part = buf[:rows * 2 * K].view(rows, 2, K).sum(0)
            yd = y.double().reshape(-1, K)
            torch.testing.assert_close(part[0], yd.sum(0), rtol=1e-5, atol=1e-4)
            torch.testing.assert_close(part[1], (yd * yd).sum(0), rtol=1e-5, atol=1e-4)
            rm, rs = torch.zeros(K).cuda(), torch.ones(K).cuda()
            rm2, rs2 = rm.clone(), rs.clone()
            a, sm, si = ops.bn_fwd_train(y, gamma, beta, rm, rs, relu=True, pre=st)
            b, sm2, si2 = ops.bn_fwd_train(y, gamma, beta, rm2, rs2, relu=True)
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(sm, sm2, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(si, si2, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(rs, rs2, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", [(1, 16, 16, 64), (2, 32, 48, 64), (1, 16, 32, 128), (5, 128, 128, 64), (3, 128, 64, 128), (14, 128, 128, 64),
                                  (2, 56, 56, 64), (3, 24, 40, 128), (1, 2, 6, 64)])
def test_fused_winograd_f2_kernel(hip, case):
    """csrc/wino2f.hip through ops (algorithm ops.FUSED2) against an fp64 convolution: forward with bias / add / ReLU / the
    batch-norm sums, and the data gradient with the accumulated add. (5,128,128,64) = 320 work items on 256 persistent
    workgroups (uneven loop), (3,128,64,128) = two output-channel chunks per block, (14,128,128,64) = 3-4 items per workgroup
    (every LDS band refilled several times); (2,56,56), (3,24,40), (1,2,6): maps that are no multiple of the 16x16 block. F(2x2) in fp32: <= 1e-6 max-norm."""
    import torch.nn.functional as Fn
    from denet_amd import ops
    N, H, W, Co = case
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, H, W, 64, generator=gen).cuda()
    w = (torch.randn(Co, 3, 3, 64, generator=gen) * (2.0 / 576) ** 0.5).cuda()
    bias = torch.randn(Co, generator=gen).cuda()
    addt = torch.randn(N, H, W, Co, generator=gen).cuda()
    g = ops.conv_geom(x.shape, w.shape, 1, 1, None)
    assert ops.conv_wino2f_ok(0, g) and ops.conv_wino2f_ok(1, g) == (Co == 64)
    with ops.algorithms(table={(0, g): ops.FUSED2, (1, g): ops.FUSED2 if Co == 64 else 0}) as wino:
        xd, wd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True), w.double().permute(0, 3, 1, 2)
        ref = Fn.conv2d(xd, wd, None, padding=1)
        r = ref.detach().permute(0, 2, 3, 1)
        s = float(r.abs().max())
        y = ops.conv_fwd(x, w, stride=1, pad=1)
        assert float((y.double() - r).abs().max()) / s <= 1e-6
        cache = {"train": True}
        y2 = ops.conv_fwd(x, w, bias=bias, add=addt, stride=1, pad=1, cache=cache, bn_stats=True)
        assert cache["fwd_tile"] == ops.FUSED2
        r2 = r + bias.double() + addt.double()
        assert float((y2.double() - r2).abs().max()) / float(r2.abs().max()) <= 1e-6
        buf, rows = cache["bn_stats"]
        blocks = N * ((H + 15) // 16) * ((W + 15) // 16)
        assert rows == (min(blocks, torch.cuda.get_device_properties(0).multi_processor_count) if Co == 64 else blocks)
        part = buf[:rows * 2 * Co].view(rows, 2, Co).sum(0)
        rr = r2.reshape(-1, Co)
        assert float((part[0] - rr.sum(0)).abs().max() / rr.abs().sum(0).max()) <= 1e-6
        assert float((part[1] - (rr * rr).sum(0)).abs().max() / (rr * rr).sum(0).max()) <= 1e-6
        y3 = ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, relu=True)
        assert float((y3.double() - (r + bias.double()).clamp_min(0)).abs().max()) / s <= 1e-6
        if Co == 64:
            dy = torch.randn(N, H, W, 64, generator=gen).cuda()
            acc0 = torch.randn(N, H, W, 64, generator=gen).cuda()
            rdx = torch.autograd.grad(ref, xd, dy.double().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1) + acc0.double()
            dx = ops.conv_dgrad(dy, w, tuple(x.shape), add=acc0, stride=1, pad=1)
            assert float((dx.double() - rdx).abs().max()) / float(rdx.abs().max()) <= 1e-6
            # the filter gradient, fused the same way (64 -> 64 only): sums over all N * H * W / 4 tiles
            assert ops.conv_wino2f_ok(2, g)
            wino[(2, g)] = ops.FUSED2
            wd2 = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            rdw = torch.autograd.grad(Fn.conv2d(xd.detach(), wd2, None, padding=1), wd2, dy.double().permute(0, 3, 1, 2))[0]
            rdw = rdw.permute(0, 2, 3, 1)
            dw = ops.conv_wgrad(x, dy, tuple(w.shape), stride=1, pad=1)
            assert float((dw.double() - rdw).abs().max()) / float(rdw.abs().max()) <= 2e-6
            dw2 = ops.conv_wgrad(x, dy, tuple(w.shape), stride=1, pad=1)
            assert torch.equal(dw, dw2)                                   # partial sums are added in a fixed order
        else:
            assert not ops.conv_wino2f_ok(2, g)


@pytest.mark.parametrize("case", [(1, 8, 32, 64, 64), (2, 16, 64, 64, 64), (3, 12, 20, 64, 64), (2, 24, 40, 32, 128), (1, 16, 32, 128, 64),
                                  (5, 64, 64, 64, 64), (2, 56, 56, 64, 64), (1, 4, 4, 32, 64),
                                  # the channel counts of the tuned file's mode-3 (inference) entries: (C, K) = (128, 128), (256, 128),
                                  # (256, 256), (512, 256), on maps that are no multiple of the 8 x 32-pixel block
                                  (1, 20, 36, 128, 128), (2, 12, 20, 256, 128), (2, 20, 44, 256, 256), (1, 8, 36, 512, 256)])
def test_fused_winograd_f4_tile_parallel_kernel(hip, case):
    """csrc/wino4t.hip through ops (algorithm ops.FUSED4: input transform, 36 products, output transform in one launch) against an
    fp64 convolution: forward plain / with bias + add + batch-norm sums / with ReLU, and the data gradient with the accumulated add
    and with the backward sums of a batch norm (both mask forms). (3,12,20) and (2,56,56): maps that are no multiple of the
    8 x 32-pixel block (tiles masked, halo zero-filled); (2,24,40,32,128): two reduction chunks, two channel blocks; (1,16,32,128,64):
    eight chunks; (1,4,4,32,64): one tile; the last four: the reduction / written channel counts of the mode-3 entries of the tuned
    file (up to 32 reduction chunks, up to four channel blocks), with the epilogue the inference fold runs (bias + residual add +
    ReLU in one call) in both inference forms. F(4x4) in fp32: <= 2.5e-5 max-norm measured at the benchmark sizes, 8e-5 asserted
    like the other F(4x4) passes (tests/test_conv_fullsize_gpu.py)."""
    import torch.nn.functional as Fn
    from denet_amd import ops
    N, H, W, C, K = case
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, H, W, C, generator=gen).cuda()
    w = (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda()
    bias = torch.randn(K, generator=gen).cuda()
    addt = torch.randn(N, H, W, K, generator=gen).cuda()
    g = ops.conv_geom(x.shape, w.shape, 1, 1, None)
    assert ops.conv_wino4t_ok(0, g) and ops.conv_wino4t_ok(1, g) == (C % 64 == 0 and K % 16 == 0)
    BOUND = 8e-5
    with ops.algorithms(table={(0, g): ops.FUSED4}) as wino:
        xd, wd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True), w.double().permute(0, 3, 1, 2)
        ref = Fn.conv2d(xd, wd, None, padding=1)
        r = ref.detach().permute(0, 2, 3, 1)
        s = float(r.abs().max())
        y = ops.conv_fwd(x, w, stride=1, pad=1)
        assert float((y.double() - r).abs().max()) / s <= BOUND
        cache = {"train": True}
        y2 = ops.conv_fwd(x, w, bias=bias, add=addt, stride=1, pad=1, cache=cache, bn_stats=True)
        assert cache["fwd_tile"] == ops.FUSED4
        r2 = r + bias.double() + addt.double()
        assert float((y2.double() - r2).abs().max()) / float(r2.abs().max()) <= BOUND
        buf, rows = cache["bn_stats"]
        assert rows == N * ((H + 7) // 8) * ((W + 31) // 32)
        part = buf[:rows * 2 * K].view(rows, 2, K).sum(0)
        yy = y2.double().reshape(-1, K)                    # the sums are those of what was STORED
        assert float((part[0] - yy.sum(0)).abs().max() / yy.abs().sum(0).max()) <= 1e-6
        assert float((part[1] - (yy * yy).sum(0)).abs().max() / (yy * yy).sum(0).max()) <= 1e-6
        y3 = ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, relu=True)
        assert float((y3.double() - (r + bias.double()).clamp_min(0)).abs().max()) / s <= BOUND
        # the inference form: a layer cache without "train" keeps the packed filters per weights version (twice: the cached ones)
        icache = {}
        for _ in range(2):
            y4 = ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, relu=True, cache=icache)
            assert torch.equal(y4, y3) and icache["fwd_tile"] == ops.FUSED4
        # the epilogue of a folded residual block's last convolution (layer/resnet.py: forward_folded(add=res, relu=True)):
        # bias + residual add + ReLU in one call
        r6 = r2.clamp_min(0)
        y6 = ops.conv_fwd(x, w, bias=bias, add=addt, stride=1, pad=1, relu=True, cache=icache)
        assert icache["fwd_tile"] == ops.FUSED4
        assert float((y6.double() - r6).abs().max()) / float(r6.abs().max()) <= BOUND
        assert bool((y6 >= 0).all()) and bool((y6 == 0).any())
        # ... and a mode-3 entry of the tuned file overrides the training decision for the inference forward pass only
        wino[(0, g)] = 0
        wino[(3, g)] = ops.FUSED4
        icache = {}
        y5 = ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, relu=True, cache=icache)
        assert torch.equal(y5, y3) and icache["fwd_tile"] == ops.FUSED4
        y7 = ops.conv_fwd(x, w, bias=bias, add=addt, stride=1, pad=1, relu=True, cache=icache)
        assert icache["fwd_tile"] == ops.FUSED4 and torch.equal(y7, y6)
        assert float((y7.double() - r6).abs().max()) / float(r6.abs().max()) <= BOUND
        tcache = {"train": True}
        ops.conv_fwd(x, w, bias=bias, stride=1, pad=1, relu=True, cache=tcache)
        assert tcache["fwd_tile"] == 0
        wino[(0, g)] = ops.FUSED4
        del wino[(3, g)]
        if ops.conv_wino4t_ok(1, g):
            wino[(1, g)] = ops.FUSED4
            dy = torch.randn(N, H, W, K, generator=gen).cuda()
            acc0 = torch.randn(N, H, W, C, generator=gen).cuda()
            rdx = torch.autograd.grad(ref, xd, dy.double().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1) + acc0.double()
            cache = {"train": True}
            dx = ops.conv_dgrad(dy, w, tuple(x.shape), add=acc0, stride=1, pad=1, cache=cache)
            assert cache["dgrad_tile"] == ops.FUSED4
            assert float((dx.double() - rdx).abs().max()) / float(rdx.abs().max()) <= BOUND
            # the backward sums of the batch norm whose output gradient dx is: sum(g), sum(g * xhat), g = dx masked by the ReLU
            xb = torch.randn(N, H, W, C, generator=gen).cuda()
            gam, bet = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
            mu = xb.reshape(-1, C).mean(0)
            isd = 1.0 / (xb.reshape(-1, C).var(0, unbiased=False) + 1e-5).sqrt()
            yb = torch.relu((xb - mu) * isd * gam + bet)
            for with_y in (True, False):
                bsum = ops.BnSums(xb, yb if with_y else None, gam, bet, mu, isd, True)
                dx2 = ops.conv_dgrad(dy, w, tuple(x.shape), add=acc0, stride=1, pad=1, cache={"train": True}, sums=bsum)
                assert torch.equal(dx2, dx)
                assert bsum.partial is not None, "the pass did not write the backward sums"
                sb, srows = bsum.partial[:2]
                s2 = sb[:srows * 2 * C].view(srows, 2, C).sum(0)
                yv = torch.relu(torch.addcmul(bet - mu * (gam * isd), xb, gam * isd)) if not with_y else yb
                gq = torch.where(yv > 0, dx, torch.zeros_like(dx)).double().reshape(-1, C)
                xh = ((xb - mu) * isd).double().reshape(-1, C)
                assert float((s2[0] - gq.sum(0)).abs().max() / gq.abs().sum(0).max()) <= 1e-6
                assert float((s2[1] - (gq * xh).sum(0)).abs().max() / (gq * xh).abs().sum(0).max()) <= 1e-6


@pytest.mark.parametrize("case", [(2, 16, 16, 64, 64), (3, 32, 48, 64, 128), (2, 20, 12, 128, 64), (1, 64, 64, 128, 256), (2, 2, 2, 64, 64),
                                  (1, 34, 18, 64, 192)])
def test_stride2_data_gradient_with_the_parity_classes_in_one_workgroup(hip, case):
    """csrc/dgrad_s2.hip through ops.conv_dgrad (3x3 stride 2 pad 1) against fp64 autograd and against the implicit-GEMM kernel
    (DENET_DGRAD_S2 = 0): plain, with the accumulated add, with the backward sums of a batch norm (both ReLU-mask forms).
    (2,20,12), (1,34,18): output maps that are no multiple of the 8 x 8-position block (positions masked, the dy halo beyond the map
    zero-filled); (3,32,48,64,128) / (1,64,64,128,256): two / four reduction chunks; (1,34,18,64,192): three; (2,2,2): one position.
    Exact fp32 FMA chains: <= 1e-5 max-norm like the direct kernels."""
    import torch.nn.functional as Fn
    from denet_amd import ops
    N, H, W, C, K = case
    gen = torch.Generator().manual_seed(sum(case))
    w = (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda()
    dy = torch.randn(N, H // 2, W // 2, K, generator=gen).cuda()
    acc0 = torch.randn(N, H, W, C, generator=gen).cuda()
    xd = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    y = Fn.conv2d(xd, w.double().cpu().permute(0, 3, 1, 2), None, stride=2, padding=1)
    ref = torch.autograd.grad(y, xd, dy.double().cpu().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1).cuda()
    g = ops.conv_geom((N, H, W, C), w.shape, 2, 1, None)
    with ops.algorithms(DGRAD_S2=True):
        cache = {"train": True}
        with ops.LaunchTrace() as lt:
            dx = ops.conv_dgrad(dy, w, (N, H, W, C), stride=2, pad=1, cache=cache)
        assert cache.get("dgrad_s2") and any(n.startswith("dgrad_s2_kernel") for n in lt.symbols), lt.symbols
        assert float((dx.double() - ref).abs().max() / ref.abs().max()) <= 1e-5
        dx1 = ops.conv_dgrad(dy, w, (N, H, W, C), add=acc0, stride=2, pad=1)
        r1 = ref + acc0.double()
        assert float((dx1.double() - r1).abs().max() / r1.abs().max()) <= 1e-5
        with ops.switches(DGRAD_S2=False):
            dxi = ops.conv_dgrad(dy, w, (N, H, W, C), add=acc0, stride=2, pad=1)
        assert float((dx1 - dxi).abs().max() / dxi.abs().max()) <= 5e-6
        xb = torch.randn(N, H, W, C, generator=gen).cuda()
        gam, bet = (torch.rand(C, generator=gen) + 0.5).cuda(), torch.randn(C, generator=gen).cuda()
        mu = xb.reshape(-1, C).mean(0)
        isd = 1.0 / (xb.reshape(-1, C).var(0, unbiased=False) + 1e-5).sqrt()
        yb = torch.relu((xb - mu) * isd * gam + bet)
        for with_y in (True, False):
            bsum = ops.BnSums(xb, yb if with_y else None, gam, bet, mu, isd, True)
            dx2 = ops.conv_dgrad(dy, w, (N, H, W, C), add=acc0, stride=2, pad=1, cache={"train": True}, sums=bsum)
            assert torch.equal(dx2, dx1)
            assert bsum.partial is not None
            sb, rows = bsum.partial[:2]
            assert rows == N * ((H // 2 + 7) // 8) * ((W // 2 + 7) // 8)
            s2 = sb[:rows * 2 * C].view(rows, 2, C).sum(0)
            yv = yb if with_y else torch.relu(torch.addcmul(bet - mu * (gam * isd), xb, gam * isd))
            gq = torch.where(yv > 0, dx1, torch.zeros_like(dx1)).double().reshape(-1, C)
            xh = ((xb - mu) * isd).double().reshape(-1, C)
            assert float((s2[0] - gq.sum(0)).abs().max() / gq.abs().sum(0).max()) <= 1e-6
            assert float((s2[1] - (gq * xh).sum(0)).abs().max() / (gq * xh).abs().sum(0).max()) <= 1e-6


@pytest.mark.parametrize("case", [(2, 24, 24, 1536, 1024), (1, 24, 24, 768, 512), (3, 8, 12, 512, 128)])
def test_opt_in_bf16_split_head_gemms(hip, case):
    """OPT-IN ops.HEAD_BF16X3 (csrc/gemm3b.hip): the head's 1x1 convolutions as 3-term bf16-split GEMMs - forward, data gradient
    (w transposed) and filter gradient (dy, x transposed; contraction over the pixels) against fp64. Not the exact fp32 chain:
    the bound is 2e-5 max-norm (measured 2-4e-6; the exact fp32 kernels give 1-2.5e-6), far inside the 1e-3 activation budget."""
    from denet_amd import ops
    N, H, W, C, K = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, H, W, C, generator=g).cuda()
    w = (torch.randn(K, 1, 1, C, generator=g) * (2.0 / C) ** 0.5).cuda()
    bias = torch.randn(K, generator=g).cuda()
    dy = torch.randn(N, H, W, K, generator=g).cuda()
    x2, w2, dy2 = x.double().reshape(-1, C), w.double().reshape(K, C), dy.double().reshape(-1, K)
    ref = {"y": x2 @ w2.T + bias.double(), "dx": dy2 @ w2, "dw": dy2.T @ x2}
    got = {}
    for flag in (False, True):
        with ops.switches(HEAD_BF16X3=flag):
            got[flag] = {"y": ops.conv_fwd(x, w, bias=bias).reshape(-1, K), "dx": ops.conv_dgrad(dy, w, tuple(x.shape)).reshape(-1, C),
                         "dw": ops.conv_wgrad(x, dy, tuple(w.shape)).reshape(K, C)}
    for k, r in ref.items():
        s = float(r.abs().max())
        e_exact = float((got[False][k].double() - r).abs().max()) / s
        e_split = float((got[True][k].double() - r).abs().max()) / s
        assert e_exact <= 5e-6 and e_split <= 2e-5, (k, e_exact, e_split)
        assert not torch.equal(got[False][k], got[True][k])           # the flag really switches the arithmetic


@pytest.mark.parametrize("case", [(3, 20, 20, 128, 64), (2, 24, 36, 128, 192), (5, 16, 28, 256, 128), (1, 64, 64, 128, 128), (9, 32, 32, 256, 64), (3, 20, 28, 64, 256)])
@pytest.mark.parametrize("tb", [64, 32, 33, 34])
def test_fused_winograd_f4_kernel(hip, case, tb):
    """csrc/wino4f.hip (F(4x4,3x3) component products + output transform in one kernel; convolution.py:80-83 and its data
    gradient, model_cnn.py:318) forced on through denet_conv_wino4f_mode, all four shapes (64-tile blocks; 32-tile blocks as one 8-wave workgroup,
    as 4-wave workgroups on 64 channels - mode 33 - or on 32 channels - mode 34), against an fp64 convolution and
    against the un-fused passes: tile counts that are no multiple of the block (75, 108, 140 tiles: workgroups with rows beyond
    the tensor), 64 / 128 / 192 output channels, 2 and 4 reduction chunks per component; all three epilogues - plain, bias + add +
    the batch-norm column sums of what is stored, ReLU, and the backward sums of the batch norm whose output gradient the data
    gradient writes (mask from y, mask recomputed from x, no mask). The reduction width must be a multiple of 128: cases with 64
    (or 192) channels on one side run that pass un-fused, the other fused."""
    import torch.nn.functional as Fn
    from denet_amd import ops
    N, H, W, C, K = case
    L = ops._L()
    gen = torch.Generator().manual_seed(sum(case) + tb)
    x = torch.randn(N, H, W, C, generator=gen).cuda()
    w = (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda()
    bias = torch.randn(K, generator=gen).cuda()
    addt = torch.randn(N, H, W, K, generator=gen).cuda()
    dy = torch.randn(N, H, W, K, generator=gen).cuda()
    acc0 = torch.randn(N, H, W, C, generator=gen).cuda()
    xd, wd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True), w.double().permute(0, 3, 1, 2)
    ref = Fn.conv2d(xd, wd, None, padding=1)
    r = ref.detach().permute(0, 2, 3, 1)
    rdx = torch.autograd.grad(ref, xd, dy.double().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    u, ud = ops.conv_wino_filter(w, 4, dgrad=False), ops.conv_wino_filter(w, 4, dgrad=True)
    T = N * (H // 4) * (W // 4)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max())

    def sums_of(sums):
        buf, rows = sums.partial
        return buf[:rows * 2 * C].view(rows, 2, C).sum(0).clone()

    # backward sums: dx is the gradient of the output of a batch norm with input xb (and output yb)
    xb = torch.randn(N, H, W, C, generator=gen).cuda()
    gamma, beta = torch.rand(C, generator=gen).cuda() + 0.5, torch.randn(C, generator=gen).cuda() * 0.3
    mean, invstd = xb.reshape(-1, C).mean(0), 1.0 / xb.reshape(-1, C).std(0)
    yb = torch.relu((xb - mean) * invstd * gamma + beta)
    res = {}
    try:
        for mode in (0, tb):
            L.denet_conv_wino4f_mode(mode)
            cache = {}
            st = torch.zeros(1 << 20, dtype=torch.float64, device="cuda")
            y = ops.conv_wino_fwd(x, w, bias, addt, tile=4, u=u, stats=(st, cache))
            if cache["bn_stats"] is None:
                assert mode == 0 and 256 % (K // 4) != 0              # the un-fused output transform cannot at this channel count
                part = None
            else:
                stt, rows = cache["bn_stats"]
                if mode and C % 128 == 0:
                    assert rows == (T + (64 if tb == 64 else 32) - 1) // (64 if tb == 64 else 32)                  # one row of partial sums per tile block
                part = stt[:rows * 2 * K].view(rows, 2, K).sum(0).clone()
            y_plain = ops.conv_wino_fwd(x, w, tile=4, u=u)
            y_relu = ops.conv_wino_fwd(x, w, bias, tile=4, u=u, relu=True)
            dx = ops.conv_wino_dgrad(dy, w, add=acc0, tile=4, u=ud)
            bs = []
            for relu_, use_y in ((True, True), (True, False), (False, False)):
                sums = ops.BnSums(xb, yb if use_y else None, gamma, beta, mean, invstd, relu_)
                dxs = ops.conv_wino_dgrad(dy, w, tile=4, u=ud, sums=sums, cache={})
                assert sums.partial is not None
                bs.append((dxs.clone(), sums_of(sums)))
            res[mode] = (y.clone(), part, y_plain.clone(), y_relu.clone(), dx.clone(), bs)
    finally:
        L.denet_conv_wino4f_mode(-1)
    y0, part0, yp0, yr0, dx0, bs0 = res[0]
    y1, part1, yp1, yr1, dx1, bs1 = res[tb]
    r2 = r + bias.double() + addt.double()
    assert rel(yp1, r) <= 3e-5 and rel(y1, r2) <= 3e-5 and rel(yr1, (r + bias.double()).clamp_min(0)) <= 3e-5
    assert rel(dx1, rdx + acc0.double()) <= 3e-5
    assert rel(y1, y0) <= 3e-5 and rel(dx1, dx0) <= 3e-5            # (the un-fused passes: another association of the same sums)
    rr = r2.reshape(-1, K)
    assert float((part1[0] - rr.sum(0)).abs().max() / rr.abs().sum(0).max()) <= 2e-5
    assert float((part1[1] - (rr * rr).sum(0)).abs().max() / (rr * rr).sum(0).max()) <= 2e-5
    for (dxa, sa), (dxb, sb), (relu_, use_y) in zip(bs0, bs1, ((True, True), (True, False), (False, False))):
        assert rel(dxb, rdx) <= 3e-5 and rel(dxb, dxa) <= 3e-5
        g = rdx if not relu_ else torch.where(yb.double() > 0, rdx, torch.zeros_like(rdx))
        xhat = ((xb - mean) * invstd).double()
        want = torch.stack([g.reshape(-1, C).sum(0), (g * xhat).reshape(-1, C).sum(0)])
        scale = float(g.abs().reshape(-1, C).sum(0).max())
        assert float((sb - want).abs().max()) / scale <= 5e-5, (relu_, use_y)
        assert float((sb - sa).abs().max()) / scale <= 5e-5, (relu_, use_y)


def test_fused_winograd_f4_kernel_under_memory_pressure(hip):
    """the chunk pipeline of csrc/wino4f.hip (LDS-DMA four chunks deep, one barrier per chunk that publishes chunk s+1 and frees
    the buffer of chunk s-1) against stretched memory latencies: a second stream saturates HBM while the fused kernel runs; same
    results as alone, run to run bit-identical"""
    from denet_amd import ops
    ops.init_streams()
    L = ops._L()
    side = torch.cuda.Stream()
    big_a = torch.empty(1 << 27, device="cuda")
    big_b = torch.empty(1 << 27, device="cuda")
    gen = torch.Generator().manual_seed(11)
    try:
        for it, (N, H, W, C, K, tb) in enumerate([(16, 64, 64, 128, 128, 64), (16, 32, 32, 256, 256, 32), (8, 64, 64, 256, 128, 33), (7, 36, 52, 128, 64, 32), (16, 64, 64, 128, 128, 33), (16, 32, 32, 256, 256, 34), (9, 64, 64, 128, 192, 34)]):
            x = torch.randn(N, H, W, C, generator=gen).cuda()
            w = (torch.randn(K, 3, 3, C, generator=gen) * 0.03).cuda()
            u = ops.conv_wino_filter(w, 4, dgrad=False)
            L.denet_conv_wino4f_mode(tb)
            alone = ops.conv_wino_fwd(x, w, tile=4, u=u).clone()
            torch.cuda.synchronize()
            for rep in range(3):
                with torch.cuda.stream(side):
                    for _ in range(8):
                        big_b.copy_(big_a, non_blocking=True)
                y = ops.conv_wino_fwd(x, w, tile=4, u=u)
                torch.cuda.synchronize()
                assert torch.equal(y, alone), (it, rep)
            L.denet_conv_wino4f_mode(0)
            ref = ops.conv_wino_fwd(x, w, tile=4, u=u)
            assert float((alone - ref).abs().max() / ref.abs().max()) < 3e-5
    finally:
        L.denet_conv_wino4f_mode(-1)


@pytest.mark.parametrize("case", [(3, 20, 20, 128, 128), (2, 24, 36, 128, 256), (5, 16, 28, 256, 128), (8, 64, 64, 128, 128), (16, 32, 32, 256, 256),
                                  (1, 8, 8, 128, 128), (7, 16, 16, 512, 256), (4, 12, 20, 64, 128)])
def test_winograd_f4_filter_gradient_kernel(hip, case):
    """csrc/wino4g.hip (F(4x4,3x3) filter-gradient component products on the contraction-major operands; tensor.grad of
    convolution.py:80-83 with respect to the filters, model_cnn.py:318) against an fp64 filter gradient and against the generic
    batched split-K path: tile counts that are no multiple of the 16-tile chunk or of the slice (75, 108, 140 tiles), one to
    sixteen slices, 128 x 128 ... 512 x 256 blocks, a 4-tile problem that stays on the generic path, 64 channels (generic path);
    run to run bit-identical (the slices are added in slice order)."""
    import torch.nn.functional as Fn
    from denet_amd import ops
    N, H, W, C, K = case
    L = ops._L()
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, H, W, C, generator=gen).cuda()
    dy = torch.randn(N, H, W, K, generator=gen).cuda()
    xd = x.double().permute(0, 3, 1, 2).contiguous()
    wd = torch.zeros(K, C, 3, 3, dtype=torch.float64, device="cuda", requires_grad=True)
    ref = torch.autograd.grad(Fn.conv2d(xd, wd, None, padding=1), wd, dy.double().permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    res = {}
    try:
        for mode in (0, 1):
            L.denet_conv_wino4g_mode(mode)
            a = ops.conv_wino_wgrad(x, dy, tile=4).clone()
            b = ops.conv_wino_wgrad(x, dy, tile=4).clone()
            assert torch.equal(a, b), "not reproducible run to run"
            res[mode] = a
    finally:
        L.denet_conv_wino4g_mode(-1)
    s = float(ref.abs().max())
    for mode in (0, 1):
        assert float((res[mode].double() - ref).abs().max()) / s <= 5e-5, mode
    assert float((res[1] - res[0]).abs().max()) / s <= 5e-5
    T = N * (H // 4) * (W // 4)
    if C % 128 or K % 128 or T < 64:
        assert torch.equal(res[0], res[1])                # the generic path either way


def test_fused_winograd_f2_kernels_under_memory_pressure(hip):
    """the LDS refill protocol of csrc/wino2f.hip (row bands streamed in by LDS-DMA while the previous item is multiplied, waits
    that leave younger pieces in flight) against stretched memory latencies: random batch / image sizes with several work items
    per workgroup, a second stream saturating HBM meanwhile; every pass against the direct implicit-GEMM kernel"""
    import random
    from denet_amd import ops
    ops.init_streams()
    rng = random.Random(5)
    side = torch.cuda.Stream()
    big_a = torch.empty(1 << 27, device="cuda")
    big_b = torch.empty(1 << 27, device="cuda")
    with ops.algorithms(AUTOTUNE=False) as wino:
        for it in range(24):
            N, H, W = rng.choice([8, 9, 17, 24, 40]), rng.choice([64, 96, 128]), rng.choice([64, 128, 144])
            g = torch.Generator().manual_seed(it)
            x = torch.randn(N, H, W, 64, generator=g).cuda()
            dy = torch.randn(N, H, W, 64, generator=g).cuda()
            w = (torch.randn(64, 3, 3, 64, generator=g) * 0.06).cuda()
            geom = ops.conv_geom(x.shape, w.shape, 1, 1, None)
            res = {}
            for algo in (0, ops.FUSED2):
                for mode in range(3):
                    wino[(mode, geom)] = algo
                if algo and it % 2:
                    with torch.cuda.stream(side):
                        for _ in range(6):
                            big_b.copy_(big_a, non_blocking=True)
                res[algo] = (ops.conv_fwd(x, w, stride=1, pad=1), ops.conv_dgrad(dy, w, tuple(x.shape), stride=1, pad=1),
                             ops.conv_wgrad(x, dy, tuple(w.shape), stride=1, pad=1))
            torch.cuda.synchronize()
            for k in range(3):
                a, b = res[0][k], res[ops.FUSED2][k]
                assert float((a - b).abs().max() / a.abs().max()) < 1e-5, (it, N, H, W, k)


@pytest.mark.parametrize("case", [(2, 32, 32, 64, 3, 2, 1), (3, 17, 23, 32, 3, 2, 1), (2, 16, 16, 128, 2, 2, 0), (1, 15, 15, 32, 3, 1, 1),
                                  (3, 20, 36, 96, 3, 2, 1), (1, 2, 2, 32, 3, 2, 1)])
def test_bn_relu_pool_fused_equals_separate_passes(hip, case):
    """BN + ReLU + max pool in one pass (bn.hip: denet_bn_relu_pool_fwd_train / _bwd; batch_norm_relu.py:34-54 -> pool.py:38)
    against bn_fwd_train(relu) + maxpool_fwd and maxpool_bwd + bn_bwd: bit-identical output, argmax taps (ties between the
    many zeros behind the ReLU included), statistics, dx, dgamma, dbeta. Even maps under the 3x3 / 2 / 1 pool take the 2 x 2-pixel
    form of the backward pointwise pass (bn_bwd_apply_pool_quad_kernel), the others the general one"""
    from denet_amd import ops
    N, H, W, C, k, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, H, W, C, generator=g).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.5).cuda()
    rm, rs = torch.zeros(C).cuda(), torch.ones(C).cuda()
    rm2, rs2 = rm.clone(), rs.clone()
    y, sm, si = ops.bn_fwd_train(x, gamma, beta, rm, rs, relu=True)
    yp, arg = ops.maxpool_fwd(y, k, s, p)
    yp2, arg2, sm2, si2 = ops.bn_relu_pool_fwd_train(x, gamma, beta, rm2, rs2, k, s, p)
    assert torch.equal(yp, yp2) and torch.equal(arg, arg2)
    assert torch.equal(sm, sm2) and torch.equal(si, si2) and torch.equal(rm, rm2) and torch.equal(rs, rs2)
    dyp = torch.randn(*yp.shape, generator=g).cuda()
    dy = ops.maxpool_bwd(dyp, arg, tuple(x.shape), k, s, p)
    dx, _, dg, db = ops.bn_bwd(x, None, dy, gamma, sm, si, relu=True, beta=beta)
    dx2, dg2, db2 = ops.bn_relu_pool_bwd(x, dyp, arg2, gamma, beta, sm2, si2, k, s, p)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    # the backward reductions over the POOLED tensors (a window sends its gradient to its argmax pixel, whose ReLU output is the
    # pooled value): the same sums in another order of a double-precision summation, from a pass over a quarter of the elements -
    # or from partial sums somebody else left behind (here: the generic reduction kernel on the pooled tensors)
    rm3, rs3 = torch.zeros(C).cuda(), torch.ones(C).cuda()
    yp3, arg3, sm3, si3, xh = ops.bn_relu_pool_fwd_train(x, gamma, beta, rm3, rs3, k, s, p, xhat=True)
    assert torch.equal(yp3, yp) and torch.equal(arg3, arg) and torch.equal(sm3, sm)
    dg3, db3 = torch.empty(C).cuda(), torch.empty(C).cuda()
    dx3 = ops.bn_relu_pool_bwd_pooled(x, xh, yp3, dyp, arg3, gamma, beta, sm3, si3, k, s, p, dg3, db3)
    torch.testing.assert_close(dg3, dg, rtol=2e-6, atol=2e-6 * float(dg.abs().max()))
    torch.testing.assert_close(db3, db, rtol=2e-6, atol=2e-6 * float(db.abs().max()))
    torch.testing.assert_close(dx3, dx, rtol=1e-5, atol=1e-6 * float(dx.abs().max()))


def test_conv_stem_small_c(hip):
    """7x7/2 stem: C=3 padded to 4, S padded 7->8 (zero tap); wgrad must leave the padded tap at 0."""
    from denet_amd import ops
    g = torch.Generator().manual_seed(5)
    N, H, W, K = 2, 32, 32, 64
    x = torch.rand(N, 3, H, W, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(K, 3, 7, 7, generator=g) * 0.1).cuda().requires_grad_(True)
    bias = torch.randn(K, generator=g).cuda()
    y_ref = Fn.conv2d(x, w, bias, stride=2, padding=3)
    dy = torch.randn(y_ref.shape, generator=g).cuda()
    y_ref.backward(dy)
    xn = ops.nchw_to_nhwc(x.detach().contiguous(), 4)
    wn = torch.zeros(K, 7, 8, 4).cuda()
    wn[:, :, :7, :3] = w.detach().permute(0, 2, 3, 1)
    y = ops.conv_fwd(xn, wn, bias=bias, stride=2, pad=3, s_real=7)
    _close(_nchw(y), y_ref)
    dw = ops.conv_wgrad(xn, _nhwc(dy), tuple(wn.shape), stride=2, pad=3, s_real=7)
    _close(dw[:, :, :7, :3].permute(0, 3, 1, 2), w.grad)
    assert float(dw[:, :, 7, :].abs().max()) == 0.0
    assert float(dw[:, :, :, 3].abs().max()) == 0.0


def test_generic_kernels_still_cover_the_first_layer(hip):
    """DENET_STEM=0 (read once per process, hence a process of its own): the implicit-GEMM kernels on the padded 7 x 8 x 4 layout,
    which the first layer ran on before csrc/stem.hip and every other small-channel geometry still does"""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "conv_stem_small_c"],
                       env=dict(os.environ, DENET_STEM="0"), capture_output=True, text=True, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("case", [(3, 48, 272), (1, 18, 130), (2, 224, 224), (5, 512, 512)])
def test_first_layer_kernels(hip, case):
    """the first layer's own kernels (csrc/stem.hip: 147 real taps instead of 7 x 8 x 4 padded ones; blocks of 8 x 64 output pixels,
    here with ragged right / bottom blocks): y, the batch-norm column sums of y, and the filter gradient against fp64; the padded
    filter column / channel of dw stay 0; two runs are bit-identical (fixed summation order over the workgroups)"""
    import ctypes
    from denet_amd import ops
    from denet_amd.lib import load as lib, ptr, check, stream_ptr
    N, H, W = case
    K, OH, OW = 64, H // 2, W // 2
    assert lib().denet_conv_stem_ok(0, N, H, W, 4, K, 7, 8, 7, 2, 3, OH, OW) and lib().denet_conv_stem_ok(1, N, H, W, 4, K, 7, 8, 7, 2, 3, OH, OW)
    g = torch.Generator().manual_seed(H + W)
    x = torch.rand(N, 3, H, W, generator=g).cuda()
    w = (torch.randn(K, 3, 7, 7, generator=g) * 0.1).cuda()
    bias = torch.randn(K, generator=g).cuda()
    dy = torch.randn(N, K, OH, OW, generator=g).cuda()
    xn = ops.nchw_to_nhwc(x.contiguous(), 4)
    xn[..., 3] = 7.0                                  # the padding channel must not matter
    wn = torch.zeros(K, 7, 8, 4).cuda()
    wn[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    wd = w.double().requires_grad_(True)
    y_ref = Fn.conv2d(x.double(), wd, bias.double(), stride=2, padding=3)
    y_ref.backward(dy.double())
    y = torch.empty(N, OH, OW, K, device="cuda")
    st = torch.zeros(4096 * 2 * K, dtype=torch.float64, device="cuda")
    rows = ctypes.c_int(0)
    check(lib().denet_conv_stem_fwd(ptr(xn), ptr(wn), ptr(bias), ptr(y), ptr(st), st.numel() * 8, ctypes.byref(rows), N, H, W,
                                    stream_ptr()), "stem_fwd")
    yr = y_ref.detach().permute(0, 2, 3, 1)
    scale = float(yr.abs().max())
    assert float((y.double() - yr).abs().max()) < 2e-6 * scale
    part = st[:rows.value * 2 * K].view(rows.value, 2, K).sum(0)
    yd = y.double().reshape(-1, K)
    # (a lane adds 32 values in fp32 before the doubles take over)
    torch.testing.assert_close(part[0], yd.sum(0), rtol=1e-6, atol=1e-6 * float(yd.abs().sum(0).max()))
    torch.testing.assert_close(part[1], (yd * yd).sum(0), rtol=1e-6, atol=1e-6)
    # through the generic entry point (which hands this geometry over), without bias / statistics; and with the ReLU of the
    # inference fold in the epilogue
    y2 = ops.conv_fwd(xn, wn, stride=2, pad=3, s_real=7)
    assert torch.equal(y2 + bias, y) or float((y2 + bias - y).abs().max()) < 1e-6 * scale
    y4 = ops.conv_fwd(xn, wn, bias=bias, stride=2, pad=3, s_real=7, relu=True)
    assert torch.equal(y4, y.clamp_min(0))
    dyn = _nhwc(dy)
    ws = torch.empty(lib().denet_conv_stem_wgrad_workspace_bytes() // 4, device="cuda")
    dws = []
    for _ in range(2):
        dw = torch.full((K, 7, 8, 4), 3.0, device="cuda")
        check(lib().denet_conv_stem_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), ws.numel() * 4, N, H, W, stream_ptr()), "stem_wgrad")
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])
    dw = dws[0]
    # the planar image batch (the reference's input layout) read directly: bit-identical to the NHWC route
    assert ops.conv_stem_ok(x, tuple(wn.shape), 2, 3, 7)
    cache = {}
    y3 = ops.conv_stem_fwd(x.contiguous(), wn, bias, cache, True)
    assert torch.equal(y3, y)
    st3, rows3 = cache["bn_stats"]
    assert rows3 == rows.value and torch.equal(st3[:rows3 * 2 * K], st[:rows3 * 2 * K])
    dw3 = ops.conv_stem_wgrad(x.contiguous(), dyn, tuple(wn.shape), torch.empty_like(dw))
    assert torch.equal(dw3, dw)
    ref = wd.grad.permute(0, 2, 3, 1)
    assert float((dw[:, :, :7, :3].double() - ref).abs().max()) < 3e-6 * float(ref.abs().max())
    assert float(dw[:, :, 7, :].abs().max()) == 0.0 and float(dw[:, :, :, 3].abs().max()) == 0.0


def test_conv_is_mfma_exact_order_free(hip):
    """A = I check with an asymmetric filter (catches transposed fragments)."""
    from denet_amd import ops
    C = K = 64
    x = torch.zeros(1, 8, 16, C).cuda()
    for c in range(C):
        x[0, c % 8, c % 16, c] = 1.0 + c
    w = torch.arange(K * C, dtype=torch.float32).reshape(K, 1, 1, C).cuda() / 100.0
    y = ops.conv_fwd(x, w)
    ref = torch.einsum("nhwc,kc->nhwk", x, w[:, 0, 0, :])
    _close(y, ref, rtol=1e-5)


@pytest.mark.parametrize("path", ["wino4", "wino2", "fused64", "direct1x1", "direct3x3s2", "direct1x1s2"])
@pytest.mark.parametrize("relu,with_y", [(False, False), (True, False), (True, True)])
def test_data_gradient_pass_leaves_the_batch_norm_backward_sums(hip, path, relu, with_y):
    """denet_conv_wino_dgrad_sums / denet_conv_wino2f_sums / denet_conv_dgrad_sums + denet_bn_bwd_final: a data-gradient pass
    whose output is the gradient of a batch norm's OUTPUT also writes that layer's two backward reductions (the cuDNN BN-grad
    reduction of batch_norm.py:51-53 / the masked one of batch_norm_relu.py:50-54) - against the reduction pass of its own
    (denet_bn_bwd_sums) on the same tensors, and the pieces against the one-call form: denet_bn_bwd == sums + apply,
    denet_bn_fwd_train_pre == stats_final + apply (bit for bit)"""
    from denet_amd import ops
    g = torch.Generator().manual_seed(5)
    N, H, W = 2, 16, 16
    C, K, R = {"wino4": (128, 96, 3), "wino2": (64, 128, 3), "fused64": (64, 64, 3), "direct1x1": (256, 160, 1),
               "direct3x3s2": (64, 128, 3), "direct1x1s2": (128, 256, 1)}[path]
    pad = 1 if R == 3 else 0
    stride = 2 if path.endswith("s2") else 1          # strided layers: a row of sums per parity class of input pixels
    dy = torch.randn(N, H // stride, W // stride, K, generator=g).cuda()   # gradient of the convolution's output
    w = (torch.randn(K, R, R, C, generator=g) * 0.05).cuda()
    addt = torch.randn(N, H, W, C, generator=g).cuda()                 # an earlier contribution to the same gradient
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).cuda()      # the batch norm's input
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    rm, rs = torch.zeros(C).cuda(), torch.ones(C).cuda()
    res = torch.randn(N, H, W, C, generator=g).cuda() if with_y else None
    y, sm, si = ops.bn_fwd_train(x, gamma, beta, rm, rs, relu=relu, res=res)
    geom = ops.conv_geom((N, H, W, C), w.shape, stride, pad, None)
    with ops.algorithms(BWD_SUMS=3) as wino:
        wino[(1, geom)] = {"wino4": 4, "wino2": 2, "fused64": ops.FUSED2}.get(path, 0)
        sums = ops.BnSums(x, y if (relu and with_y) else None, gamma, beta, sm, si, relu)
        cache = {}
        dz = ops.conv_dgrad(dy, w, (N, H, W, C), add=addt, stride=stride, pad=pad, cache=cache, sums=sums)
        assert sums.partial is not None, "the pass did not leave the sums"
        dz_plain = ops.conv_dgrad(dy, w, (N, H, W, C), add=addt, stride=stride, pad=pad, cache={})
        assert torch.equal(dz, dz_plain)                               # the gradient itself is untouched by the request
        yy = y if (relu and with_y) else None
        la, _ = ops.bn_bwd_link(x, yy, dz, gamma, sm, si, relu=relu, beta=beta, pre=sums.partial)
        lb, _ = ops.bn_bwd_link(x, yy, dz, gamma, sm, si, relu=relu, beta=beta)
        _close(la.coef, lb.coef, rtol=2e-5)
        assert torch.equal(la.materialise(), la.materialise())
        # the pieces == the one-call forms
        dx_ref, _, dg_ref, db_ref = ops.bn_bwd(x, yy, dz, gamma, sm, si, relu=relu, beta=beta)
        assert torch.equal(lb.materialise(), dx_ref)


@pytest.mark.parametrize("case", [
    # N, H, W, C, K, R, stride, pad, add, sums
    (4, 32, 32, 64, 128, 3, 2, 1, True, True),       # strided 3x3 (first convolution of a stage): four parity classes, 1..4 taps
    (4, 32, 32, 64, 128, 1, 2, 0, False, True),      # strided 1x1 projection
    (2, 24, 24, 1536, 1024, 1, 1, 0, False, True),   # a head layer below the 1x1t threshold: pipelined 128x128 tile
    (3, 20, 20, 96, 160, 3, 1, 1, True, False),      # 3x3 stride 1 on the direct kernel, ragged tiles in every dimension
    (2, 16, 16, 256, 512, 3, 2, 1, False, False),
])
def test_data_gradient_over_the_transposed_filter_is_bit_identical(hip, case):
    """denet_conv_dgrad_t (igemm MODE_DGRAD_T: the filter operand wt [R][S][C][K] reduction-contiguous, ops.DGRAD_T) against
    denet_conv_dgrad / denet_conv_dgrad_sums on the same tensors: same products in the same order - the gradient (with and without
    an earlier contribution) and the batch norm's backward sums bit for bit, from a prepared transposed copy and from the call's own;
    and against fp64. Reference op: tensor.grad w.r.t. the input of conv2d (model_cnn.py:318, convolution.py:80-83)."""
    from denet_amd import ops
    N, H, W, C, K, R, stride, pad, with_add, with_sums = case
    g = torch.Generator().manual_seed(17)
    OH = (H + 2 * pad - R) // stride + 1
    dy = torch.randn(N, OH, OH, K, generator=g).cuda()
    w = (torch.randn(K, R, R, C, generator=g) * 0.05).cuda()
    addt = torch.randn(N, H, W, C, generator=g).cuda() if with_add else None
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    y, sm, si = ops.bn_fwd_train(x, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda(), relu=True)
    out = {}
    # DGRAD_S2 off: the subject is the implicit-GEMM kernel's two filter layouts, also at stride 2; the direct kernels (no Winograd
    # pass, nothing measured)
    with ops.algorithms(BWD_SUMS=3, DGRAD_1X1T_GFLOP=0.0, DGRAD_S2=False, POLICY=ops.direct_policy) as wino:
        for mode in ("plain", "transposed", "prepared"):
            wino.clear()
            with ops.switches(DGRAD_T=mode != "plain"):
                sums = ops.BnSums(x, None, gamma, beta, sm, si, True) if with_sums else None
                cache = {"train": True}
                if mode == "prepared":
                    cache["dgrad_t"] = True
                    ops.wino_prefetch_filters([(cache, w)])
                    assert cache["wt"][1]
                dx = ops.conv_dgrad(dy, w, (N, H, W, C), add=addt, stride=stride, pad=pad, cache=cache, sums=sums)
                assert ops._last_igemm_name().startswith("igemm_kernel<%d," % (1 if mode == "plain" else 3)), ops._last_igemm_name()
                if mode == "prepared":
                    assert not cache["wt"][1]
                if with_sums:
                    assert sums.partial is not None
                    la, _ = ops.bn_bwd_link(x, None, dx, gamma, sm, si, relu=True, beta=beta, pre=sums.partial)
                    out[mode] = (dx.clone(), la.coef.clone())
                else:
                    out[mode] = (dx.clone(),)
    for mode in ("transposed", "prepared"):
        for a, b in zip(out[mode], out["plain"]):
            assert torch.equal(a, b), "%s: differs from denet_conv_dgrad" % mode
    # fp64: dx = conv_transpose of dy with the (already flipped, KRSC) filter
    import torch.nn.functional as Fn
    w64 = w.double().permute(0, 3, 1, 2).contiguous()                     # [K][C][R][S]
    ref = Fn.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w64, stride=stride, padding=pad,
                              output_padding=(H + 2 * pad - R) % stride).permute(0, 2, 3, 1)
    if with_add:
        ref = ref + addt.double()
    _close(out["transposed"][0], ref.float(), rtol=2e-5)


@pytest.mark.parametrize("case", [(2, 12, 12, 448, 160, False, False), (2, 12, 12, 256, 96, True, False), (3, 8, 8, 160, 256, True, True),
                                  (1, 5, 7, 96, 64, False, True)])
def test_data_gradient_of_a_1x1_layer_over_the_transposed_filter(hip, case):
    """denet_conv_dgrad_1x1t (the head layers: forward kernel over w^T, ops.DGRAD_1X1T_GFLOP) against denet_conv_dgrad /
    denet_conv_dgrad_sums on the same tensors: the gradient bit for bit (with and without an earlier contribution), the batch
    norm's backward sums bit for bit as well (the same epilogue over the same 128-row tiles); from a prepared transposed copy
    (ops.wino_prefetch_filters) and from the call's own"""
    from denet_amd import ops
    N, H, W, C, K, with_add, with_sums = case
    g = torch.Generator().manual_seed(9)
    dy = torch.randn(N, H, W, K, generator=g).cuda()
    w = (torch.randn(K, 1, 1, C, generator=g) * 0.05).cuda()
    addt = torch.randn(N, H, W, C, generator=g).cuda() if with_add else None
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    y, sm, si = ops.bn_fwd_train(x, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda(), relu=True)
    out = {}
    with ops.algorithms(BWD_SUMS=3, DGRAD_T=False):          # DGRAD_T off: "plain" = denet_conv_dgrad itself (the k-major filter reads)
        for mode in ("plain", "transposed", "prepared"):
            with ops.switches(DGRAD_1X1T_GFLOP=0.0 if mode == "plain" else 1e-9):
                sums = ops.BnSums(x, None, gamma, beta, sm, si, True) if with_sums else None
                cache = {"train": True}
                if mode == "prepared":
                    cache["dgrad_1x1t"] = True
                    ops.wino_prefetch_filters([(cache, w)])
                    assert cache["wt"][1]
                dx = ops.conv_dgrad(dy, w, (N, H, W, C), add=addt, stride=1, pad=0, cache=cache, sums=sums)
                if mode != "plain":
                    assert cache.get("dgrad_1x1t")
                if mode == "prepared":
                    assert not cache["wt"][1]                  # consumed: valid for one step
                if with_sums:
                    assert sums.partial is not None
                    la, _ = ops.bn_bwd_link(x, None, dx, gamma, sm, si, relu=True, beta=beta, pre=sums.partial)
                    out[mode] = (dx.clone(), la.coef.clone())
                else:
                    out[mode] = (dx.clone(),)
    ref = torch.einsum("nhwk,kc->nhwc", dy.double(), w[:, 0, 0, :].double())
    if with_add:
        ref = ref + addt.double()
    _close(out["plain"][0], ref.float(), rtol=1e-5)
    for mode in ("transposed", "prepared"):
        for a, b in zip(out[mode], out["plain"]):
            assert torch.equal(a, b), mode


@pytest.mark.parametrize("code,C,K,R,stride,pad", [
    (0, 32, 160, 3, 1, 1), (1, 32, 160, 3, 1, 1), (5, 32, 160, 3, 1, 1), (2, 32, 160, 3, 1, 1), (6, 32, 160, 1, 1, 0),
    (1, 160, 32, 3, 1, 1), (5, 160, 32, 3, 1, 1), (6, 160, 32, 1, 1, 0),            # the data gradients' columns are C
    (1, 32, 160, 3, 2, 1), (5, 32, 160, 3, 2, 1), (1, 160, 32, 3, 2, 1), (5, 160, 32, 3, 2, 1),
])
@pytest.mark.parametrize("state", ["cleared", "committed"])
def test_what_is_planned_is_what_runs(hip, code, C, K, R, stride, pad, state):
    """denet_conv_plan against denet_conv_last_config of the launch itself, at batch 2, 16 x 16: 160 channels are two column
    tiles of 128 (or three of 64), the last one padded; stride 2 runs four parity classes; the filter gradient has workspace for
    more than one split slice. With the table of measured configurations empty and as the process loaded it."""
    import ctypes
    from denet_amd import ops
    g = ops.conv_geom((2, 16, 16, C), (K, R, R, C), stride, pad)
    t = _igemm_tensors(g, 3)
    ws_bytes = t["ws"].numel() * 4

    def check_once(L):
        plan = [ctypes.c_int() for _ in range(4)]
        assert L.denet_conv_plan(code, *g, 1, ws_bytes if code == 2 else 0, *[ctypes.byref(v) for v in plan]) == 0
        _igemm_pass(L, code, g, t, ws_bytes)
        ran = [ctypes.c_int() for _ in range(5)]
        L.denet_conv_last_config(*[ctypes.byref(v) for v in ran])
        assert [v.value for v in ran] == [{0: 0, 1: 1, 2: 2, 5: 3, 6: 0}[code]] + [v.value for v in plan]
        return [v.value for v in plan]

    if state == "cleared":
        with _TunedTable() as L:
            plan = check_once(L)
    else:
        ops._load_tuned_once()
        plan = check_once(ops._L())
    torch.cuda.synchronize()
    assert plan[3] == (stride * stride if code in (1, 5) else 1) or code == 2
    if code == 2:
        assert plan[3] > 1, plan                      # 16 pixel chunks, 64 slices of workspace: the price loop splits


@pytest.mark.parametrize("mode,C,K,ncand", [(0, 32, 160, 4), (1, 160, 32, 4), (2, 32, 160, 9)])
def test_conv_tune_times_its_candidates_and_keeps_one(hip, mode, C, K, ncand):
    """denet_conv_tune (the timing loop of csrc/igemm.hip) at batch 2, 16 x 16, 3x3: it stores one of its candidates, leaves the
    pass's result in `out` - the bits of an untuned run for forward and data gradient, whose candidates sum in one order; the
    filter gradient (another split-K grouping) within the tolerance of test_conv_fwd_dgrad_wgrad against float64 -, and a second
    call measures nothing: one launch, the record as it was."""
    import ctypes
    from denet_amd import ops
    from denet_amd.ops import ptr, stream_ptr
    g = ops.conv_geom((2, 16, 16, C), (K, 3, 3, C), 1, 1)
    t = _igemm_tensors(g, 5 + mode)
    ws_bytes = t["ws"].numel() * 4
    a, b, out = {0: ("x", "w", "y"), 1: ("dy", "w", "dx"), 2: ("x", "dy", "dw")}[mode]
    cand = {(0, nb, r) for nb, rr in ((1, 6), (2, 3)) for r in range(1, rr + 1)} if mode == 2 else \
        {(tl, nb, 0) for tl in (0, 1) for nb in (1, 2)}
    assert len(cand) == ncand

    def record(L):
        v = [ctypes.c_int() for _ in range(3)]
        rc = L.denet_conv_tuned(mode, *g[:10], *[ctypes.byref(x) for x in v])
        return rc, tuple(x.value for x in v)

    def tune(L):
        return L.denet_conv_tune(mode, ptr(t[a]), ptr(t[b]), None, None, ptr(t[out]), ptr(t["ws"]), ws_bytes, *g, stream_ptr())

    with _TunedTable() as L:
        assert record(L)[0] == 1
        plain = _igemm_pass(L, mode, g, t, ws_bytes).clone()
        t[out].zero_()
        assert tune(L) == 0, L.denet_last_error()
        rc, rec = record(L)
        assert rc == 0 and rec in cand, rec
        tuned = t[out].clone()
        t[out].zero_()
        assert L.denet_conv_profile(2) == 0              # launch trace: which matrix kernels the second call starts
        try:
            assert tune(L) == 0
            launches = L.denet_conv_profile_count()
        finally:
            L.denet_conv_profile(0)
        assert launches == 1 and record(L) == (0, rec)
        assert torch.equal(t[out], tuned)
    if mode == 2:
        x64, dy64 = t["x"].double().permute(0, 3, 1, 2), t["dy"].double().permute(0, 3, 1, 2)
        ref = torch.nn.grad.conv2d_weight(x64, (K, C, 3, 3), dy64, stride=1, padding=1).permute(0, 2, 3, 1)
        _close(tuned, ref.float())
        _close(plain, ref.float())
    else:
        assert torch.equal(tuned, plain)


def test_conv_wino_tune_leaves_a_record_per_batched_product(hip):
    """denet_conv_wino_tune at F(2x2), batch 2, 8 x 8, 32 channels: the same timing loop over the batched component GEMM (mode 3,
    one key for forward and data gradient at C = K) and the batched filter-gradient product (mode 4) of 16 members, 32 tiles"""
    import ctypes
    from denet_amd.ops import ptr, stream_ptr
    N, H, W, C, K, tile = 2, 8, 8, 32, 32, 2
    with _TunedTable() as L:
        ws = torch.empty(L.denet_conv_wino_workspace_bytes(tile, N, H, W, C, K) // 4, device="cuda")
        sws = torch.empty(64 * 16 * C * K, device="cuda")
        key = (16, 1, N * (H // tile) * (W // tile), C, K, 1, 1, 1, 1, 0)
        v = [ctypes.c_int() for _ in range(3)]
        assert L.denet_conv_tuned(3, *key, *[ctypes.byref(x) for x in v]) == 1
        assert L.denet_conv_wino_tune(ptr(ws), ws.numel() * 4, ptr(sws), sws.numel() * 4, tile, N, H, W, C, K, stream_ptr()) == 0, \
            L.denet_last_error()
        assert L.denet_tune_export(None, 0) == 2
        assert L.denet_conv_tuned(3, *key, *[ctypes.byref(x) for x in v]) == 0
        assert tuple(x.value for x in v) in {(1, 1, 0), (1, 2, 0)}                      # 32 columns: the 128 x 64 tile only
        assert L.denet_conv_tuned(4, *key, *[ctypes.byref(x) for x in v]) == 0
        assert tuple(x.value for x in v) in {(0, nb, r) for nb, rr in ((1, 6), (2, 3)) for r in range(1, rr + 1)}


@pytest.mark.parametrize("shape", [(4, 16, 16, 64), (2, 8, 8, 1536), (3, 5, 7, 768), (2, 32, 32, 128)])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_bn_fwd_bwd(hip, shape, relu, res):
    from denet_amd import ops
    g = torch.Generator().manual_seed(11)
    N, H, W, C = shape
    x = (torch.randn(shape, generator=g) * 2 + 0.5).cuda().requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda().requires_grad_(True)
    beta = torch.randn(C, generator=g).cuda().requires_grad_(True)
    r = torch.randn(shape, generator=g).cuda().requires_grad_(True) if res else None
    rm, rs = torch.zeros(C).cuda(), torch.ones(C).cuda()
    eps = 1e-5
    xf = x.reshape(-1, C)
    mean = xf.mean(0)
    var = xf.var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(var + eps)
    yr = (x - mean) * inv * gamma + beta
    if res:
        yr = yr + r
    if relu:
        yr = torch.relu(yr)
    dy = torch.randn(shape, generator=g).cuda()
    yr.backward(dy)

    y, sm, si = ops.bn_fwd_train(x.detach(), gamma.detach(), beta.detach(), rm, rs, 0.9, eps, relu=relu,
                                 res=r.detach() if res else None)
    _close(y, yr)
    _close(sm, mean)
    _close(si, inv)
    _close(rm, 0.1 * mean)
    _close(rs, 0.9 + 0.1 * inv)
    dx, dres, dgamma, dbeta = ops.bn_bwd(x.detach(), y, dy, gamma.detach(), sm, si, relu=relu, want_dres=res)
    if relu and not res:
        # mask recomputed from x instead of read from y: bit-identical results
        dx2, _, dg2, db2 = ops.bn_bwd(x.detach(), None, dy, gamma.detach(), sm, si, relu=True, beta=beta.detach())
        assert torch.equal(dx2, dx) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    _close(dx, x.grad, rtol=2e-3)
    _close(dgamma, gamma.grad, rtol=2e-3)
    _close(dbeta, beta.grad, rtol=2e-3)
    if res:
        _close(dres, r.grad)


def _bn_final_order(p):
    """csrc/bn_reduce.h in numpy float64: the sum of the rows p [rows] of one column as the second stage adds them - lane jl of
    32 takes rows jl, jl + 32, ...: four at a time as (p[j] + p[j+32]) + (p[j+64] + p[j+96]) while j + 96 < rows, then one by
    one; the lane sums go through a butterfly over the xor offsets 1, 2, 4, 8, 16; lane 0 holds the result"""
    rows = len(p)
    lanes = np.zeros(32, np.float64)
    for jl in range(32):
        acc, j = np.float64(0), jl
        while j + 96 < rows:
            acc = acc + ((p[j] + p[j + 32]) + (p[j + 64] + p[j + 96]))
            j += 128
        while j < rows:
            acc = acc + p[j]
            j += 32
        lanes[jl] = acc
    for off in (1, 2, 4, 8, 16):
        lanes = lanes + lanes[np.arange(32) ^ off]
    return lanes[0]


@pytest.mark.parametrize("rows", [1, 2, 32, 33, 96, 97, 128, 129, 300])
def test_bn_final_summation_order_is_pinned(hip, rows):
    """the second stage of the batch-norm reductions (denet_bn_bwd_final over a given partial [rows][2][C]) is DEFINED bit for
    bit: the order of csrc/bn_reduce.h, emulated in numpy float64 (_bn_final_order). 33 rows: the first count that gives a lane
    two rows; 97: the first that enters the four-loads-in-flight loop. The rows cancel (a half, its negation permuted per column,
    magnitudes up to 2^40), so what is left of a sum is the rounding of ITS order: a plain in-order sum gives other float32
    values, which the test checks on the host before it trusts the comparison"""
    from denet_amd import ops
    C, M = 6, 3
    rng = np.random.RandomState(rows)
    h = rows // 2
    a = rng.standard_normal((h, 2, C)) * 2.0 ** rng.randint(0, 40, (h, 2, C))
    b = np.empty_like(a)
    for k in range(2):
        for c in range(C):
            b[:, k, c] = -a[rng.permutation(h), k, c]
    p = np.concatenate([a, b] + ([rng.standard_normal((1, 2, C))] if rows % 2 else []))
    assert p.shape == (rows, 2, C)
    want = np.array([[_bn_final_order(p[:, k, c]) for c in range(C)] for k in range(2)])
    if rows >= 32:
        plain = np.zeros((2, C))
        for j in range(rows):
            plain = plain + p[j]
        differ = int((plain.astype(np.float32) != want.astype(np.float32)).sum())
        assert differ >= 6, "the inputs do not show the order: an in-order sum differs in %d of 12 values" % differ
    partial = torch.from_numpy(p).cuda()
    dgamma, dbeta, coef = ops.empty(C), ops.empty(C), ops.empty(2 * C)
    ops.check(ops._L().denet_bn_bwd_final(ops.ptr(partial), rows, M, C, ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(coef),
                                          ops.stream_ptr()), "bn_bwd_final")
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits(dbeta), want[0].astype(np.float32).view(np.uint32))
    assert np.array_equal(bits(dgamma), want[1].astype(np.float32).view(np.uint32))
    assert np.array_equal(bits(coef), (want / np.float64(M)).astype(np.float32).reshape(2 * C).view(np.uint32))


def test_bn_known_answer(hip):
    """Reference's own KAT (denet/layer/batch_norm.py:131-154): x~U(0,1) (64,128,32,32), running stdinv mean
    = 0.9 + 0.1/sqrt(1/12 + 1e-5) = 1.24641, running mean = 0.1*mean(x), output mean 0 / std 1."""
    from denet_amd import ops
    rng = np.random.RandomState(1002)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (64, 128, 32, 32)).astype(np.float32)).cuda()
    xn = ops.nchw_to_nhwc(x, 128)
    C = 128
    rm, rs = torch.zeros(C).cuda(), torch.ones(C).cuda()
    y, _, _ = ops.bn_fwd_train(xn, torch.ones(C).cuda(), torch.zeros(C).cuda(), rm, rs, 0.9, 1e-5)
    eps = 1e-4
    assert abs(float(y.mean())) < eps and abs(float(y.std()) - 1.0) < eps
    assert abs(float(rm.mean()) - float(x.mean()) * 0.1) < eps
    assert abs(float(rs.mean()) - 1.24641) < eps


def test_bn_test_mode_double_eps(hip):
    from denet_amd import ops
    g = torch.Generator().manual_seed(3)
    C = 64
    x = torch.randn(2, 4, 4, C, generator=g).cuda()
    gamma, beta = torch.rand(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    rm, rs = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    y = ops.bn_fwd_test(x, gamma, beta, rm, rs, eps=1e-5, relu=True)
    var = (1.0 / rs) ** 2
    ref = torch.relu((x - rm) / torch.sqrt(var + 1e-5) * gamma + beta)
    _close(y, ref)


@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
def test_maxpool(hip, k, s, p):
    from denet_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 64, 18, 22, generator=g).cuda().requires_grad_(True)
    yr = Fn.max_pool2d(x, k, s, p)
    dy = torch.randn(yr.shape, generator=g).cuda()
    yr.backward(dy)
    y, arg = ops.maxpool_fwd(_nhwc(x.detach()), k, s, p)
    assert torch.equal(_nchw(y), yr)
    dx = ops.maxpool_bwd(_nhwc(dy), arg, (2, 18, 22, 64), k, s, p)
    _close(_nchw(dx), x.grad, rtol=1e-5)


@pytest.mark.parametrize("k,s,p", [(8, 8, 0), (7, 7, 0), (3, 2, 1)])
def test_avgpool(hip, k, s, p):
    from denet_amd import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 16, 16, generator=g).cuda().requires_grad_(True)
    yr = Fn.avg_pool2d(x, k, s, p, count_include_pad=True)
    dy = torch.randn(yr.shape, generator=g).cuda()
    yr.backward(dy)
    y = ops.avgpool_fwd(_nhwc(x.detach()), k, s, p)
    _close(_nchw(y), yr, rtol=1e-5)
    dx = ops.avgpool_bwd(_nhwc(dy), (2, 16, 16, 64), k, s, p)
    _close(_nchw(dx), x.grad, rtol=1e-5)


def test_pool_inv(hip):
    """Differential design of the reference's own check (denet/layer/pool_inv.py:43-88): op vs double repeat."""
    from denet_amd import ops
    rng = np.random.RandomState(1)
    x = torch.from_numpy(rng.uniform(-5, 5, (4, 64, 4, 4)).astype(np.float32)).cuda()
    y = ops.pool_inv_fwd(_nhwc(x), 2, 2)
    ref = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    assert torch.equal(_nchw(y), ref)
    dy = torch.from_numpy(rng.uniform(-1, 1, (4, 64, 8, 8)).astype(np.float32)).cuda()
    dx = ops.pool_inv_bwd(_nhwc(dy), 2, 2)
    ref = dy.reshape(4, 64, 4, 2, 4, 2).sum(dim=(3, 5))
    _close(_nchw(dx), ref, rtol=1e-6)


def test_border_crop_dropout_concat_kernels_vs_oracle(hip):
    """csrc/augment.hip against the oracle restatements, bit-exact (pure copies / one multiply by a constant)"""
    from denet_amd import ops
    from oracle import layers as L
    rng = np.random.RandomState(4)
    N, C, CP, H, W = 3, 40, 64, 9, 11
    x = rng.randn(N, C, H, W).astype(np.float32)
    xd = ops.nchw_to_nhwc(torch.from_numpy(x).cuda(), CP)

    def back(t, c=C):
        return ops.nhwc_to_nchw(t, c).cpu().numpy()

    # B
    b = (2, 1, 0, 3)
    y = ops.border_fwd(xd, b)
    assert np.array_equal(back(y), L.border(x, b))
    assert np.array_equal(back(ops.border_bwd(y, b)), x)
    # CM: training geometry per image from the counter generator, centre crop at test time
    for train in (True, False):
        for it in range(4):
            seed = L.layer_seed(77, 1, it)
            geom = L.crop_mirror_geom(N, H, W, 5, 6, 0.5, 0.5, train, seed)
            y = ops.crop_mirror_fwd(xd, (5, 6), 0.5, 0.5, train, seed)
            ref = L.crop_mirror(x, (5, 6), geom)
            assert np.array_equal(back(y), ref)
            dy = rng.randn(*ref.shape).astype(np.float32)
            dx = ops.crop_mirror_bwd(ops.nchw_to_nhwc(torch.from_numpy(dy).cuda(), CP), (N, H, W, CP), 0.5, 0.5, train, seed)
            assert np.array_equal(back(dx), L.crop_mirror_grad(dy, x.shape, geom))
    # D: mask is a function of the LOGICAL NCHW index (independent of the channel padding), padding stays zero
    for rate in (0.0, 0.3, 0.5):
        seed = L.layer_seed(5, 2, 9)
        y = ops.dropout(xd, C, rate, seed)
        assert np.array_equal(back(y), x * L.dropout_mask(x.shape, rate, seed))
        assert float(y[..., C:].abs().max()) == 0.0
        y32 = ops.dropout(ops.nchw_to_nhwc(torch.from_numpy(x[:, :32].copy()).cuda(), 32), 32, rate, seed)
        assert np.array_equal(back(y32, 32), x[:, :32] * L.dropout_mask((N, 32, H, W), rate, seed))
    # SKIP concat of two channel-padded buffers and its split gradient
    z = rng.randn(N, 24, H, W).astype(np.float32)
    zd = ops.nchw_to_nhwc(torch.from_numpy(z).cuda(), 32)
    y = ops.concat_fwd(xd, zd, C, 24, 64)
    assert y.shape[-1] == 64 and np.array_equal(back(y, 64), np.concatenate([x, z], axis=1))
    y96 = ops.concat_fwd(xd, zd, C, 24, 96)
    assert float(y96[..., 64:].abs().max()) == 0.0
    da, db = ops.concat_bwd(y, C, CP, 24, 32)
    assert np.array_equal(back(da, CP)[:, :C], x) and float(da[..., C:].abs().max()) == 0.0
    assert np.array_equal(back(db, 32)[:, :24], z) and float(db[..., 24:].abs().max()) == 0.0
    # bias epilogue of DC
    bias = torch.from_numpy(rng.randn(CP).astype(np.float32)).cuda()
    yb = ops.add_bias(xd, bias)
    assert torch.equal(yb, xd + bias)


def test_dropout_full_size_statistics(hip):
    """a hot-path-sized activation (32 x 64 x 128 x 128): keep rate, mean preservation, forward/backward masks equal"""
    from denet_amd import ops
    x = torch.ones(32, 128, 128, 64, device="cuda")
    y = ops.dropout(x, 64, 0.25, 12345)
    keep = (y > 0).float().mean().item()
    assert abs(keep - 0.75) < 1e-3
    assert abs(y.mean().item() - 1.0) < 2e-3
    assert torch.equal(y, ops.dropout(x, 64, 0.25, 12345))
    assert not torch.equal(y, ops.dropout(x, 64, 0.25, 12346))


def test_elementwise_and_solver(hip):
    from denet_amd import ops
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1024, generator=g).cuda(), torch.randn(1024, generator=g).cuda()
    assert torch.equal(ops.add(a, b), a + b)
    assert torch.equal(ops.add(a, b, relu=True), torch.relu(a + b))
    y = ops.relu_fwd(a)
    assert torch.equal(y, torch.relu(a))
    assert torch.equal(ops.relu_bwd(y, b), b * (y > 0))
    m = torch.randn(300, 96, generator=g).cuda()
    _close(ops.colsum(m), m.sum(0), rtol=1e-5)
    for mode in (0, 1):
        for it in (0, 3):
            p = torch.randn(1000, generator=g).cuda()
            mom = torch.randn(1000, generator=g).cuda()
            gr = torch.randn(1000, generator=g).cuda()
            p0, m0 = p.clone(), mom.clone()
            ops.solver_step(p, mom, gr, 600, 0.1, 0.9, it, 1e-2, mode)
            gg = gr.clone()
            gg[:600] += 1e-2 * p0[:600]
            rho = 0.9 if it > 0 else 0.0
            if mode == 1:
                mr = rho * m0 + gg
                pr = p0 - 0.1 * (gg + 0.9 * mr)
            else:
                mr = rho * m0 + (1 - rho) * gg
                pr = p0 - 0.1 * mr
            _close(mom, mr, rtol=1e-5)
            _close(p, pr, rtol=1e-5)


def test_corner_fwd_loss(hip):
    from denet_amd import ops
    g = torch.Generator().manual_seed(10)
    B, H, W, CP, Cn = 3, 16, 16, 128, 4
    conv = (torch.randn(B, H, W, CP, generator=g) * 3).cuda().requires_grad_(True)
    x = conv[..., :Cn].permute(0, 3, 1, 2)
    lh = torch.stack([x, -x], dim=1)
    pr_ref = torch.log_softmax(lh, dim=1)
    tgt = torch.rand(B, 2, Cn, H, W, generator=g).cuda() / (H * W * Cn)
    cost_ref = 100.0 * (-(tgt * pr_ref).sum(dim=(1, 2, 3, 4)).mean() / np.log(2))
    cost_ref.backward()
    pr = ops.corner_fwd(conv.detach(), Cn)
    _close(pr, pr_ref, rtol=1e-5, atol=1e-6)
    dconv = torch.zeros(B, H, W, CP).cuda()
    cost = torch.zeros(1).cuda()
    ops.corner_loss(pr, tgt, dconv, cost, 100.0)
    _close(cost, cost_ref.reshape(1), rtol=1e-5)
    _close(dconv, conv.grad, rtol=1e-4)


def _sparse_ref(fmap_nchw, bbox, gs, rule):
    """numpy restatement of the two tap formulas (denet_sparse.py:72-84 / denet_sparse_op.py:65-71)."""
    B, Fc, H, W = fmap_nchw.shape
    M = bbox.shape[0]
    rois = M // B
    out = np.zeros((M, gs * gs * Fc + 2), np.float32)
    taps = np.zeros((M, gs * gs), np.int32)
    f32 = np.float32
    for m in range(M):
        b = m // rois
        x0, y0, x1, y1 = [f32(v) for v in bbox[m]]
        bw, bh = f32(x1 - x0), f32(y1 - y0)

        def tap(p0, ext, i, size):
            if rule == 0:
                p = f32(p0 + f32(f32(f32(i) * ext) / f32(gs - 1)))
            else:
                k = f32(f32(1.0) / f32(gs - 1))
                p = f32(p0 + f32(f32(f32(i) * ext) * k))
            f = f32(p * f32(size))
            f = max(f32(0.0), min(f, f32(size - 1)))
            if rule == 0:
                return int(np.rint(f))
            return int(np.floor(f + f32(0.5))) if f >= 0 else int(np.ceil(f - f32(0.5)))

        for yi in range(gs):
            ys = tap(y0, bh, yi, H)
            for xi in range(gs):
                xs = tap(x0, bw, xi, W)
                t = yi * gs + xi
                taps[m, t] = ys * W + xs
                out[m, t * Fc:(t + 1) * Fc] = fmap_nchw[b, :, ys, xs]
        out[m, gs * gs * Fc] = bh
        out[m, gs * gs * Fc + 1] = bw
    return out, taps


@pytest.mark.parametrize("rule", [0, 1])
def test_sparse_fwd_bwd(hip, rule):
    from denet_amd import ops
    rng = np.random.RandomState(1)
    B, Fc, H, W, sn, gs = 3, 32, 16, 16, 6, 7
    CP, coff = 64, 4
    rois = sn * sn
    M = B * rois
    fm = rng.uniform(-5, 5, (B, Fc, H, W)).astype(np.float32)
    bbox = np.zeros((M, 4), np.float32)
    for m in range(M):
        x0, y0 = rng.uniform(0, 1), rng.uniform(0, 1)
        bbox[m] = (x0, y0, rng.uniform(x0, 1), rng.uniform(y0, 1))
    # detector-style boxes on the cell lattice: exact .5 taps exercise the rounding rule
    for m in range(0, M, 3):
        c = rng.randint(0, W, 4)
        bbox[m] = (min(c[0], c[2]) / W, min(c[1], c[3]) / H, (max(c[0], c[2]) + 1) / W, (max(c[1], c[3]) + 1) / H)
    ref, taps_ref = _sparse_ref(fm, bbox, gs, rule)
    fmap = torch.zeros(B, H, W, CP).cuda()
    fmap[..., coff:coff + Fc] = torch.from_numpy(fm).cuda().permute(0, 2, 3, 1)
    KP = ((gs * gs * Fc + 2 + 31) // 32) * 32
    out, taps = ops.sparse_fwd(fmap, torch.from_numpy(bbox).cuda(), coff, Fc, rois, gs, KP, rule)
    assert np.array_equal(taps.cpu().numpy(), taps_ref)            # bit-exact indices
    assert np.array_equal(out[:, :gs * gs * Fc + 2].cpu().numpy(), ref)   # pure copy -> bit-exact values
    assert float(out[:, gs * gs * Fc + 2:].abs().max()) == 0.0
    # gradient: scatter-add of dy back to the sampled cells
    dy = rng.uniform(-1, 1, (M, KP)).astype(np.float32)
    dref = np.zeros((B, H * W, Fc), np.float64)
    for m in range(M):
        for t in range(gs * gs):
            dref[m // rois, taps_ref[m, t]] += dy[m, t * Fc:(t + 1) * Fc]
    dfmap = torch.full((B, H, W, CP), 7.0).cuda()
    ops.sparse_bwd(torch.from_numpy(dy).cuda(), taps, dfmap, coff, Fc, rois, gs, coff + Fc)
    got = dfmap.cpu().numpy().reshape(B, H * W, CP)
    np.testing.assert_allclose(got[:, :, coff:coff + Fc], dref, rtol=1e-4, atol=1e-5)
    assert np.all(got[:, :, coff + Fc:] == 0.0)
    assert np.all(got[:, :, :coff] == 7.0)      # corner-logit channels are owned by corner_loss
    # determinism
    dfmap2 = torch.zeros(B, H, W, CP).cuda()
    ops.sparse_bwd(torch.from_numpy(dy).cuda(), taps, dfmap2, coff, Fc, rois, gs, coff + Fc)
    assert torch.equal(dfmap2[..., coff:], dfmap[..., coff:])


@pytest.mark.parametrize("Fc", [96, 80, 32, 256])
def test_sparse_bwd_summation_order(hip, Fc):
    """the gather gradient's result is DEFINED bit for bit (the deterministic replacement of the reference's atomicAdd scatter,
    denet_sparse_op.py:171-212): the (roi, tap) entries of a cell in ascending slot order, entry j in chain j % epi with
    epi = 64 // (F / 4), every chain summed left to right from +0, the chains added in order - emulated here in numpy float32.
    Clustered boxes put hundreds of entries on a cell (the kernel takes the slots of a cell in chunks of (64 // epi) * epi)"""
    from denet_amd import ops
    rng = np.random.RandomState(4)
    B, H, W, rois, gs = 2, 12, 12, 150, 5
    CP = ((Fc + 31) // 32) * 32
    M = B * rois
    cx, cy = rng.normal(0.5, 0.06, M), rng.normal(0.5, 0.06, M)
    w, h = rng.uniform(0.02, 0.15, M), rng.uniform(0.02, 0.15, M)
    bbox = np.clip(np.stack([cx - w, cy - h, cx + w, cy + h], 1), 0, 1).astype(np.float32)
    fmap = torch.zeros(B, H, W, CP).cuda()
    KP = ((gs * gs * Fc + 2 + 31) // 32) * 32
    _, taps = ops.sparse_fwd(fmap, torch.from_numpy(bbox).cuda(), 0, Fc, rois, gs, KP, 0)
    dy = rng.uniform(-1, 1, (M, KP)).astype(np.float32)
    dfmap = torch.zeros(B, H, W, CP).cuda()
    ops.sparse_bwd(torch.from_numpy(dy).cuda(), taps, dfmap, 0, Fc, rois, gs, Fc)
    got = dfmap.cpu().numpy().reshape(B, H * W, CP)
    tp = taps.cpu().numpy().reshape(B, rois * gs * gs)
    epi = 64 // (Fc // 4)
    ntap = gs * gs
    most = 0
    for b in range(B):
        for cell in range(H * W):
            slots = np.nonzero(tp[b] == cell)[0]                      # ascending slot = roi * ntap + tap
            most = max(most, len(slots))
            chains = [np.zeros(Fc, np.float32) for _ in range(epi)]
            for j, sl in enumerate(slots):
                roi, tap = divmod(int(sl), ntap)
                chains[j % epi] = chains[j % epi] + dy[b * rois + roi, tap * Fc:(tap + 1) * Fc]
            tot = chains[0]
            for k in range(1, epi):
                tot = tot + chains[k]
            assert np.array_equal(got[b, cell, :Fc], tot), (b, cell, len(slots))
    assert most > 128                                                  # more than two chunks of slots on one cell


@pytest.mark.parametrize("case", [(32, 64, 64, 576, 7), (3, 20, 36, 100, 5), (2, 128, 128, 2304, 7), (1, 9, 7, 3000, 2),
                                  (2, 90, 77, 1500, 7), (1, 33, 31, 30000, 3)])
def test_sparse_tap_counting_sort(hip, case):
    """the grouping of the (roi, tap) slots by cell that the gather gradient sums over (replaces the reference's atomicAdd
    scatter, denet_sparse_op.py:171-212): per image it must be exactly the STABLE sort of the tap list by cell - every
    cell's slots in ascending order - including cells hit thousands of times and lists that span many 2048-slot chunks"""
    import ctypes
    from denet_amd import ops
    B, H, W, rois, gs = case
    rng = np.random.RandomState(B * 7 + rois)
    n = rois * gs * gs
    taps = rng.randint(0, H * W, (B, n)).astype(np.int32)
    taps[0, : n // 2] = rng.randint(0, 3, n // 2)              # three cells collect half of image 0's slots
    taps[-1, n // 3:] = H * W - 1                               # the last cell collects two thirds of the last image's
    L = ops._L()
    nbytes = L.denet_sparse_sort_workspace_bytes(B, H, W, rois, gs)
    ws = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
    td = torch.from_numpy(taps).cuda()
    ops.check(L.denet_sparse_sort(ops.ptr(td), ops.ptr(ws), nbytes, B, H, W, rois, gs, ops.stream_ptr()), "sparse_sort")
    got = ws.cpu().numpy()
    order = got[:B * n].reshape(B, n)
    start = got[B * n:B * n + B * (H * W + 1)].reshape(B, H * W + 1)
    for b in range(B):
        assert np.array_equal(order[b], np.argsort(taps[b], kind="stable")), b
        cnt = np.bincount(taps[b], minlength=H * W)
        assert np.array_equal(start[b], np.concatenate([[0], np.cumsum(cnt)])), b
    # too small a workspace / too large a map are argument errors, not memory corruption
    assert L.denet_sparse_sort(ops.ptr(td), ops.ptr(ws), nbytes - 4, B, H, W, rois, gs, ops.stream_ptr()) == -1000
    assert L.denet_sparse_sort_workspace_bytes(1, 256, 256, 4, 2) == 0


def test_side_streams_run_beside_the_compute_stream(hip):
    """ops.init_streams: the filter-gradient / side streams are picked by probing (two idle kernels) so that they sit on a
    hardware queue of their own - the HIP runtime multiplexes all streams of a process onto 4 queues, and a filter-gradient
    stream that shares the compute stream's queue serialises the two backward chains silently"""
    import time
    from denet_amd import ops
    ops.init_streams(force=True)
    main = torch.cuda.current_stream()
    assert ops._runs_beside(ops._WGRAD_STREAM, main)
    assert ops._runs_beside(ops._SIDE_FILTER, main) and ops._runs_beside(ops._SORT_STREAM, main)
    assert not ops._runs_beside(main, main)                       # same stream: strictly serial
    # the probe kernel idles for about the time asked for
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.check(hip.denet_spin(20000, main.cuda_stream), "spin")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert 0.015 < dt < 0.08, dt


@pytest.mark.parametrize("bounded", [False, True])
def test_detect_loss(hip, bounded):
    from denet_amd import ops
    g = torch.Generator().manual_seed(12)
    B, rois, ncls, CP = 2, 36, 81, 96
    M = B * rois
    logits = torch.randn(M, CP, generator=g).cuda().requires_grad_(True)
    t = torch.zeros(M, ncls)
    cls = torch.randint(0, ncls, (M,), generator=g)
    t[torch.arange(M), cls] = 1.0
    t[::5, 3] = 1.0
    t = (t / t.sum(1, keepdim=True) / rois).cuda()
    valid = ((torch.rand(M, generator=g) > 0.5).float() / rois).cuda()
    roi = torch.rand(M, 4, generator=g)
    roi[:, 2:] = roi[:, :2] + 0.05 + roi[:, 2:] * 0.5
    tb = torch.rand(M, 4, generator=g)
    tb[:, 2:] = tb[:, :2] + 0.05 + tb[:, 2:] * 0.5
    def cxcywh(bx):
        return torch.stack([0.5 * (bx[:, 0] + bx[:, 2]), 0.5 * (bx[:, 1] + bx[:, 3]), bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], 1)
    bt = torch.cat([cxcywh(tb), cxcywh(roi)], 1).cuda()
    roi = roi.cuda()
    cost_factor, bbox_factor = 1.0, 2.0
    lp = torch.log_softmax(logits[:, :ncls], 1)
    det_err = -(t * lp).sum(1) / np.log(ncls)
    reg = logits[:, ncls:ncls + 4]
    if not bounded:
        tt = torch.stack([(bt[:, 0] - bt[:, 4]) / bt[:, 6], (bt[:, 1] - bt[:, 5]) / bt[:, 7],
                          torch.log(bt[:, 2] / bt[:, 6]), torch.log(bt[:, 3] / bt[:, 7])], 1)
        d = tt - reg
    else:
        scx, scy = 0.5 * (roi[:, 0] + roi[:, 2]), 0.5 * (roi[:, 1] + roi[:, 3])
        sw, sh = roi[:, 2] - roi[:, 0], roi[:, 3] - roi[:, 1]
        pcx, pcy = reg[:, 0] * sw + scx, reg[:, 1] * sh + scy
        pw, ph = torch.exp(reg[:, 2]) * sw, torch.exp(reg[:, 3]) * sh
        dx, dyv = bt[:, 0] - pcx, bt[:, 1] - pcy
        e = 0.001
        cx = torch.where(dx >= 0, 2 * dx / (bt[:, 2] + dx + e), -2 * dx / (bt[:, 2] - dx + e))
        cy = torch.where(dyv >= 0, 2 * dyv / (bt[:, 3] + dyv + e), -2 * dyv / (bt[:, 3] - dyv + e))
        cw = 1.0 - torch.minimum(bt[:, 2] / (pw + e), pw / (bt[:, 2] + e))
        ch = 1.0 - torch.minimum(bt[:, 3] / (ph + e), ph / (bt[:, 3] + e))
        d = torch.stack([cx, cy, cw, ch], 1)
    sl1 = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    bbox_err = bbox_factor * valid * sl1.sum(1)
    c_det = cost_factor * det_err.sum() / B
    c_bbox = bbox_factor * bbox_err.sum() / B
    (c_det + c_bbox).backward()
    dl = torch.full((M, CP), 5.0).cuda()
    costs = torch.zeros(2).cuda()
    ops.detect_loss(logits.detach(), t, valid, bt, roi, dl, costs, B, ncls, 4, cost_factor, bbox_factor, bounded)
    _close(costs, torch.stack([c_det, c_bbox]).detach(), rtol=1e-4)
    _close(dl, logits.grad, rtol=2e-3, atol=1e-7)


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("shape", [(2, 8, 8, 32, 64), (3, 16, 12, 64, 32), (2, 32, 32, 256, 128)])
def test_conv_winograd_vs_direct(hip, shape, tile):
    """Winograd F(2x2,3x3) / F(4x4,3x3) forward, data gradient and filter gradient of the 3x3 stride-1 pad-1 convolution
    against the direct implicit-GEMM kernels (same sums, different rounding) incl. bias and residual add epilogues"""
    from denet_amd import ops
    N, H, W, C, K = shape
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, H, W, C, device="cuda", generator=g)
    w = torch.randn(K, 3, 3, C, device="cuda", generator=g) * 0.1
    bias = torch.randn(K, device="cuda", generator=g)
    add = torch.randn(N, H, W, K, device="cuda", generator=g)
    dy = torch.randn(N, H, W, K, device="cuda", generator=g)
    addx = torch.randn(N, H, W, C, device="cuda", generator=g)
    tol = 2e-5 if tile == 2 else 1e-4
    with ops.switches(AUTOTUNE=False):
        ref = ops.conv_fwd(x, w, bias=bias, add=add, stride=1, pad=1)
        got = ops.conv_wino_fwd(x, w, bias=bias, add=add, tile=tile)
        assert float((ref - got).abs().max()) <= tol * float(ref.abs().max())
        ref2 = ops.conv_fwd(x, w, stride=1, pad=1)
        got2 = ops.conv_wino_fwd(x, w, tile=tile)
        assert float((ref2 - got2).abs().max()) <= tol * float(ref2.abs().max())
        rd = ops.conv_dgrad(dy, w, tuple(x.shape), add=addx, stride=1, pad=1)
        gd = ops.conv_wino_dgrad(dy, w, add=addx, tile=tile)
        assert float((rd - gd).abs().max()) <= tol * float(rd.abs().max())
        rw = ops.conv_wgrad(x, dy, tuple(w.shape), stride=1, pad=1)
        gw = ops.conv_wino_wgrad(x, dy, tile=tile)
        assert float((rw - gw).abs().max()) <= 3 * tol * float(rw.abs().max())


def _linked_case(case, tile, backward):
    """random operands of a batch norm linked into the Winograd transforms of a 3x3 convolution C -> K on an N x H x W map; the
    batch norm sits on the convolution's input (forward: C channels) or on its output gradient (backward: K channels)"""
    N, H, W, C, K = case
    gen = torch.Generator().manual_seed(sum(case) + 10 * tile + int(backward))
    ch = K if backward else C
    t = {"w": (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda(),
         "x": torch.randn(N, H, W, ch, generator=gen).cuda(),        # the batch norm's input
         "aux": torch.randn(N, H, W, ch, generator=gen).cuda(),      # forward: residual input; backward: gradient of its output
         "y": torch.randn(N, H, W, ch, generator=gen).cuda(),        # backward: forward output (only its sign is read)
         "xin": torch.randn(N, H, W, C, generator=gen).cuda(),       # backward: the convolution's input (filter gradient)
         "gamma": (torch.rand(ch, generator=gen) + 0.5).cuda(), "beta": torch.randn(ch, generator=gen).cuda(),
         "mean": (torch.randn(ch, generator=gen) * 0.3).cuda(), "invstd": (torch.rand(ch, generator=gen) + 0.5).cuda(),
         "coef": (torch.randn(2, ch, generator=gen) * 0.1).cuda()}
    return t


_LINKED_CASES = [(2, 8, 8, 32, 32), (1, 20, 12, 64, 32), (2, 7, 10, 32, 64), (1, 32, 32, 64, 64)]


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("case", _LINKED_CASES)
def test_linked_forward_transform_equals_the_separate_kernels(hip, case, tile):
    """denet_conv_wino_fwd_fold (the batch norm in front evaluated inside the input transform, wino_prep_lds_kernel) against
    denet_bn_apply + denet_conv_wino_fwd, through the C ABI, bit for bit: the activation, the transformed input V and y. Maps:
    a 2 x 2 tile grid inside one 4 x 4 tile block; partial blocks on both axes with two channel blocks; a map that is no multiple
    of either tile; full blocks. Plain, with ReLU, with ReLU and a residual input."""
    import ctypes
    from denet_amd import ops
    N, H, W, C, K = case
    t = _linked_case(case, tile, False)
    L = ops._L()
    T = N * -(-H // tile) * -(-W // tile)
    nv = (tile + 2) ** 2 * T * C
    ws = ops._wino_ws(tile, N, H, W, C, K)
    for relu, res in ((0, 0), (1, 0), (1, 1)):
        link = ops.BnLink(False, t["x"], t["aux"] if res else None, None, t["gamma"], t["beta"], t["mean"], t["invstd"], None, relu)
        act = torch.full_like(t["x"], float("nan"))
        v1, v2 = (torch.full((nv,), float("nan"), device="cuda") for _ in range(2))
        y1, y2 = (torch.full((N, H, W, K), float("nan"), device="cuda") for _ in range(2))
        bn = link.c_struct(act)
        ops.check(L.denet_conv_wino_fwd_fold(ctypes.byref(bn), ops.ptr(t["w"]), None, ops.ptr(v1), None, None, ops.ptr(y1), 0, None, 0,
                                             None, ops.ptr(ws), ws.numel(), tile, N, H, W, C, K, ops.stream_ptr()), "conv_wino_fwd_fold")
        ref = link.materialise()
        ops.check(L.denet_conv_wino_fwd(ops.ptr(ref), ops.ptr(t["w"]), None, ops.ptr(v2), None, None, ops.ptr(y2), ops.ptr(ws),
                                        ws.numel(), tile, N, H, W, C, K, ops.stream_ptr()), "conv_wino_fwd")
        assert torch.equal(act, ref), (relu, res)
        assert torch.equal(v1, v2), (relu, res)
        assert torch.equal(y1, y2), (relu, res)
        assert bool(torch.isfinite(y1).all())


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("case", _LINKED_CASES)
def test_linked_backward_transform_equals_the_separate_kernels(hip, case, tile):
    """denet_conv_wino_dgrad_fold + denet_conv_wino_wgrad_dm (the backward pointwise pass of the batch norm behind the
    convolution evaluated inside the transform kernel, which writes V and dM = A d A^T) against denet_bn_bwd_apply +
    denet_conv_wino_dgrad + denet_conv_wino_wgrad, through the C ABI, bit for bit: dx, the residual-branch gradient, dw. Without
    ReLU; with the mask recomputed from x; with the mask from the forward output (the last two with dres)."""
    import ctypes
    from denet_amd import ops
    N, H, W, C, K = case
    t = _linked_case(case, tile, True)
    L = ops._L()
    T = N * -(-H // tile) * -(-W // tile)
    ws = ops._wino_ws(tile, N, H, W, C, K)
    sws = ops.WS.get("wgrad", ops.WGRAD_WS_BYTES)
    for relu, from_y, want_dres in ((0, 0, 0), (1, 0, 1), (1, 1, 1)):
        def link(dres):
            return ops.BnLink(True, t["x"], t["aux"], t["y"] if from_y else None, t["gamma"], t["beta"], t["mean"], t["invstd"],
                              t["coef"], relu, out=dres)
        dres1, dres2 = ((torch.full_like(t["x"], float("nan")) if want_dres else None) for _ in range(2))
        dm = torch.full(((tile + 2) ** 2 * T * K,), float("nan"), device="cuda")
        dx1, dx2 = (torch.full((N, H, W, C), float("nan"), device="cuda") for _ in range(2))
        dw1, dw2 = (torch.full((K, 3, 3, C), float("nan"), device="cuda") for _ in range(2))
        l1 = link(dres1)
        bn = l1.c_struct(l1.out)
        ops.check(L.denet_conv_wino_dgrad_fold(ctypes.byref(bn), ops.ptr(dm), ops.ptr(t["w"]), None, None, ops.ptr(dx1), None, None, 0,
                                               None, ops.ptr(ws), ws.numel(), tile, N, H, W, C, K, None, ops.stream_ptr()),
                  "conv_wino_dgrad_fold")
        ops.check(L.denet_conv_wino_wgrad_dm(ops.ptr(t["xin"]), ops.ptr(dm), None, ops.ptr(dw1), ops.ptr(ws), ws.numel(), ops.ptr(sws),
                                             sws.numel(), tile, N, H, W, C, K, ops.stream_ptr()), "conv_wino_wgrad_dm")
        d = link(dres2).materialise()
        ops.check(L.denet_conv_wino_dgrad(ops.ptr(d), ops.ptr(t["w"]), None, None, ops.ptr(dx2), ops.ptr(ws), ws.numel(), tile, N, H, W,
                                          C, K, ops.stream_ptr()), "conv_wino_dgrad")
        ops.check(L.denet_conv_wino_wgrad(ops.ptr(t["xin"]), ops.ptr(d), None, ops.ptr(dw2), ops.ptr(ws), ws.numel(), ops.ptr(sws),
                                          sws.numel(), tile, N, H, W, C, K, ops.stream_ptr()), "conv_wino_wgrad")
        assert torch.equal(dx1, dx2), (relu, from_y)
        assert torch.equal(dw1, dw2), (relu, from_y)
        if want_dres:
            assert torch.equal(dres1, dres2), (relu, from_y)
        assert bool(torch.isfinite(dx1).all()) and bool(torch.isfinite(dw1).all())


@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("kc", [(32, 64), (96, 32)])
def test_data_gradient_filters_are_the_transform_of_the_rotated_filters(hip, kc, tile):
    """conv_wino_filter(dgrad=True), U'[xi][c][k] through the LDS transposition of wino_filter_dgrad_kernel, is bit for bit the
    forward transform of the filters with the taps rotated by 180 degrees and the channel roles swapped"""
    from denet_amd import ops
    K, C = kc
    gen = torch.Generator().manual_seed(K + C + tile)
    w = torch.randn(K, 3, 3, C, generator=gen).cuda()
    ud = ops.conv_wino_filter(w, tile, True)
    uf = ops.conv_wino_filter(w.flip(1, 2).permute(3, 1, 2, 0).contiguous(), tile, False)
    assert ud.numel() == uf.numel() == (tile + 2) ** 2 * K * C
    assert torch.equal(ud.reshape(-1), uf.reshape(-1))


def test_filter_transform_rejects_channel_counts_no_pass_accepts(hip):
    """denet_conv_wino_filter with C = 24: DENET_ERR_ARG and a message, nothing launched (the buffer keeps its contents)"""
    from denet_amd import ops
    L = ops._L()
    w = torch.randn(32, 3, 3, 24).cuda()
    for tile in (2, 4):
        for dgrad in (0, 1):
            u = torch.full(((tile + 2) ** 2 * 32 * 24,), 7.0, device="cuda")
            assert L.denet_conv_wino_filter(ops.ptr(w), ops.ptr(u), tile, dgrad, 24, 32, ops.stream_ptr()) == -1000
            assert b"multiples" in L.denet_last_error()
            torch.cuda.synchronize()
            assert bool((u == 7.0).all())
