"""Opt-in bilinear RoI sampling of the DNS layer (tapRule 2, `DNS.I`; csrc/sparse_bilinear.hip) on the GPU, against the definition
of DESIGN.md section 16 restated here in plain numpy: coordinates in np.float32, operation by operation; weights and sums in
float64. The reference implementation has no such mode, so this file holds the contract.

Tolerance, per element, from the reference alone: |got - ref| <= (n + 4) * 2^-23 * A, A = float64 sum of |w * value| over the
element's terms, n = their number (4 in the forward pass, the length of the cell's slot list in the gradient): twice the fp32 bound
of a left-to-right sum with rounded weights and products. The largest observed err / bound is printed (pytest -s)."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from denet_amd import ops
from denet_amd.layer import set_train
from denet_amd.model import audit, model_cnn, zoo

F32 = np.float32
EPS = 2.0 ** -23
RATIOS = {}


# ---- the definition in numpy ---------------------------------------------------------------------------

def ref_axis(p0, ext, gs, size):
    """one axis of every tap of every box: fp32 coordinate f [M, gs], cells i0, i1 and the fp32-exact fraction t = f - i0"""
    i = np.arange(gs, dtype=F32)[None, :]
    p0, ext = np.asarray(p0, F32)[:, None], np.asarray(ext, F32)[:, None]
    num = (i * ext).astype(F32)
    q = (num / F32(gs - 1)).astype(F32)
    p = (p0 + q).astype(F32)
    f = (p * F32(size)).astype(F32)
    f = np.maximum(F32(0), np.minimum(f, F32(size - 1))).astype(F32)
    i0 = np.floor(f).astype(np.int64)
    t = (f - np.floor(f)).astype(F32)
    assert np.array_equal(t.astype(np.float64), f.astype(np.float64) - i0)           # exact in fp32
    i1 = np.minimum(i0 + 1, size - 1)
    return f, i0, i1, t


def ref_taps(bbox, gs, H, W):
    """cells [M, ntap, 4] (q = (y0,x0), (y0,x1), (y1,x0), (y1,x1)), float64 weights, fp32 weights as the kernel forms them,
    box height / width in fp32, and the fp32 coordinates (fy, fx)"""
    bbox = np.asarray(bbox, F32)
    bw, bh = (bbox[:, 2] - bbox[:, 0]).astype(F32), (bbox[:, 3] - bbox[:, 1]).astype(F32)
    fy, ya, yb, ty = ref_axis(bbox[:, 1], bh, gs, H)
    fx, xa, xb, tx = ref_axis(bbox[:, 0], bw, gs, W)
    M = len(bbox)
    ys = np.stack([ya, ya, yb, yb], -1)[:, :, None, :]                     # [M, gs(y), 1, 4]
    xs = np.stack([xa, xb, xa, xb], -1)[:, None, :, :]                     # [M, 1, gs(x), 4]
    cells = (ys * W + xs).reshape(M, gs * gs, 4)
    ty64, tx64 = ty.astype(np.float64), tx.astype(np.float64)
    wy = np.stack([1 - ty64, 1 - ty64, ty64, ty64], -1)[:, :, None, :]
    wx = np.stack([1 - tx64, tx64, 1 - tx64, tx64], -1)[:, None, :, :]
    w64 = (wy * wx).reshape(M, gs * gs, 4)
    wy32 = np.stack([(F32(1) - ty).astype(F32)] * 2 + [ty] * 2, -1)[:, :, None, :]
    wx32 = np.stack([(F32(1) - tx).astype(F32), tx] * 2, -1)[:, None, :, :]
    w32 = (wy32 * wx32).astype(F32).reshape(M, gs * gs, 4)
    return cells, w64, w32, bh, bw, (fy, fx)


def ref_forward(feat, bbox, rois, gs):
    """feat [B, H, W, F] (the sampled channels) -> float64 features [M, ntap * F] and the bound's A, same shape"""
    B, H, W, Fc = feat.shape
    cells, w64, _, _, _, _ = ref_taps(bbox, gs, H, W)
    M = len(bbox)
    ref = np.zeros((M, gs * gs, Fc))
    A = np.zeros((M, gs * gs, Fc))
    f64 = feat.reshape(B, H * W, Fc).astype(np.float64)
    for m in range(M):
        v = f64[m // rois][cells[m]]                                       # [ntap, 4, F]
        term = w64[m][:, :, None] * v
        ref[m], A[m] = term.sum(1), np.abs(term).sum(1)
    return ref.reshape(M, -1), A.reshape(M, -1)


def ref_backward(dy, bbox, rois, gs, H, W, Fc):
    """dy [M, KP] -> float64 gradient [B, H*W, F], the bound's A and the slot count n [B, H*W] of every cell"""
    M = len(bbox)
    B, ntap = M // rois, gs * gs
    cells, w64, _, _, _, _ = ref_taps(bbox, gs, H, W)
    rows = dy[:, :ntap * Fc].astype(np.float64).reshape(B, rois * ntap, Fc)
    ref, A, n = np.zeros((B, H * W, Fc)), np.zeros((B, H * W, Fc)), np.zeros((B, H * W), np.int64)
    for b in range(B):
        S = np.zeros((H * W, rois * ntap))                                 # S[cell, roi * ntap + tap] = the weights that meet there
        c = cells[b * rois:(b + 1) * rois].reshape(-1, 4)
        w = w64[b * rois:(b + 1) * rois].reshape(-1, 4)
        col = np.arange(rois * ntap)
        for q in range(4):
            np.add.at(S, (c[:, q], col), w[:, q])
            np.add.at(n[b], c[:, q], 1)
        ref[b], A[b] = S @ rows[b], S @ np.abs(rows[b])                     # (weights are >= 0: |w * v| = w * |v|)
    return ref, A, n


def check_bound(name, got, ref, A, n):
    bound = (n + 4) * EPS * A
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("sparse_bilinear %s: largest err / bound = %.4f (largest n = %d)" % (name, ratio, int(np.max(n))))
    bad = err > bound
    assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()), ratio)


# ---- kernel level -------------------------------------------------------------------------------------------------------------

def boxes_a(H, W, gs):
    """the crafted set of the 5 x 7 shapes, 6 boxes per image"""
    special = [(-0.2, -0.1, 1.3, 1.2),              # reaches outside [0, 1] on each side: clamping
               (0.4, 0.6, 0.4, 0.6),                # zero extent
               (0.25, 0.5, 1.0, 1.0),               # far edge: f = size - 1 exactly
               (0.0, 0.0, 2.0 / W, 2.0 / H),        # all-integral coordinates: f = 0, 1, 2 on both axes
               (0.13, 0.21, 0.58, 0.77),
               (0.05, 0.02, 0.93, 0.97)]
    rng = np.random.RandomState(8)
    second = [(x0, y0, x0 + rng.uniform(0, 1 - x0), y0 + rng.uniform(0, 1 - y0)) for x0, y0 in rng.uniform(0, 1, (6, 2))]
    return np.array(special + second, F32)


def random_boxes(M, H, W, seed):
    rng = np.random.RandomState(seed)
    bbox = np.zeros((M, 4), F32)
    for m in range(M):
        x0, y0 = rng.uniform(0, 1), rng.uniform(0, 1)
        bbox[m] = (x0, y0, rng.uniform(x0, 1), rng.uniform(y0, 1))
    for m in range(0, M, 3):             # detector-style boxes on the cell lattice
        c = rng.randint(0, W, 4)
        bbox[m] = (min(c[0], c[2]) / W, min(c[1], c[3]) / H, (max(c[0], c[2]) + 1) / W, (max(c[1], c[3]) + 1) / H)
    return bbox


SHAPES = {"odd_map_aligned": (2, 5, 7, 32, 4, 8, 3, 6, "A"),
          "odd_map_dnc_c_offset": (2, 5, 7, 32, 5, 8, 3, 6, "A"),
          "test_sparse_fwd_bwd_geometry": (3, 16, 16, 64, 4, 32, 7, 36, "random"),
          "three_kernel_grouping": (1, 16, 16, 32, 4, 8, 7, 576, "random")}


def _case(name):
    B, H, W, CP, coff, Fc, gs, rois, kind = SHAPES[name]
    rng = np.random.RandomState(len(name))
    bbox = boxes_a(H, W, gs) if kind == "A" else random_boxes(B * rois, H, W, 1 + rois)
    assert len(bbox) == B * rois
    feat = rng.uniform(-5, 5, (B, H, W, Fc)).astype(F32)
    fmap = rng.uniform(-9, 9, (B, H, W, CP)).astype(F32)       # the other channels hold values a wrong offset would pick up
    fmap[..., coff:coff + Fc] = feat
    KP = ((gs * gs * Fc + 2 + 31) // 32) * 32
    dy = rng.uniform(-1, 1, (B * rois, KP)).astype(F32)
    return B, H, W, CP, coff, Fc, gs, rois, bbox, feat, fmap, KP, dy


def test_boxes_a_hold_the_required_cases():
    H, W, gs = 5, 7, 3
    bbox = boxes_a(H, W, gs)
    _, _, _, _, _, (fy, fx) = ref_taps(bbox, gs, H, W)
    assert bbox[0, 0] < 0 and bbox[0, 1] < 0 and bbox[0, 2] > 1 and bbox[0, 3] > 1
    assert fx[0, 0] == 0 and fy[0, 0] == 0 and fx[0, -1] == W - 1 and fy[0, -1] == H - 1
    assert bbox[1, 0] == bbox[1, 2] and bbox[1, 1] == bbox[1, 3]
    assert fx[2, -1] == W - 1 and fy[2, -1] == H - 1 and fx[2, 0] < W - 1
    assert np.array_equal(fx[3], [0, 1, 2]) and np.array_equal(fy[3], [0, 1, 2])
    assert np.any(fx[4] != np.floor(fx[4])) and np.any(fy[4] != np.floor(fy[4]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernels_against_float64(hip, name):
    B, H, W, CP, coff, Fc, gs, rois, bbox, feat, fmap, KP, dy = _case(name)
    M, ntap = B * rois, gs * gs
    L = ops._L()
    if name == "three_kernel_grouping":
        assert rois * ntap * 4 == 112896 and L.denet_sparse_sort_is_single(B, H, W, rois * 4, gs) == 0
    else:
        assert L.denet_sparse_sort_is_single(B, H, W, rois * 4, gs) == 1
    fm_d, bb_d = torch.from_numpy(fmap).cuda(), torch.from_numpy(bbox).cuda()
    out, taps4, wts4 = ops.sparse_bilinear_fwd(fm_d, bb_d, coff, Fc, rois, gs, KP)
    cells, _, w32, bh, bw, _ = ref_taps(bbox, gs, H, W)
    assert np.array_equal(taps4.cpu().numpy().reshape(M, ntap, 4), cells)
    assert np.array_equal(wts4.cpu().numpy().reshape(M, ntap, 4), w32)                 # the fp32 weights, bit for bit
    got = out.cpu().numpy()
    ref, A = ref_forward(feat, bbox, rois, gs)
    check_bound("fwd " + name, got[:, :ntap * Fc], ref, A, 4)
    assert np.array_equal(got[:, ntap * Fc], bh) and np.array_equal(got[:, ntap * Fc + 1], bw)
    assert not got[:, ntap * Fc + 2:].any() and not np.signbit(got[:, ntap * Fc + 2:]).any()      # +0 padding
    # inference form: the same values, no arrays
    out2, t2, w2 = ops.sparse_bilinear_fwd(fm_d, bb_d, coff, Fc, rois, gs, KP, keep=False)
    assert t2 is None and w2 is None and torch.equal(out2, out)
    # the gradient
    zero_from = coff + Fc
    dfmap = torch.full((B, H, W, CP), 7.0).cuda()
    ops.sparse_bilinear_bwd(torch.from_numpy(dy).cuda(), taps4, wts4, dfmap, coff, Fc, rois, gs, zero_from)
    g = dfmap.cpu().numpy().reshape(B, H * W, CP)
    dref, dA, n = ref_backward(dy, bbox, rois, gs, H, W, Fc)
    check_bound("bwd " + name, g[:, :, coff:coff + Fc], dref, dA, n[:, :, None])
    assert np.all(g[:, :, zero_from:] == 0.0)
    assert np.all(g[:, :, :coff] == 7.0)
    assert int(n.sum()) == M * ntap * 4                      # zero-weight slots stay in the lists


def test_integral_coordinates_reduce_to_the_nearest_rule(hip):
    """corners on multiples of 1/8 and extents that are multiples of 2/8 on an 8 x 8 map with gs = 3: every coordinate is an exact
    integer (dyadic arithmetic; checked on the fp32 numpy coordinates), so the bilinear tap IS the nearest tap, bit for bit"""
    H = W = 8
    gs, Fc, CP, coff = 3, 8, 32, 4
    rng = np.random.RandomState(2)
    boxes = []
    for x0 in range(0, 8):
        for ext in (0, 2, 4, 6, 8):
            y0, ey = int(rng.randint(0, 8)), int(rng.choice([0, 2, 4, 6, 8]))
            boxes.append((x0 / 8.0, y0 / 8.0, (x0 + ext) / 8.0, (y0 + ey) / 8.0))
    bbox = np.array(boxes, F32)
    rois, B = len(boxes) // 2, 2
    _, _, _, _, _, (fy, fx) = ref_taps(bbox, gs, H, W)
    assert np.array_equal(fx, np.floor(fx)) and np.array_equal(fy, np.floor(fy))
    assert len(np.unique(fx)) == 8 and len(np.unique(fy)) == 8
    fmap = torch.from_numpy(rng.uniform(-5, 5, (B, H, W, CP)).astype(F32)).cuda()
    KP = ((gs * gs * Fc + 2 + 31) // 32) * 32
    bb = torch.from_numpy(bbox).cuda()
    near, taps = ops.sparse_fwd(fmap, bb, coff, Fc, rois, gs, KP, tap_rule=0)
    out, taps4, wts4 = ops.sparse_bilinear_fwd(fmap, bb, coff, Fc, rois, gs, KP)
    assert np.array_equal(out.cpu().numpy(), near.cpu().numpy())
    assert np.array_equal(taps4.cpu().numpy().reshape(B * rois, gs * gs, 4)[..., 0], taps.cpu().numpy())
    w = wts4.cpu().numpy().reshape(B * rois, gs * gs, 4)
    assert np.all(w[..., 0] == 1.0) and not w[..., 1:].any()


def _grad_case(name):
    B, H, W, CP, coff, Fc, gs, rois, bbox, feat, fmap, KP, dy = _case(name)
    out, taps4, wts4 = ops.sparse_bilinear_fwd(torch.from_numpy(fmap).cuda(), torch.from_numpy(bbox).cuda(), coff, Fc, rois, gs, KP)
    return (B, H, W, CP, coff, Fc, gs, rois, KP), fmap, out, taps4, wts4, torch.from_numpy(dy).cuda()


def test_adjointness(hip):
    """<gather(fmap), dy> = <fmap, gather^T(dy)> over the feature channels, both sides from the device results, summed in
    float64: 1e-5 relative (the fp32 budget of sums of a few thousand terms)"""
    (B, H, W, CP, coff, Fc, gs, rois, KP), fmap, out, taps4, wts4, dy = _grad_case("test_sparse_fwd_bwd_geometry")
    ntap = gs * gs
    dfmap = torch.zeros(B, H, W, CP).cuda()
    ops.sparse_bilinear_bwd(dy, taps4, wts4, dfmap, coff, Fc, rois, gs, coff + Fc)
    lhs = float(np.sum(out.cpu().numpy()[:, :ntap * Fc].astype(np.float64) * dy.cpu().numpy()[:, :ntap * Fc].astype(np.float64)))
    rhs = float(np.sum(fmap[..., coff:coff + Fc].astype(np.float64) * dfmap.cpu().numpy()[..., coff:coff + Fc].astype(np.float64)))
    scale = float(np.sum(np.abs(out.cpu().numpy()[:, :ntap * Fc].astype(np.float64) * dy.cpu().numpy()[:, :ntap * Fc].astype(np.float64))))
    print("sparse_bilinear adjointness: lhs %.9g rhs %.9g, |lhs - rhs| / sum|terms| = %.3g" % (lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("Fc", [8, 32])
def test_summation_order_is_pinned(hip, Fc):
    """the slots s' = (roi * ntap + tap) * 4 + q of a cell in ascending order; entry j in chain j % epi,
    epi = 64 // (F / 4); a chain adds fl(w * row) left to right from +0; the chains are added in order - emulated in numpy float32.
    Clustered boxes put hundreds of slots on a cell (more than one chunk of 64 per cell)"""
    rng = np.random.RandomState(4)
    B, H, W, rois, gs = 2, 12, 12, 150, 5
    CP = ((Fc + 31) // 32) * 32
    M, ntap = B * rois, gs * gs
    cx, cy = rng.normal(0.5, 0.06, M), rng.normal(0.5, 0.06, M)
    w, h = rng.uniform(0.02, 0.15, M), rng.uniform(0.02, 0.15, M)
    bbox = np.clip(np.stack([cx - w, cy - h, cx + w, cy + h], 1), 0, 1).astype(F32)
    fmap = torch.zeros(B, H, W, CP).cuda()
    KP = ((ntap * Fc + 2 + 31) // 32) * 32
    _, taps4, wts4 = ops.sparse_bilinear_fwd(fmap, torch.from_numpy(bbox).cuda(), 0, Fc, rois, gs, KP)
    dy = rng.uniform(-1, 1, (M, KP)).astype(F32)
    dfmap = torch.zeros(B, H, W, CP).cuda()
    ops.sparse_bilinear_bwd(torch.from_numpy(dy).cuda(), taps4, wts4, dfmap, 0, Fc, rois, gs, Fc)
    got = dfmap.cpu().numpy().reshape(B, H * W, CP)
    tp = taps4.cpu().numpy().reshape(B, rois * ntap * 4)
    wt = wts4.cpu().numpy().reshape(B, rois * ntap * 4)
    epi = 64 // (Fc // 4)
    most = 0
    for b in range(B):
        for cell in range(H * W):
            slots = np.nonzero(tp[b] == cell)[0]                      # ascending slot
            most = max(most, len(slots))
            chains = [np.zeros(Fc, F32) for _ in range(epi)]
            for j, sl in enumerate(slots):
                roi, tap = divmod(int(sl) >> 2, ntap)
                prod = (wt[b, sl] * dy[b * rois + roi, tap * Fc:(tap + 1) * Fc]).astype(F32)
                chains[j % epi] = chains[j % epi] + prod
            tot = chains[0]
            for k in range(1, epi):
                tot = tot + chains[k]
            assert np.array_equal(got[b, cell, :Fc], tot), (b, cell, len(slots))
    assert most > 128


def test_gradient_does_not_depend_on_scheduling(hip):
    """the gradient of the 16 x 16 shape three times: grouped ahead on a side stream (presorted), and twice beside a stream that
    keeps the memory system busy - bit-identical"""
    (B, H, W, CP, coff, Fc, gs, rois, KP), fmap, out, taps4, wts4, dy = _grad_case("test_sparse_fwd_bwd_geometry")
    L = ops._L()
    side = torch.cuda.Stream()
    ws = ops._sparse_bilinear_ws(B, H, W, rois, gs)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.check(L.denet_sparse_bilinear_sort(ops.ptr(taps4), ops.ptr(ws), ws.numel(), B, H, W, rois, gs, ops.stream_ptr()), "sort")
        ev = torch.cuda.Event()
        ev.record(side)
    results = []
    d0 = torch.full((B, H, W, CP), 3.0).cuda()
    ops.sparse_bilinear_bwd(dy, taps4, wts4, d0, coff, Fc, rois, gs, coff + Fc, presorted=ev)
    results.append(d0.cpu().numpy())
    a, b = torch.empty(1 << 24, device="cuda"), torch.empty(1 << 24, device="cuda")
    for _ in range(2):
        with torch.cuda.stream(side):
            for _ in range(40):
                b.copy_(a, non_blocking=True)
        d = torch.full((B, H, W, CP), 3.0).cuda()
        ops.sparse_bilinear_bwd(dy, taps4, wts4, d, coff, Fc, rois, gs, coff + Fc)
        results.append(d.cpu().numpy())
    side.synchronize()
    assert results[0][..., coff:coff + Fc].any()
    for r in results[1:]:
        assert np.array_equal(results[0].view(np.uint32), r.view(np.uint32))


# ---- through the layer --------------------------------------------------------------------------------------------------------

B_, IMG = 2, 128


def _model(tag="DNS.I", seed=1):
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "%s[7,24,0.01,0.1]" % tag)
    model = zoo.denet34(B_, "skip", IMG, class_num=80, seed=seed, head_desc=desc)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    return model, by_type("denet-corner"), by_type("denet-sparse"), by_type("denet-detect")


def _layer_feat(fmap, dnc):
    return fmap.cpu().numpy()[..., dnc.corner_num:dnc.corner_num + dnc.sample_feat]


def test_layer_forward_and_backward(hip):
    """DeNet-34 skip with DNS.I, B = 2, 128 x 128: a crafted RoI list through set_samples, forward and backward of the layer
    against the definition evaluated on the corner layer's own sampling map"""
    model, dnc, dns, _ = _model()
    assert dns.tap_rule == 2
    x, _ = zoo.synthetic_batch(B_, IMG, seed=3)
    model.forward(x, None, train=True, stop_after=dnc)            # (no targets: only the sampling map is needed)
    S, gs = dns.sample_count, dns.grid_size
    rng = np.random.RandomState(12)
    lists = []
    for b in range(B_):
        bx = random_boxes(S - 40 * b, dnc.height, dnc.width, 20 + b)          # image 1 has a shorter list: the rest stays 0
        lists.append([(float(rng.uniform()), tuple(float(v) for v in r)) for r in bx])
    set_train(True)
    arr = dns.set_samples(lists)
    dns.forward(None)
    bbox = arr.reshape(-1, 4)
    fmap, coff, Fc = dnc.sample_map()
    feat = _layer_feat(fmap, dnc)
    ntap = gs * gs
    got = dns.output.data.view(B_ * S, -1).cpu().numpy()
    ref, A = ref_forward(feat, bbox, S, gs)
    check_bound("layer fwd", got[:, :ntap * Fc], ref, A, 4)
    assert np.array_equal(got[:, ntap * Fc], (bbox[:, 3] - bbox[:, 1]).astype(F32)) and not got[:, ntap * Fc + 2:].any()
    grad = rng.uniform(-1, 1, got.shape).astype(F32)
    dns.output.grad = torch.from_numpy(grad).cuda().view(dns.output.data.shape)
    dnc.dconv = None
    dns.backward(None)
    g = dnc.dconv.cpu().numpy().reshape(B_, dnc.height * dnc.width, -1)
    dref, dA, n = ref_backward(grad, bbox, S, gs, dnc.height, dnc.width, Fc)
    check_bound("layer bwd", g[:, :, coff:coff + Fc], dref, dA, n[:, :, None])
    assert not g[:, :, coff + Fc:].any()


_ALONE = {}


def _train_alone(tag):
    """two steps of a model that has the process to itself while it steps; computed once per rule, shared by the tests below"""
    if tag not in _ALONE:
        _ALONE[tag] = _train(tag)
    return _ALONE[tag]


def _train(tag, steps=2, seed=1, lr=0.05):
    from tests.test_cluster_device_gpu import _params_of
    model, dnc, dns, _ = _model(tag, seed)
    model.build_train_func("nesterov")
    random.seed(9)
    costs, launches = [], []
    for it in range(steps):
        x, metas = zoo.synthetic_batch(B_, IMG, seed=3 + it)
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, it, lr, [0.9], 1e-4)
            dns.sample_bbox_list
        costs.append(cost)
        launches.append([s for s in ka.other if s.startswith("sparse_bilinear_")])
    torch.cuda.synchronize()
    return costs, launches, _params_of(model)


def test_training_steps_are_reproducible_and_use_the_kernels(hip):
    ca, la, wa = _train_alone("DNS.I")
    cb, lb, wb = _train("DNS.I")
    assert ca == cb and all(np.isfinite(ca)), (ca, cb)
    assert len(wa) == len(wb) > 0 and all(np.array_equal(a, b) for a, b in zip(wa, wb))
    for l in la + lb:
        assert sorted(l) == ["sparse_bilinear_bwd_kernel", "sparse_bilinear_fwd_kernel"], l
    c0, l0, w0 = _train_alone("DNS")
    assert l0 == [[], []]
    # the mode did something: the detection head's last layer starts from zero weights, so the FIRST cost cannot see the gathered
    # features under either rule; the first update makes it see them, and the second cost differs
    assert c0[1] != ca[1], (c0, ca)
    assert any(not np.array_equal(a, b) for a, b in zip(w0, wa))


def test_mode_off_is_untouched(hip):
    """a rule-0 model steps, a rule-2 model is built and steps in the same process, the rule-0 model steps again: costs and
    parameters equal those of a rule-0 model that took the two steps on its own, bit for bit, and its audits hold no
    sparse_bilinear_* launch. (The generators' states are put back after the rule-2 step: its RoI editing draws from them.)"""
    from tests.test_cluster_device_gpu import _params_of
    alone_costs, alone_launches, alone_w = _train_alone("DNS")
    model, dnc, dns, _ = _model("DNS")
    model.build_train_func("nesterov")
    random.seed(9)
    costs, launches = [], []
    for it in range(2):
        x, metas = zoo.synthetic_batch(B_, IMG, seed=3 + it)
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
            dns.sample_bbox_list
        costs.append(cost)
        launches.append([s for s in ka.other if s.startswith("sparse_bilinear_")])
        if it == 0:
            torch.cuda.synchronize()
            saved = (random.getstate(), np.random.get_state())
            ic, il, _ = _train("DNS.I", steps=1)
            assert len(il[0]) == 2 and np.isfinite(ic[0])
            random.setstate(saved[0])
            np.random.set_state(saved[1])
    torch.cuda.synchronize()
    assert launches == [[], []] and alone_launches == [[], []]
    assert costs == alone_costs, (costs, alone_costs)
    w = _params_of(model)
    assert len(w) == len(alone_w) > 0 and all(np.array_equal(a, b) for a, b in zip(w, alone_w))


def test_inference_and_the_model_file(hip, tmp_path):
    """a DNS.I model keeps rule 2 through .mdl.gz; get_detections runs on the reloaded model, makes no tap or weight arrays, and its
    gather equals the definition on the features kept by the proposal (sample_shared)"""
    model, _, _, _ = _model()
    zoo.warm_corner_head(model, bias=7.5)
    fname = str(tmp_path / "bilinear.mdl.gz")
    model_cnn.save_to_file(model, fname)
    loaded = model_cnn.load_from_file(fname, B_)
    by_type = lambda t: [l for l in loaded.layers if l.type_name == t][0]
    dnc, dns, dnd = by_type("denet-corner"), by_type("denet-sparse"), by_type("denet-detect")
    assert dns.tap_rule == 2 and dns.export_json()["tapRule"] == 2
    x, _ = zoo.synthetic_batch(B_, IMG, seed=11)
    res = dnd.get_detections(loaded, x, None, {"cornerThreshold": 0.01, "prThreshold": 0.01, "nmsThreshold": 0.5})
    assert len(res) == B_
    assert dns._taps is None and dns._wts is None
    assert sum(len(b) for b in dns.sample_boxes) > 0, "the warmed detector proposed nothing"
    S, gs, Fc = dns.sample_count, dns.grid_size, dnc.sample_feat
    bbox = dns.sample_bbox.cpu().numpy()
    got = dns.output.data.view(B_ * S, -1).cpu().numpy()
    ref, A = ref_forward(_layer_feat(dnc.sample_shared, dnc), bbox, S, gs)
    check_bound("inference fwd", got[:, :gs * gs * Fc], ref, A, 4)
    assert np.array_equal(got[:, gs * gs * Fc + 1], (bbox[:, 2] - bbox[:, 0]).astype(F32))
