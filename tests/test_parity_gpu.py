"""GPU parity of the hot path against the oracle (oracle/): every check goes through the C-ABI via the product's
host layer (denet_amd) and compares with the CPU restatement on the same seeded inputs.

  * RoI proposal (GPU build_samples) vs oracle C++: integer boxes bit-exact, order identical up to exact score ties
  * sparse gather taps bit-exact (both tap rules)
  * one/two full training steps of a reduced DeNet-34 skip and of the CIFAR 3-layer CNN vs the numpy oracle:
    activations / costs / updated parameters within 1e-3 relative, RoI lists bit-identical
  * full-size (B=32, 512x512) size-independent properties: determinism, sortedness, idempotence, gather checksum
"""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from denet_amd import lib, ops
from denet_amd.model import audit, zoo
from denet_amd.model.model_cnn import walk_layers as model_cnn_walk
from oracle import model as OM
from oracle import layers as OL


ELEMENTWISE = {}      # what -> (max-norm relative error, p99.99 of the element-wise statistic): tests print the worst at the end


def rel_close(a, b, rtol=1e-3, what="", atol=0.0, rtol_elem=None):
    """two clauses, both asserted:
      max-norm      max|a - b| <= rtol * max|b| (+ atol)
      element-wise  |a - b| <= rtol * (|b| + rms(b)) (+ atol) for 99.99 % of the elements (the 99.99th percentile of
                    |a - b| / (|b| + rms(b)); tensors of fewer than 10^4 elements: every element). The rms floor keeps sums that
                    cancel to ~0 from dominating; a max-norm bound alone lets small activations be 100 % wrong."""
    if np.size(a) >= (1 << 22) and np.asarray(a).dtype == np.float32 and np.asarray(b).dtype == np.float32:
        return _rel_close_large(np.asarray(a), np.asarray(b), rtol, what, atol, rtol_elem)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-12
    d = np.abs(a - b)
    err = d.max() if d.size else 0.0
    assert err <= rtol * scale + atol, "%s: max abs err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)
    if d.size == 0:
        return
    rms = float(np.sqrt(np.mean(b * b)))
    stat = (np.maximum(d - atol, 0.0) / (np.abs(b) + rms + 1e-30)).reshape(-1)
    q = float(np.quantile(stat, 0.9999)) if stat.size >= 10000 else float(stat.max())
    if what:
        prev = ELEMENTWISE.get(what.split(" ")[0], (0.0, 0.0))
        ELEMENTWISE[what.split(" ")[0]] = (max(prev[0], err / scale), max(prev[1], q))
    rtol_elem = rtol if rtol_elem is None else rtol_elem
    assert q <= rtol_elem, "%s: element-wise p99.99 of |a-b| / (|b| + rms) = %.3e > %.1e (max-norm rel %.2e, rms %.3e)" % (
        what, q, rtol_elem, err / scale, rms)


def _err_stats(a, b):
    """(element-wise p99.99 of |a - b| / (|b| + rms(b)), max|a - b| / max|b|): the two figures rel_close asserts on"""
    b = np.asarray(b, np.float64)
    d = np.abs(np.asarray(a, np.float64) - b)
    rms = float(np.sqrt(np.mean(b * b)))
    stat = (d / (np.abs(b) + rms + 1e-30)).reshape(-1)
    q = float(np.quantile(stat, 0.9999)) if stat.size >= 10000 else float(stat.max())
    return q, float(d.max() / (np.abs(b).max() + 1e-12))


def _rel_close_large(a, b, rtol, what, atol, rtol_elem):
    """rel_close for float32 tensors of millions of elements (the B = 32 steps: up to 134 M per activation) without the float64
    copies and the full sort: the difference of two nearby float32 values is exact in float32, the sums that need it accumulate
    in float64, the percentile is one partition of a float32 array. Same two clauses, same recorded figures."""
    a, b = a.reshape(-1), b.reshape(-1)
    absb = np.abs(b)
    scale = float(absb.max()) + 1e-12
    d = np.abs(a - b)
    err = float(d.max())
    assert err <= rtol * scale + atol, "%s: max abs err %.3e vs scale %.3e (rel %.2e)" % (what, err, scale, err / scale)
    rms = float(np.sqrt(np.sum(b * b, dtype=np.float64) / b.size))
    if atol:
        d = np.maximum(d - np.float32(atol), np.float32(0.0))
    absb += np.float32(rms + 1e-30)
    d /= absb
    k = min(d.size - 1, int(np.ceil(0.9999 * (d.size - 1))))
    q = float(np.partition(d, k)[k])       # (the upper neighbour of np.quantile's interpolation point: never smaller than it)
    if what:
        prev = ELEMENTWISE.get(what.split(" ")[0], (0.0, 0.0))
        ELEMENTWISE[what.split(" ")[0]] = (max(prev[0], err / scale), max(prev[1], q))
    rtol_elem = rtol if rtol_elem is None else rtol_elem
    assert q <= rtol_elem, "%s: element-wise p99.99 of |a-b| / (|b| + rms) = %.3e > %.1e (max-norm rel %.2e, rms %.3e)" % (
        what, q, rtol_elem, err / scale, rms)


def random_corner_map(rng, B, H, W, frac, Cn=4):
    """log-probability maps with roughly `frac` of the cells above the 0.01 threshold"""
    z = rng.randn(B, Cn, H, W).astype(np.float32) * 2.0
    thr = np.quantile(z, 1.0 - frac)
    x = (z - thr) * 1.5 - 2.2975        # logit offset so that sigma(2x') crosses 0.01 at the quantile
    pos = -np.logaddexp(0, -2 * x).astype(np.float32)      # log sigma(2x)
    neg = -np.logaddexp(0, 2 * x).astype(np.float32)
    return np.ascontiguousarray(np.stack([neg, pos], axis=1).astype(np.float32))


def _box_key(pr_map, b, box):
    """|pr_f - pr_t| of a candidate box as the reference evaluates it (denet_sparse.cc:276-303): sequential fp32 sums over the
    four corner cells in the order TL, TR, BL, BR (+ the centre cell of the 5-map variant)"""
    x0, y0, x1, y1 = box
    cells = [(0, y0, x0), (1, y0, x1), (2, y1, x0), (3, y1, x1)]
    if pr_map.shape[2] == 5:
        cells.append((4, (y0 + y1) // 2, (x0 + x1) // 2))
    sf = st = np.float32(0.0)
    for c, y, x in cells:
        sf = np.float32(sf + pr_map[b, 0, c, y, x])
        st = np.float32(st + pr_map[b, 1, c, y, x])
    return np.float32(abs(np.float32(sf - st)))


def check_samples(pr_map, thr, sn, maxc, lm):
    d = torch.from_numpy(pr_map).cuda()
    box, absd, cnt = ops.build_samples(d, thr, sn * sn, maxc, lm)
    box, absd, cnt = box.cpu(), absd.cpu(), cnt.cpu()
    got = ops.samples_finish_host(box, absd, cnt, pr_map.shape[3], pr_map.shape[4]).numpy()
    ref, rbox, rabsd, rcnt = OM.oracle_build_samples_raw(pr_map, thr, sn, maxc, lm)
    assert np.array_equal(cnt.numpy(), rcnt)
    box, absd = box.numpy(), absd.numpy()
    nties = 0
    for b in range(pr_map.shape[0]):
        n = rcnt[b]
        # scores: identical multiset, non-increasing
        assert np.array_equal(got[b, :n, 0], ref[b, :n, 0]), "score sequence differs"
        assert np.all(np.diff(absd[b, :n]) >= 0)
        # boxes: identical inside every group of equal score (order inside a tie group is unspecified)
        i = 0
        while i < n:
            j = i
            while j + 1 < n and ref[b, j + 1, 0] == ref[b, i, 0]:
                j += 1
            ga = sorted(map(tuple, box[b, i:j + 1].tolist()))
            gb = sorted(map(tuple, rbox[b, i:j + 1].tolist()))
            if j + 1 == n and n == sn * sn and ga != gb:
                # a tie group cut by the top-K boundary may keep different members - but only members that really HAVE the
                # boundary score: the key of every box one side kept and the other did not is recomputed from the map
                for bx in set(ga) ^ set(gb):
                    assert _box_key(pr_map, b, bx) == absd[b, i], ("a box without the boundary score at the cut", b, bx)
            else:
                assert ga == gb, "boxes differ at rank %d..%d" % (i, j)
            if j == i:
                assert np.array_equal(got[b, i], ref[b, i])
            nties += j - i
            i = j + 1
    return int(rcnt.sum()), nties


def reference_edit_of_the_products_proposal(dns, cl, metas, seed):
    """RoI lists of a training step against the reference, tie-aware: (1) the device proposal against the C++ oracle on the
    product's own corner map, group by group of equal score (check_samples; inside such a group the reference's
    std::partial_sort leaves the order open); (2) the editing (denet_sparse.py:184-201), which picks list
    POSITIONS with random.sample, replayed by the oracle on the product's proposal order. Returns (reference lists, number
    of detector boxes). An exact comparison with the oracle's own order fails whenever a corner map holds a tie group -
    which implementation a first step measures fastest varies from run to run at these sizes, and so does the map."""
    B = dns.batch_size
    total, _ = check_samples(cl.corner_pr.cpu().numpy(), dns.corner_threshold, dns.sample_num, 1024, int(dns.local_max))
    raw = dns._raw_samples
    lists = [[] for _ in range(B)] if raw is None else \
        [[(float(r[0]), tuple(float(v) for v in r[1:5])) for r in raw[0][b, :int(raw[1][b])]] for b in range(B)]
    assert sum(len(l) for l in lists) == total
    random.seed(seed)
    return OL.edit_samples(lists, metas, dns.sample_count, dns.random_sample, dns.sample_gt), total


@pytest.mark.parametrize("frac,lm", [(0.0, 0), (0.004, 0), (0.01, 0), (0.02, 1), (0.05, 2), (0.4, 0)])
def test_build_samples_vs_oracle(hip, frac, lm):
    rng = np.random.RandomState(int(frac * 1000) + lm)
    pr = random_corner_map(rng, 4, 64, 64, frac)
    total, ties = check_samples(pr, 0.01, 24, 1024, lm)
    if frac == 0.0:
        assert total == 0
    else:
        assert total > 0


@pytest.mark.parametrize("frac,lm", [(0.004, 0), (0.01, 1), (0.05, 0), (0.3, 0)])
def test_build_samples_center_variant_vs_oracle(hip, frac, lm):
    """DNC.C: five maps (TL, TR, BL, BR, centre); every centre proposes the boxes that have it as mid-point and one
    selected corner (denet_sparse.cc:374-466), the score adds the centre term (:296-303)"""
    rng = np.random.RandomState(int(frac * 1000) + lm + 50)
    pr_map = random_corner_map(rng, 3, 32, 48, frac, Cn=5)
    n, nties = check_samples(pr_map, 0.01, 12, 1024, lm)
    assert n > 0


def test_build_samples_truncation_and_small_k(hip):
    rng = np.random.RandomState(9)
    pr = random_corner_map(rng, 2, 64, 64, 0.5)        # > 1024 corners per type -> top-1024 by log-probability
    counts = np.zeros(8, np.int32)
    import ctypes
    f = OM.oracle_lib().oracle_count_corners
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    f(pr.ctypes.data, 2, 4, 64, 64, 0.01, 100000, 0, counts.ctypes.data)
    assert counts.min() > 1024
    check_samples(pr, 0.01, 24, 1024, 0)
    check_samples(pr, 0.01, 4, 64, 0)
    check_samples(random_corner_map(rng, 3, 16, 16, 0.1), 0.01, 24, 1024, 0)


def test_build_samples_exact_ties(hip):
    """hand-built ties: identical scores for many boxes -> same scores, same boxes per tie group"""
    P = np.full((1, 4, 16, 16), 1e-4, np.float64)
    for (x, y) in [(1, 1), (2, 1), (1, 2), (3, 3)]:
        P[0, 0, y, x] = 0.5
    for (x, y) in [(10, 10), (12, 10), (10, 12), (14, 14)]:
        P[0, 3, y, x] = 0.5
    pr = np.ascontiguousarray(np.stack([np.log(1 - P), np.log(P)], axis=1).astype(np.float32))
    total, ties = check_samples(pr, 0.01, 24, 1024, 0)
    assert total == 16 and ties > 0


@pytest.fixture(autouse=True)
def _materialised_stem_activation(request):
    """The teacher-forced comparisons read EVERY layer's output; training normally never writes relu(bn(x)) of a BN + ReLU layer
    whose only reader is a max pool (ops.BN_POOL_FUSE, bit-identical to the separate passes: test_kernels_gpu.py and
    test_bn_pool_fusion_leaves_training_unchanged below). The full-size property tests keep the product's default."""
    name = request.node.name
    if "full_size" in name or "fusion" in name or "cli" in name or "timed_batch" in name:
        yield
        return
    with ops.switches(BN_POOL_FUSE=False):
        yield


# tests that run on the MEASURED decisions (the committed tuned file at the benchmark geometries, or the tuner itself)
_MEASURED_TESTS = ("full_size", "measured", "timed_batch", "cli")


@pytest.fixture(autouse=True)
def _deterministic_algorithms(request):
    """Which implementation a convolution pass uses is a measured choice; at the small sizes of these tests the measurement is
    a timing race that ends differently from run to run, and so did the kernels a test covered. Every whole-network test of
    this file therefore runs under ops.static_policy (fused 64-channel kernels, else F(4x4), else F(2x2), else direct - the
    non-trivial path wherever one exists; no launch configuration is measured), except the tests at the benchmark geometries,
    which run what bench.py runs: the decisions of denet_amd/tuned/gfx950.json. The direct kernels at every layer are the
    subject of test_direct_and_measured_paths_agree and of the per-op tests (test_kernels_gpu.py, test_conv_fullsize_gpu.py)."""
    if any(k in request.node.name for k in _MEASURED_TESTS):
        yield
        return
    with ops.algorithms(POLICY=ops.static_policy):
        yield


KERNELS_RUN = {}       # test name -> audit summary (printed by the tests that assert on it)


def _is_3x3s1(geom):
    return " 3x3/1" in geom


def _chan(geom):
    c, k = geom.split(" ")[1].split("->")
    return int(c), int(k)


def _map(geom):
    return int(geom.split(" ")[0].split("x")[0])


def assert_kernels(table, batch, w4f=None, expect_w4f=None, expect_w4g=None):
    """per-layer assertions on a KernelAudit table of a DeNet-34 / ResNet-34 training step: WHICH kernel every 3x3 stride-1
    layer ran. expect_w4f(geom) / expect_w4g(geom) -> bool say where the fused F(4x4) product + output-transform kernel and
    the F(4x4) filter-gradient kernel must have run (None: the C side's default policy for this batch); w4f names the
    instantiation (32x2 / 32 / 64) when a test forces one."""
    seen = {"wino4f": 0, "wino4g": 0, "wino2f": 0, "wino4t": 0, "stem": 0}
    for r in table:
        g, fwd, bwd = r["geometry"], r["fwd"], r["bwd"]
        assert fwd, "layer %s (%s) launched no matrix kernel in the forward pass" % (r["layer"], g)
        if "7x7/2" in g and _chan(g)[0] == 3:
            assert fwd == ["stem_fwd_kernel"] and bwd == ["stem_wgrad_kernel"], (r["layer"], fwd, bwd)
            seen["stem"] += 1
            continue
        if not _is_3x3s1(g):
            # (the 3x3 stride-2 layers' data gradients: csrc/dgrad_s2.hip, the four parity classes in one workgroup)
            assert all(k.startswith("igemm_kernel<") or (k.startswith("dgrad_s2_kernel<") and " 3x3/2" in g) for k in fwd + bwd), (
                r["layer"], g, fwd, bwd)
            continue
        c, k = _chan(g)
        if c == 64 and k == 64:
            # the 64-channel stage: the fused F(2x2) kernels, or - where the tuned file says so (algorithm 44: the benchmark
            # geometry) - the tile-parallel fused F(4x4) kernel for the forward pass / the data gradient (csrc/wino4t.hip);
            # the filter gradient stays with the fused F(2x2) kernel
            assert fwd in (["wino2f_ws_kernel<false>"], ["wino4t_kernel<1>"]), (r["layer"], g, fwd)
            assert sorted(bwd) in (["wino2f_wgrad_kernel", "wino2f_ws_kernel<true>"], ["wino2f_wgrad_kernel", "wino4t_kernel<2>"],
                                   ["wino2f_wgrad_kernel", "wino4t_kernel<0>"]), (r["layer"], g, bwd)
            seen["wino2f"] += 1
            seen["wino4t"] += int(fwd[0].startswith("wino4t")) + int(any(x.startswith("wino4t") for x in bwd))
            continue
        T = batch * (_map(g) // 4) ** 2
        f4 = expect_w4f(g, T) if expect_w4f is not None else None
        g4 = expect_w4g(g, T) if expect_w4g is not None else None
        has_f4_f = any(x.startswith("wino4f_kernel") for x in fwd)
        has_f4_b = any(x.startswith("wino4f_kernel") for x in bwd)
        has_g4 = any(x.startswith("wino4g_kernel") for x in bwd)
        if f4 is not None:
            assert has_f4_f == f4 and has_f4_b == f4, "layer %s (%s): fused F(4x4) kernel %s, expected %s: fwd %s bwd %s" % (
                r["layer"], g, has_f4_f and has_f4_b, f4, fwd, bwd)
            if f4 and w4f:
                assert all(x.startswith("wino4f_kernel_%s<" % w4f) for x in fwd + bwd if x.startswith("wino4f")), (r["layer"], fwd, bwd)
        if g4 is not None:
            assert has_g4 == g4, "layer %s (%s): F(4x4) filter-gradient kernel %s, expected %s: %s" % (r["layer"], g, has_g4, g4, bwd)
        if not has_f4_f:
            # the un-fused Winograd pass: ONE batched launch of the forward implicit-GEMM kernel (the 36 / 16 components)
            assert len(fwd) == 1 and fwd[0].startswith("igemm_kernel<0,"), (r["layer"], g, fwd)
        seen["wino4f"] += int(has_f4_f and has_f4_b)
        seen["wino4g"] += int(has_g4)
    return seen


def _product_acts(model):
    out = {}
    for i, layer in enumerate(model.layers[1:], 1):
        a = layer.output
        if a.data is None:
            continue
        if a.data.dim() == 4:
            out[i] = ops.nhwc_to_nchw(a.data, a.shape[1]).cpu().numpy()
    return out


def _force_list(model):
    """the product's op outputs (NCHW numpy) in the order the oracle interpreter evaluates its ops"""
    def nchw(act):
        if act.data is None:
            # a tensor the product never writes (relu(bn(x)) of the stem when BN + ReLU + max pool run as one pass, ops.BN_POOL_FUSE:
            # the product default, kept by the test at the timed batch): not forced, the oracle continues with its own value
            return None
        return ops.nhwc_to_nchw(act.data, act.shape[1]).cpu().numpy()

    out = []
    for layer in model.layers[1:]:
        t = layer.type_name
        if t == "conv" and getattr(layer, "skip_behind", None) is not None and layer.output.data is None:
            out.append(None)              # the SKIP layer behind adds its tap in this convolution's epilogue: only the sum exists
        elif t == "batchnorm" and getattr(layer, "act_fused", False):
            out.append(None)              # `BN A` run as one fused pass: only the activation's output exists
        elif t in ("conv", "batchnorm", "batchnorm-relu", "pool", "pool-inv", "deconv", "border", "crop-mirror"):
            out.append(nchw(layer.output))
        elif t == "dropout":
            out.append(nchw(layer.output))        # parity runs are training steps (the test path is an identity)
        elif t == "activation":
            if layer.activation != "none":
                out.append(nchw(layer.output))
        elif t == "resnet":
            main, sc = layer._main(), layer._shortcut()
            for s in main:
                fused_tail = (s is main[-1])     # original: last BN fused with add+ReLU; pre-activation: the
                if s.type_name == "activation" and s.activation == "none":   # residual add rides in the last conv
                    continue
                out.append(None if fused_tail or (s.type_name == "batchnorm" and getattr(s, "act_fused", False)) else nchw(s.output))
            for s in sc:
                out.append(nchw(s.output))
            out.append(nchw(layer.output))
        elif t == "skip":
            if len(layer.layers) > 1:
                out.append(None)          # 1x1 projection of the tap: its epilogue already holds the skip add
            out.append(nchw(layer.output))
        elif t in ("denet-corner", "denet-detect"):
            out.append(nchw(layer.conv.output))
        elif t == "denet-sparse":
            out.append(nchw(layer.output))
    return out


def _param_pairs(model, om):
    def walk(layers):
        out = []
        for l in layers:
            if l.type_name == "deconv" or (l.type_name == "conv" and l.enabled):
                out.append(l.omega)
                if l.use_bias:
                    out.append(l.beta)
            elif l.type_name in ("batchnorm", "batchnorm-relu") and l.enabled:
                out += [l.omega, l.beta]
            out += walk([s for s in l.layers if s.type_name != "initial"])
        return out

    pp, op = walk(model.layers[1:]), om.params()
    assert len(pp) == len(op)
    for a, b in zip(pp, op):
        assert a.value.shape == b.v.shape
    # a conv bias directly in front of a batch norm has an analytically zero gradient
    # (also through a SKIP addition between the two: `C.B[384,3] SKIP[1] BNA` of papers/dss/denet101.sh:13)
    tops = model.layers
    for i, l in enumerate(tops[1:-1], 1):
        j = i + 1
        while j < len(tops) - 1 and tops[j].type_name == "skip":
            j += 1
        if l.type_name in ("conv", "deconv") and l.use_bias and tops[j].type_name in ("batchnorm", "batchnorm-relu"):
            l.beta.zero_grad_expected = l.omega
    return list(zip(pp, op))


def _bn_pairs(model, om):
    def walk(layers):
        out = []
        for l in layers:
            if l.type_name in ("batchnorm", "batchnorm-relu") and l.enabled:
                out.append(l)
            out += walk([s for s in l.layers if s.type_name != "initial"])
        return out

    a, b = walk(model.layers[1:]), om.bn_nodes()
    assert len(a) == len(b)
    return list(zip(a, b))


def _forced_step_check(model, om, x, metas, it, lr, mu, decay, solver, roi_lists, rtol=1e-3):
    """op-by-op parity: the oracle re-runs the step with every op output replaced by the product's tensor
    (identical inputs per op, identical ReLU masks), so forward, gradients, running statistics and the solver
    update are each compared without 40 layers of accumulated rounding in between."""
    grads = [(p, p.get_grad()) for p, _ in _param_pairs(model, om)]
    om.force = _force_list(model)
    n_forced = len(om.force)
    ocost, ocosts = om.train_step(x, metas, it, lr, mu, decay, solver, sample_override=roi_lists)
    om.force = None
    assert om._fpos == n_forced, "op order mismatch between product and oracle"
    worst = max(om.force_err, key=lambda e: e[1])
    assert worst[1] <= 2e-4, "per-op forward error %s" % (worst,)
    for (p, g), (_, o) in zip(grads, _param_pairs(model, om)):
        og = o.g if o.g is not None else np.zeros_like(o.v)
        atol = 0.0
        w = getattr(p, "zero_grad_expected", None)
        if w is not None:      # both sides hold only fp32 roundoff: bound it by the layer's weight-gradient scale
            atol = 1e-3 * float(np.abs(w.get_grad()).max()) * w.value[0].size ** 0.5
        rel_close(g, og, rtol, "it%d grad %s %s" % (it, p.name, g.shape), atol=atol)
    for p, o in _param_pairs(model, om):
        # updated value of a zero-gradient bias = lr * roundoff: same bound, scaled by the learning rate
        w = getattr(p, "zero_grad_expected", None)
        atol = 1e-6 if w is None else 1e-6 + lr * 1e-3 * float(np.abs(w.get_grad()).max()) * w.value[0].size ** 0.5 * 2
        if w is not None and solver == "adam":
            # adam divides the gradient by its own magnitude: a bias whose true gradient is zero (conv bias in front
            # of a BN) moves by +-lr per step on roundoff alone, on both sides - only that bound can be checked
            atol = 2.0 * lr
        rel_close(p.get_value(), o.v, rtol, "it%d updated %s" % (it, p.name), atol=atol)
        if w is not None and solver == "adam":
            o.v = p.get_value().copy()       # keep the noise-driven bias identical on both sides for the next step
    for l, n in _bn_pairs(model, om):
        rel_close(l.mean.get_value(), n["mean"], rtol, "running mean")
        rel_close(l.stdinv.get_value(), n["stdinv"], rtol, "running stdinv")
    return ocost, ocosts


def _warm_corner_head(model, bias, std, seed=3):
    """makes the corner detector fire: random corner filters + a lower bias (SURVEY §8d 'warm' regime)"""
    rng = np.random.RandomState(seed)
    dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
    conv, cn = dnc.layers[-1], dnc.corner_num
    w = conv.omega.get_value().copy()
    w[:cn] = rng.normal(0, std, w[:cn].shape)
    conv.omega.set_value(w)
    b = conv.beta.get_value().copy()
    b[:cn] = bias
    conv.beta.set_value(b)


def _denet34_skip_steps_vs_oracle(regime, B, IMG, steps, model=None, free_running=True):
    """free-running forward + teacher-forced forward / backward / solver of `steps` training steps against oracle/model.py
    (reference: ModelCNN.train_step, model_cnn.py:407-445, on papers/dss/denet34.sh:13-15)"""
    if model is None:
        model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    dns, dnc = by_type("denet-sparse"), by_type("denet-corner")
    # break the all-zero detect head so that its gradients are exercised
    rng = np.random.RandomState(5)
    dconv = by_type("denet-detect").layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    if regime == "warm":
        _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=2)
    om_free = OM.OracleModel(model.export_json(), B)      # free running
    om = OM.OracleModel(model.export_json(), B)           # teacher forced, op by op
    model.build_train_func("nesterov")
    lr, mu, decay = 0.05, 0.9, 1e-4
    for it in range(steps):
        random.seed(100 + it)
        cost, costs = model.train_step(x, metas, 0, it, lr, [mu], decay)
        roi_lists = dns.sample_bbox_list
        if regime == "warm":
            # the RoI proposal contract is exact on the SAME corner map: oracle C++ on the product's map
            ref_lists, total = reference_edit_of_the_products_proposal(dns, dnc, metas, 100 + it)
            if it == 0:
                assert total > 0, "warm regime produced no detector boxes"
            assert ref_lists == roi_lists, "RoI lists differ from the reference editing of the same proposal"
        if it == 0 and free_running:
            # free-running oracle: whole-network forward parity (1e-3 rel on activations and costs)
            random.seed(100 + it)
            if regime == "warm":
                fcost, fcosts = om_free.forward_costs(x, metas, sample_override=roi_lists)      # forward quantities only are compared
            else:
                fcost, fcosts = om_free.forward_costs(x, metas)
                assert om_free.sample_bbox_list == roi_lists, "RoI lists differ (cold: random boxes + GT injection)"
            ys, xs = om_free.taps
            taps_ref = (ys[:, :, None] * (IMG // 8) + xs[:, None, :]).reshape(ys.shape[0], -1)
            assert np.array_equal(dns._taps.cpu().numpy(), taps_ref)
            assert abs(cost - fcost) <= 1e-3 * abs(fcost), (cost, fcost)
            for c, oc in zip(costs, fcosts):
                assert abs(c - oc) <= 1e-3 * max(abs(oc), 1e-6), (costs, fcosts)
            for i, a in _product_acts(model).items():
                rel_close(a, om_free.acts[i], 1e-3, "activation L%d %s" % (i, model.layers[i].type_name))
            rel_close(dnc.corner_pr.cpu().numpy(), om_free.corner_pr, 1e-3, "corner_pr")
        # op-by-op forward + backward + solver parity
        ocost, ocosts = _forced_step_check(model, om, x, metas, it, lr, mu, decay, "nesterov", roi_lists)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)
        ys, xs = om.taps
        taps_ref = (ys[:, :, None] * (IMG // 8) + xs[:, None, :]).reshape(ys.shape[0], -1)
        assert np.array_equal(dns._taps.cpu().numpy(), taps_ref)


@pytest.mark.parametrize("regime", ["cold", "warm"])
def test_denet34_skip_train_step_vs_oracle(hip, regime):
    _denet34_skip_steps_vs_oracle(regime, 2, 128, 2)


@pytest.mark.parametrize("regime", ["cold", "warm"])
def test_denet34_std_train_step_vs_oracle(hip, regime):
    """the recipe's other DeNet-34 (papers/dss/denet34.sh:13-14, the non-skip MODEL_DESC: biased 3x3 convolutions behind the
    pool-inverse layers, no skip taps): same checks as the skip model"""
    _denet34_skip_steps_vs_oracle(regime, 2, 128, 2, model=zoo.denet34(2, "std", 128, class_num=80, seed=1))


def test_denet101_skip_train_step_vs_oracle(hip):
    """DeNet-101 skip (papers/dss/denet101.sh:13-15: bottleneck backbone, two skip taps, DNC[128,50], 24x24 RoIs), warm corner
    head: RoI lists against the reference editing of the same proposal, taps, teacher-forced step op by op. (No free-running
    comparison: 101 layers deep on 4x4 maps of one image, batch statistics over 16 values - the element-wise p99.99 of the last
    stage reaches 1.05e-3 at a max-norm of 3.8e-4; the wide model's test does the same.)"""
    _denet34_skip_steps_vs_oracle("warm", 1, 128, 1, model=zoo.denet101(1, "skip", 128, class_num=80, seed=1), free_running=False)


@pytest.mark.parametrize("regime", ["cold", "warm"])
def test_denet34_skip_512_train_step_vs_oracle(hip, regime):
    """the same at the resolution bench.py times (papers/dss/denet34.sh:13-15,42-43: 512x512, 64x64 corner maps, 576 RoIs per
    image), B = 2, one step, element-wise and max-norm. What runs at this batch (asserted per layer below): the fused 64-channel
    F(2x2) kernels, the first layer's kernels on 256-pixel rows, UN-fused F(4x4) on the 64x64 / 32x32 / 16x16 maps with the
    F(4x4) filter-gradient kernel where a layer has >= 64 tiles. The fused F(4x4) product + output-transform kernel does NOT
    launch at B = 2 under the default policy (too few tiles to fill the chip): its whole-network comparisons are
    test_denet34_skip_512_fused_kernels_vs_oracle (forced, B = 2) and test_denet34_skip_512_timed_batch_vs_oracle (B = 32)."""
    model = zoo.denet34(2, "skip", 512, class_num=80, seed=1)
    with audit.KernelAudit(model) as ka:
        _denet34_skip_steps_vs_oracle(regime, 2, 512, 1, model=model)
    seen = assert_kernels(ka.table, 2, expect_w4f=lambda g, T: False,
                          expect_w4g=lambda g, T: T >= 64 and _chan(g)[0] % 128 == 0 and _chan(g)[1] % 128 == 0)
    assert seen["wino2f"] == 6 and seen["stem"] == 1 and seen["wino4g"] >= 12, seen
    worst = sorted(ELEMENTWISE.items(), key=lambda kv: -kv[1][1])[:5]
    print("element-wise p99.99 / max-norm, worst five:", [(k, "%.2e" % v[1], "%.2e" % v[0]) for k, v in worst])


@pytest.mark.parametrize("mode,regime", [(33, "warm"), (32, "cold"), (64, "warm")])
def test_denet34_skip_512_fused_kernels_vs_oracle(hip, mode, regime):
    """DeNet-34 skip 512x512, B = 2, THROUGH the kernels bench.py times: the fused F(4x4) product + output-transform kernel
    (csrc/wino4f.hip) forced on in each of its three shapes (denet_conv_wino4f_mode 33 / 32 / 64: 32-tile blocks as two 4-wave
    workgroups per CU, as one 8-wave workgroup, 64-tile blocks) and the F(4x4) filter-gradient kernel (csrc/wino4g.hip) wherever
    the geometry allows - forward (bias / skip add / batch-norm statistics epilogues), data gradient (backward-sums epilogue,
    linked batch-norm gradient) and filter gradient of every 128...512-channel 3x3 layer, free-running + op-by-op teacher-forced
    against oracle/model.py, with the per-layer assertion that those kernels really ran. Reference: ModelCNN.train_step,
    model_cnn.py:407-445 on papers/dss/denet34.sh:13-15."""
    L = lib.load()
    model = zoo.denet34(2, "skip", 512, class_num=80, seed=1)
    old = (L.denet_conv_wino4f_mode(mode), L.denet_conv_wino4g_mode(1))
    try:
        with audit.KernelAudit(model) as ka:
            _denet34_skip_steps_vs_oracle(regime, 2, 512, 1, model=model)
    finally:
        L.denet_conv_wino4f_mode(old[0])
        L.denet_conv_wino4g_mode(old[1])
    name = {33: "32x2", 32: "32", 64: "64"}[mode]
    seen = assert_kernels(ka.table, 2, w4f=name,
                          expect_w4f=lambda g, T: _chan(g)[0] % 128 == 0 and _chan(g)[1] % 64 == 0,
                          expect_w4g=lambda g, T: T >= 64 and _chan(g)[0] % 128 == 0 and _chan(g)[1] % 128 == 0)
    # 128-channel stage: 7 layers (the strided first convolution is a direct kernel), 256: 11, 512: 5, the two up-sampling convolutions
    assert seen["wino4f"] == 25 and seen["wino2f"] == 6 and seen["stem"] == 1, seen
    KERNELS_RUN["fused_%d_%s" % (mode, regime)] = ka.summary()


def test_denet34_skip_512_timed_batch_vs_oracle(hip):
    """THE configuration bench.py times (BASELINE config 3: DeNet-34 skip, 512x512, B = 32, papers/dss/denet34.sh:13-15,42-43)
    against oracle/model.py: one training step, free-running forward (activations, corner map, costs: 1e-3 max-norm AND
    element-wise p99.99) + the op-by-op teacher-forced step (per-op forward error, every gradient, running statistics, the
    nesterov update). The kernels are the ones the committed tuned file selects - NOTHING is measured in this test (asserted: every
    3x3 pass has a decision before the step) - and the per-layer audit asserts what the bench's roofline line describes: fused
    F(4x4) on the 64x64 / 32x32 maps (l2, l3, up1, up2) with the F(4x4) filter-gradient kernel, the fused F(2x2) kernels on the
    64-channel stage, the first layer's own kernels, un-fused F(4x4) on the 16x16 maps. ~50 s of CPU oracle per pass.
    The corner head is warm (RoI proposal, trimming by random.sample and the gather all see detector boxes)."""
    import gc
    import json
    import os
    B = 32
    model = zoo.denet34(B, "skip", 512, class_num=80, seed=1)
    missing = audit.decisions_cover(model)
    assert not missing, "passes without a committed decision (would be measured on the first step): %s" % (missing[:4],)
    assert ops.POLICY is None and ops.AUTOTUNE and not ops.MEASURE
    with audit.KernelAudit(model) as ka:
        _denet34_skip_steps_vs_oracle("warm", B, 512, 1, model=model)
    gc.collect()
    fused = lambda g, T: _map(g) in (64, 32)
    seen = assert_kernels(ka.table, B, expect_w4f=fused, expect_w4g=lambda g, T: True)
    assert seen["wino4f"] == 20 and seen["wino4g"] == 25 and seen["wino2f"] == 6 and seen["stem"] == 1, seen
    # the 64-channel stage at this geometry: forward pass and data gradient of all six layers on the tile-parallel fused F(4x4)
    # kernel (algorithm 44 of the committed file; DENET_WINO4T=0 would put the fused F(2x2) kernels back)
    assert seen["wino4t"] == (12 if ops.WINO4T == 3 else seen["wino4t"]), seen
    for r in ka.table:      # 32-tile blocks everywhere: two 4-wave workgroups per CU where that fills the chip (the 64x64 maps, and the
        # data gradient of up1, whose 512 output channels give 512 workgroups), one 8-wave workgroup else
        if _is_3x3s1(r["geometry"]) and _chan(r["geometry"])[0] >= 128 and _map(r["geometry"]) in (64, 32):
            shape = "wino4f_kernel_32x2<" if _map(r["geometry"]) == 64 else "wino4f_kernel_32"
            assert all(k.startswith(shape) for k in r["fwd"] + r["bwd"] if k.startswith("wino4f")), r
    worst = sorted(ELEMENTWISE.items(), key=lambda kv: -kv[1][1])[:8]
    rep = {"test": "test_denet34_skip_512_timed_batch_vs_oracle", "batch": B,
           "elementwise_p9999_and_maxnorm_worst": [(k, float("%.3e" % v[1]), float("%.3e" % v[0])) for k, v in worst],
           "kernels": ka.summary()}
    print("B=32 oracle parity, element-wise p99.99 / max-norm, worst:", rep["elementwise_p9999_and_maxnorm_worst"])
    out = os.environ.get("PARITY_REPORT_PATH")
    if out:
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)


def test_denet34_edge_case_ground_truth_vs_oracle(hip):
    """ragged ground truth through the whole step: an image without objects, a crowded image (39 boxes, more than any
    MSCOCO-like batch of the synthetic generator), a sliver box, boxes partly / completely off screen and an exact
    duplicate - corner targets (denet_corner.py:81-123), RoI editing + GT injection (denet_sparse.py:184-201),
    detection targets (denet_detect.py:147-235) and both costs, op by op against the oracle"""
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
    rng = np.random.RandomState(9)
    dconv = model.layers[40].layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, _ = zoo.synthetic_batch(B, IMG, seed=4)
    crowd, cls = [], []
    for k in range(34):
        cx, cy, w, h = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.02, 0.5), rng.uniform(0.02, 0.5)
        crowd.append((float(max(cx - w / 2, 0)), float(max(cy - h / 2, 0)), float(min(cx + w / 2, 1)), float(min(cy + h / 2, 1))))
        cls.append(int(rng.randint(0, 80)))
    # (zero-area boxes are not part of the contract: the reference's IoU is 0/0 = NaN for them and its cost turns NaN,
    # which train_epoch treats as fatal, model_cnn.py:462; the loader never emits them, image_loader.py:128)
    crowd += [(0.3, 0.3, 0.30001, 0.6),                             # a sliver, narrower than one feature cell
              (-0.2, 0.1, 0.25, 0.4), (0.8, 0.7, 1.3, 1.2),         # partly off screen
              (1.1, 1.1, 1.4, 1.5),                                 # completely off screen
              crowd[0]]                                             # exact duplicate (other class)
    cls += [3, 5, 6, 7, (cls[0] + 1) % 80]
    metas = [{"bbox": [], "class": []}, {"bbox": crowd, "class": cls}]
    om_free = OM.OracleModel(model.export_json(), B)
    om = OM.OracleModel(model.export_json(), B)
    model.build_train_func("nesterov")
    lr, mu, decay = 0.05, 0.9, 1e-4
    for it in range(2):
        random.seed(300 + it)
        cost, costs = model.train_step(x, metas, 0, it, lr, [mu], decay)
        assert np.isfinite(cost)
        dns, cl = model.layers[31], model.layers[30]
        roi_lists = dns.sample_bbox_list
        ref_lists, _ = reference_edit_of_the_products_proposal(dns, cl, metas, 300 + it)
        assert ref_lists == roi_lists, "RoI lists differ from the reference editing of the same proposal"
        assert [r for r in roi_lists[1][-len(crowd):]] == [(1.0, b) for b in crowd[::-1]]     # GT injection, reversed
        if it == 0:
            random.seed(300 + it)
            fcost, fcosts = om_free.forward_costs(x, metas, sample_override=roi_lists)      # forward quantities only are compared
            assert abs(cost - fcost) <= 1e-3 * abs(fcost), (cost, fcost)
            for c, oc in zip(costs, fcosts):
                assert abs(c - oc) <= 1e-3 * max(abs(oc), 1e-6), (costs, fcosts)
        ocost, _ = _forced_step_check(model, om, x, metas, it, lr, mu, decay, "nesterov", roi_lists)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


def test_denet34_odd_geometry_vs_oracle(hip):
    """batch 3 at 160x160: feature maps of 40 / 20 / 10 / 5 cells - the 5x5 and 10x10 maps are not multiples of the
    Winograd tile (direct kernels there), M is not a multiple of the GEMM tile anywhere; op-by-op against the oracle"""
    B, IMG = 3, 160
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
    rng = np.random.RandomState(5)
    dconv = model.layers[40].layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=6)
    om = OM.OracleModel(model.export_json(), B)
    model.build_train_func("nesterov")
    for it in range(2):
        random.seed(40 + it)
        cost, _ = model.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
        dns, cl = model.layers[31], model.layers[30]
        roi_lists = dns.sample_bbox_list
        lists = OM.oracle_build_samples(cl.corner_pr.cpu().numpy(), dns.corner_threshold, dns.sample_num, 1024, 0)
        random.seed(40 + it)
        ref_lists = OL.edit_samples(lists, metas, dns.sample_count, dns.random_sample, dns.sample_gt)
        assert [[p for p, _ in l] for l in ref_lists] == [[p for p, _ in l] for l in roi_lists]
        ocost, _ = _forced_step_check(model, om, x, metas, it, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


def test_cifar3_train_step_vs_oracle(hip):
    """BASELINE config 1 (README.md:52 three-layer CNN): unfused BN / A / P / P.A / R path"""
    B = 8
    model = zoo.cifar3(B, 10, seed=3)
    rng = np.random.RandomState(1)
    x = rng.uniform(0, 1, (B, 3, 32, 32)).astype(np.float32)
    metas = [{"image_class": int(rng.randint(0, 10)), "bbox": [], "class": []} for _ in range(B)]
    rconv = model.layers[-2]
    rconv.omega.set_value(rng.normal(0, 0.05, rconv.omega.value.shape))
    om = OM.OracleModel(model.export_json(), B)
    om_free = OM.OracleModel(model.export_json(), B)
    model.build_train_func("sgd")
    for it in range(2):
        cost, costs = model.train_step(x, metas, 0, it, 0.1, [0.9], 1e-4)
        if it == 0:
            fcost, _ = om_free.train_step(x, metas, it, 0.1, 0.9, 1e-4, "sgd")
            assert abs(cost - fcost) <= 1e-3 * abs(fcost), (cost, fcost)
            for i, a in _product_acts(model).items():
                rel_close(a, om_free.acts[i], 1e-3, "activation L%d" % i)
        ocost, _ = _forced_step_check(model, om, x, metas, it, 0.1, 0.9, 1e-4, "sgd", None)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)
    # inference: BN test mode (double eps) + softmax probabilities
    p = model.predict_output_step(x)
    om.forward(x, None, train=False)
    logits = om.out.v.reshape(B, 10).astype(np.float64)
    ref = np.exp(OL.log_softmax(logits, axis=1))
    rel_close(p, ref, 1e-3, "predict")


def test_full_size_properties(hip):
    """BASELINE config 3 at full size (B=32, 512x512): properties that do not need the slow CPU oracle"""
    B = 32
    x, metas = zoo.synthetic_batch(B, 512, seed=1)
    xd = torch.from_numpy(x).cuda()
    results = []
    ops.FINAL_COUNT[:] = [0, 0]
    for run in range(2):
        model = zoo.denet34(B, "skip", 512, seed=1)
        _warm_corner_head(model, 7.5, 0.3)
        model.build_train_func("nesterov")
        random.seed(1)
        c0 = model.train_step(xd, metas, 0, 0, 0.1, [0.9], 1e-4)
        c1 = model.train_step(xd, metas, 0, 1, 0.1, [0.9], 1e-4)
        results.append((c0, c1, model.P.clone()))
        assert np.isfinite(c0[0]) and np.isfinite(c1[0])
    # determinism: no atomics on floating point anywhere in the step
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert torch.equal(results[0][2], results[1][2])
    # the OPTION of finishing the batch-norm reductions inside the producing launches (ops.BnFinal: last-workgroup tickets,
    # write-through rows; off by default, measured slower) against the separate final launches at the full size: bit-identical
    # parameters after two steps - a stale partial row would show as a bit
    assert ops.FINAL_COUNT == [0, 0], ops.FINAL_COUNT
    saved_fold = ops.set_final_fold(3)
    try:
        m2 = zoo.denet34(B, "skip", 512, seed=1)
        _warm_corner_head(m2, 7.5, 0.3)
        m2.build_train_func("nesterov")
        random.seed(1)
        d0 = m2.train_step(xd, metas, 0, 0, 0.1, [0.9], 1e-4)
        d1 = m2.train_step(xd, metas, 0, 1, 0.1, [0.9], 1e-4)
    finally:
        ops.set_final_fold(saved_fold)
    assert ops.FINAL_COUNT[0] >= 30 and ops.FINAL_COUNT[1] >= 30, ops.FINAL_COUNT
    assert d0 == results[0][0] and d1 == results[0][1]
    assert torch.equal(m2.P, results[0][2]) and torch.equal(m2.S, model.S) and torch.equal(m2.M, model.M)
    del m2
    # RoI proposal: sortedness + idempotence at full size, against the oracle on the same map
    cl, dns = model.layers[30], model.layers[31]
    pr = cl.corner_pr
    b1 = ops.build_samples(pr, 0.01, 576, 1024, 0)
    b2 = ops.build_samples(pr, 0.01, 576, 1024, 0)
    assert all(torch.equal(a, b) for a, b in zip(b1, b2))
    cnt = b1[2].cpu().numpy()
    absd = b1[1].cpu().numpy()
    assert cnt.sum() > 0
    for b in range(B):
        assert np.all(np.diff(absd[b, :cnt[b]]) >= 0)
    check_samples(pr.cpu().numpy(), 0.01, 24, 1024, 0)
    # gather checksum: every output row is a copy of fmap rows at the recorded taps
    fmap, coff, F = cl.sample_map()
    out = dns.output.data.view(B * 576, -1)
    taps = dns._taps.long()
    rows = torch.arange(B * 576, device="cuda") // 576
    for t in (0, 24, 48):
        src = fmap.view(B, -1, fmap.shape[-1])[rows, taps[:, t], coff:coff + F]
        assert torch.equal(out[:, t * F:(t + 1) * F], src)
    assert float(out[:, 49 * F + 2:].abs().max()) == 0.0


def test_denet101_wide_full_size_properties(hip):
    """BASELINE config 5 at full size (DeNet-101 wide, 512x512, B = 16, 2304 RoIs per image, `DND.JB`: joint fitness + bounded-IoU
    loss; papers/dss/denet101.sh:13-19): two runs of two training steps are finite and bit-identical (no floating-point atomics
    anywhere on this path either), the RoI proposal on the 128x128 corner map - 2304 of up to 2 x 1024^2 candidates through the
    two-level final sort - is sorted, idempotent and equal to the oracle's on the same map, the gather is a copy of feature rows
    at the recorded taps. The per-layer numerics at these shapes: tests/test_conv_fullsize_gpu.py (d101_*)."""
    B = 16
    x, metas = zoo.synthetic_batch(B, 512, seed=1)
    xd = torch.from_numpy(x).cuda()
    desc = zoo.DENET101_WIDE_DESC.replace("DND[0.5,1,1]", "DND.JB[0.5,1,1]")
    results = []
    for run in range(2):
        model = zoo.denet101(B, "wide", 512, 80, seed=1, head_desc=desc)
        _warm_corner_head(model, 7.5, 0.3)
        model.build_train_func("nesterov")
        random.seed(1)
        c0 = model.train_step(xd, metas, 0, 0, 0.1, [0.9], 1e-4)
        c1 = model.train_step(xd, metas, 0, 1, 0.1, [0.9], 1e-4)
        results.append((c0, c1, model.P.clone()))
        assert np.isfinite(c0[0]) and np.isfinite(c1[0])
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert torch.equal(results[0][2], results[1][2])
    # the proposal / gather properties on the map of a FIRST step (two steps at lr 0.1 train this corner head silent again)
    del model
    model = zoo.denet101(B, "wide", 512, 80, seed=1, head_desc=desc)
    _warm_corner_head(model, 4.0, 0.3)
    model.build_train_func("nesterov")
    random.seed(1)
    model.train_step(xd, metas, 0, 0, 0.1, [0.9], 1e-4)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    cl, dns = by_type("denet-corner"), by_type("denet-sparse")
    assert dns.sample_count == 2304 and cl.corner_pr.shape[-1] == 128
    pr = cl.corner_pr
    b1 = ops.build_samples(pr, 0.01, 2304, 1024, 0)
    b2 = ops.build_samples(pr, 0.01, 2304, 1024, 0)
    assert all(torch.equal(a, b) for a, b in zip(b1, b2))
    cnt, absd = b1[2].cpu().numpy(), b1[1].cpu().numpy()
    assert cnt.sum() > 0
    for b in range(B):
        assert np.all(np.diff(absd[b, :cnt[b]]) >= 0)
    check_samples(pr.cpu().numpy(), 0.01, 48, 1024, 0)
    fmap, coff, F = cl.sample_map()
    out = dns.output.data.view(B * 2304, -1)
    taps = dns._taps.long()
    rows = torch.arange(B * 2304, device="cuda") // 2304
    for t in (0, 24, 48):
        src = fmap.view(B, -1, fmap.shape[-1])[rows, taps[:, t], coff:coff + F]
        assert torch.equal(out[:, t * F:(t + 1) * F], src)
    assert float(out[:, 49 * F + 2:].abs().max()) == 0.0


def _generic_step_check(desc, data_shape, B, solver="nesterov", steps=2, convert=False, class_num=10, seed=11):
    from denet_amd.model import model_cnn, modify
    np.random.seed(seed)
    model = model_cnn.ModelCNN()
    model.batch_size = B
    model.class_num = class_num
    model.build(desc, data_shape, "relu", "half", ["he-backward"])
    if convert:
        model = modify.convert_bn_relu(model)
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, (B,) + tuple(data_shape)).astype(np.float32)
    metas = [{"image_class": int(rng.randint(0, class_num)), "bbox": [], "class": []} for _ in range(B)]
    # non-trivial BN parameters and a non-zero classifier so that every gradient path carries signal
    for l in model.layers[1:]:
        for p in l.biases():
            p.set_value(p.value + rng.normal(0, 0.1, p.value.shape).astype(np.float32))
    rconv = model.layers[-2]
    rconv.omega.set_value(rng.normal(0, 0.05, rconv.omega.value.shape))
    om = OM.OracleModel(model.export_json(), B, rng_seed=model.rng_seed)
    om_free = OM.OracleModel(model.export_json(), B, rng_seed=model.rng_seed)
    model.build_train_func(solver)
    mom = [0.9, 0.999] if solver == "adam" else [0.9]
    omom = mom if solver == "adam" else mom[0]
    lr = 0.002 if solver == "adam" else 0.05
    for it in range(steps):
        cost, _ = model.train_step(x, metas, 0, it, lr, mom, 1e-4)
        if it == 0:
            fcost, _ = om_free.train_step(x, metas, it, lr, omom, 1e-4, solver)
            assert abs(cost - fcost) <= 1e-3 * abs(fcost), (cost, fcost)
            for i, a in _product_acts(model).items():
                rel_close(a, om_free.acts[i], 1e-3, "activation L%d %s" % (i, model.layers[i].type_name))
        ocost, _ = _forced_step_check(model, om, x, metas, it, lr, omom, 1e-4, solver, None)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)
    return model


@pytest.mark.parametrize("convert", [False, True])
def test_resnet_variants_vs_oracle(hip, convert):
    """pre-activation and original residual blocks, basic and bottleneck bodies, projection shortcuts with and
    without BN (denet/layer/resnet.py:52-113), unfused BN + A and the --convert-bn-relu fused form"""
    desc = "C.B[32,3] BN A nRSN[2,64,3,2,32] nRSN.O[2,64,3,1,32] nRSN[1,96,3,2] RSN.O[96,3] P.A[4] R"
    model = _generic_step_check(desc, (3, 16, 16), 4, convert=convert)
    versions = [l.version for l in model.layers if l.type_name == "resnet"]
    assert any("pre-activation" in v for v in versions) and any("original" in v for v in versions)
    assert all(("bnrelu" in v) == (convert and "original" in v) or "pre-activation" in v for v in versions)


def test_resnet34_224_config2_vs_oracle(hip):
    """BASELINE config 2 (ResNet-34 backbone, 224x224, examples/resnet34-imagenet.sh:7) at B=2 against the numpy oracle:
    free-running activations and cost, then the op-by-op teacher-forced step (gradients, running statistics, update)"""
    _generic_step_check(zoo.RESNET34_DESC, (3, 224, 224), 2, steps=1, class_num=1000, seed=5)


def test_resnet34_224_config2_full_size_properties(hip):
    """config 2 at its workload (B=64, 224x224, 1000 classes): two training steps are finite, bit-reproducible run to run
    (same measured launch configurations inside one process), the cost moves; the per-layer numerics at these shapes are covered by tests/test_conv_fullsize_gpu.py (r34_*)"""
    B = 64
    rng = np.random.RandomState(3)
    x = torch.from_numpy(rng.uniform(0, 1, (B, 3, 224, 224)).astype(np.float32)).cuda()
    metas = [{"image_class": int(rng.randint(0, 1000)), "bbox": [], "class": []} for _ in range(B)]
    results = []
    for run in range(2):
        model = zoo.resnet34(B, 224, seed=1)
        model.build_train_func("nesterov")
        c0 = model.train_step(x, metas, 0, 0, 0.1, [0.9], 1e-4)
        c1 = model.train_step(x, metas, 0, 1, 0.1, [0.9], 1e-4)
        results.append((c0, c1, model.P.clone()))
        assert np.isfinite(c0[0]) and np.isfinite(c1[0])
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert torch.equal(results[0][2], results[1][2])
    assert results[0][0][0] != results[0][1][0] and results[0][0][0] > 0


def test_direct_and_measured_paths_agree(hip):
    """the same training step with the heuristic direct kernels (DENET_AUTOTUNE=0 behaviour) and with the measured
    configurations / Winograd passes: the costs agree to rounding, and - layer by layer, on the tensors of the real step -
    every convolution pass of the measured implementation agrees with the direct kernel within the per-layer bound that
    tests/test_conv_fullsize_gpu.py establishes against fp64 at the benchmark geometries (direct 4e-6, F(4x4) 2.5e-5
    measured; 1e-4 asserted). The whole-network parameter update is NOT compared element-wise: it is a discontinuous
    function of 1e-6-level forward differences (ReLU mask flips move a BN beta gradient by 0.5 % at M = 1152, see
    _forced_step_check), which says nothing about a kernel."""
    from denet_amd import ops
    from denet_amd.model import model_cnn
    B, IMG = 2, 128
    x, metas = zoo.synthetic_batch(B, IMG, seed=2)
    res = []
    with ops.algorithms() as wino:
        for tuned in (False, True):
            # MEASURE: the explicit measuring mode (DENET_TUNE=1, what tools/tune.py runs): this test exercises the tuner
            with ops.switches(AUTOTUNE=tuned, MEASURE=tuned):
                wino.clear()
                model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
                _warm_corner_head(model, 4.0, 0.3)
                model.build_train_func("nesterov")
                random.seed(3)
                c0, _ = model.train_step(x, metas, 0, 0, 0.002, [0.9], 1e-4)
                torch.cuda.synchronize()
                res.append((c0, dict(ops._WINO)))
        assert not any(res[0][1].values()), "the heuristic run must not use Winograd passes"
        if ops.WINOGRAD:           # DENET_WINOGRAD=0 leaves only the measured direct configurations to compare
            assert any(res[1][1].values()), "the measured run chose no Winograd pass at all: the test compares nothing"
        assert abs(res[0][0] - res[1][0]) <= 1e-4 * abs(res[0][0])
        # per layer, on the step's own tensors (the model of the measured run is still alive): x, dy, w of every convolution
        convs = [l for l in model_cnn.walk_layers(model.layers) if l.type_name == "conv" and l.output.grad is not None]
        assert len(convs) >= 40
        worst = {}
        for l in convs:
            xin, dy, w = l.input.data, l.output.grad, l._w()
            st, pad, sr = l.stride[0], l.pad, l.filter_shape[3]
            out = {}
            for tuned in (True, False):         # (the measuring mode stays on, as it was left by the measured step above)
                with ops.switches(AUTOTUNE=tuned, MEASURE=True):
                    if not tuned:
                        wino.clear()
                    y = ops.conv_fwd(xin, w, stride=st, pad=pad, s_real=sr)
                    dw = ops.conv_wgrad(xin, dy, tuple(w.shape), stride=st, pad=pad, s_real=sr)
                    dx = ops.conv_dgrad(dy, w, tuple(xin.shape), stride=st, pad=pad, s_real=sr) if xin.shape[-1] >= 32 else None
                    out[tuned] = (y, dw, dx)
            wino.clear()
            wino.update(res[1][1])
            for name, a, d in zip(("fwd", "wgrad", "dgrad"), out[True], out[False]):
                if a is None:
                    continue
                err = float((a - d).abs().max()) / (float(d.abs().max()) + 1e-30)
                worst[name] = max(worst.get(name, 0.0), err)
                assert err <= 1e-4, "layer %d %s: measured vs direct implementation differ by %.2e (max-norm)" % (
                    l.layer_index, name, err)
        print("worst per-layer measured-vs-direct difference:", worst)


@pytest.mark.parametrize("mode", [33, 64])
def test_bn_reductions_finished_in_the_producing_launch_are_bit_identical(hip, mode):
    """ops.BnFinal / csrc/bn_final.h (an OPTION, off by default: measured slower than the launches it replaces): the second stage of a batch norm's reductions (forward statistics: batch_norm.py:50-53, 75-76;
    backward sums of tensor.grad, model_cnn.py:318) runs in the LAST workgroup of the convolution pass that writes the partial rows
    (write-through rows, an agent-scope ticket per column group, reads past the caches) instead of a launch of its own. By
    construction the arithmetic is the separate kernels': six training steps of DeNet-34 skip (B = 4, 256x256; the fused F(4x4)
    kernel forced on so that every producer takes part: fused F(4x4) forward / data gradient, fused F(2x2), implicit-GEMM
    epilogues of the head and the 1x1 layers) with the fold on and off give bit-identical parameters, momentum and running
    statistics - under uneven load (a second stream hammers the memory system with copies of changing size), several times over.
    A stale row, a lost ticket or a counter that is not at rest would show as a different bit (or a hang: the suite's timeout)."""
    L = lib.load()
    B, IMG = 4, 256
    x, metas = zoo.synthetic_batch(B, IMG, seed=2)
    xd = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    a, b = torch.empty(1 << 26, device="cuda"), torch.empty(1 << 26, device="cuda")
    old = (L.denet_conv_wino4f_mode(mode), ops.set_final_fold(0))

    def run(fold, pressure):
        ops.set_final_fold(3 if fold else 0)
        ops.FINAL_COUNT[:] = [0, 0]
        model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
        _warm_corner_head(model, 4.0, 0.3)
        model.build_train_func("nesterov")
        random.seed(5)
        costs = []
        for it in range(6):
            if pressure:
                with torch.cuda.stream(side):
                    for k in range(40):
                        n = 1 << (18 + (k * 7 + it) % 9)
                        b[:n].copy_(a[:n], non_blocking=True)
            costs.append(model.train_step(xd, metas, 0, it, 0.05, [0.9], 1e-4)[0])
        torch.cuda.synchronize()
        return costs, model.P.clone(), model.M.clone(), model.S.clone(), list(ops.FINAL_COUNT)

    try:
        ref = run(False, False)
        assert ref[4] == [0, 0]
        for rep in range(3):
            got = run(True, True)
            assert got[4][0] >= 6 * 25 and got[4][1] >= 6 * 25, "too few reductions were finished in their producers: %s" % (got[4],)
            assert got[0] == ref[0], (rep, got[0], ref[0])
            for k in (1, 2, 3):
                assert torch.equal(got[k], ref[k]), "run %d: %s differs" % (rep, "PMS"[k - 1])
    finally:
        L.denet_conv_wino4f_mode(old[0])
        ops.set_final_fold(old[1])


def test_bn_final_fold_in_front_of_a_pool_fused_batch_norm(hip):
    """with the fold on, a generic convolution (not the stem kernels) in front of a batch norm whose BN + ReLU +
    max pool run as ONE pass must not finish the statistics itself - the fused pass reduces the rows and updates the running
    statistics, a second update would advance run_mean / run_stdinv twice per step. The three-layer CIFAR network (C BN A P x 3:
    layers 2 and 3 are generic convolutions feeding pool-fused batch norms): parameters, momentum and RUNNING STATISTICS after
    four steps are bit-identical with the fold on and off."""
    B = 32
    x, metas = zoo.synthetic_batch(B, 32, class_num=10, image_class=True, seed=4)
    xd = torch.from_numpy(x).cuda()
    old = ops.set_final_fold(0)

    def run(fold):
        ops.set_final_fold(3 if fold else 0)
        model = zoo.cifar3(B, class_num=10, seed=2)
        model.build_train_func("nesterov")
        fused = [l for l in model_cnn_walk(model.layers) if getattr(l, "pool_behind", None) is not None]
        costs = [model.train_step(xd, metas, 0, it, 0.05, [0.9], 1e-4)[0] for it in range(4)]
        torch.cuda.synchronize()
        return costs, model.P.clone(), model.M.clone(), model.S.clone(), len(fused)

    try:
        with ops.switches(BN_POOL_FUSE=True):      # (the file's autouse fixture switches the pooled pass off for the teacher-forced tests)
            ref, got = run(False), run(True)
            assert ref[4] >= 2 and ops.BN_POOL_FUSE, "no pool-fused batch norm in the network: the test exercises nothing"
            assert got[0] == ref[0]
            for k in (1, 2, 3):
                assert torch.equal(got[k], ref[k]), "%s differs with the fold on" % "PMS"[k - 1]
    finally:
        ops.set_final_fold(old)


def test_bn_pool_fusion_leaves_training_unchanged(hip):
    """a training step of DeNet-34 skip with the stem's BN + ReLU + max pool as one pass and as three. The pooled form takes the
    layer's two backward reductions over the pooled tensors (ops.bn_relu_pool_bwd_pooled: the same sums in another order of a
    double-precision summation; the element values - output, argmax, statistics, dx given the sums - are bit-identical,
    test_bn_relu_pool_fused_equals_separate_passes), so the states agree numerically: 1e-5 max-norm relative per buffer. ONE
    step: the forward passes are bit-identical (same RoIs), the difference is in the stem's gradients only; a second step would
    feed it through the discrete RoI selection"""
    res = []
    for fuse in (True, False):
        with ops.switches(BN_POOL_FUSE=fuse):
            random.seed(7)
            model = zoo.warm_corner_head(zoo.denet34(2, "skip", 128, class_num=80, seed=1), 4.0, 0.3)
            model.build_train_func("nesterov")
            stem_bn = [l for l in model.layers if getattr(l, "pool_behind", None) is not None]
            assert len(stem_bn) == 1
            x, metas = zoo.synthetic_batch(2, 128, seed=11)
            costs = [model.train_step(x, metas, 0, it, 0.02, [0.9], 1e-4)[0] for it in range(1)]
            torch.cuda.synchronize()
            assert (stem_bn[0].output.data is None) == fuse
            res.append((model.P.clone(), model.M.clone(), model.S.clone(), costs))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    for ca, cb in zip(res[0][3], res[1][3]):
        assert abs(ca - cb) <= 1e-5 * abs(cb)


def test_bn_followed_by_activation_runs_fused_and_trains_the_same(hip, monkeypatch):
    """`BN A` as two layers (un-converted ResNet-34, examples/resnet34-imagenet.sh:7): the batch norm runs the fused BN + ReLU
    passes into the activation's output where that activation is its only reader (ActivationLayer.fused_into; the stem's
    `BN A P` becomes the one-pass BN + ReLU + max pool). Against DENET_BN_ACT_FUSE=0 (three layers, three passes): same costs
    and state after two steps to rounding (the fused backward takes its reductions from other kernels), same class
    probabilities in test mode"""
    res = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("DENET_BN_ACT_FUSE", fuse)
        model = zoo.resnet34(2, 224, 10, seed=1)
        model.build_train_func("nesterov")
        pairs = [l for l in model_cnn_walk(model.layers) if l.type_name == "batchnorm" and getattr(l, "act_behind", None) is not None]
        assert len(pairs) == 17 and all(l.act_fused == (fuse == "1") for l in pairs)
        x, metas = zoo.synthetic_batch(2, 224, 10, seed=3, image_class=True)
        costs = [model.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)[0] for it in range(2)]
        torch.cuda.synchronize()
        assert (pairs[1].output.data is None) == (fuse == "1")
        res.append((model.P.clone(), model.M.clone(), model.S.clone(), costs, model.predict_output_step(x)))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())
    for ca, cb in zip(res[0][3], res[1][3]):
        assert abs(ca - cb) <= 1e-5 * abs(cb)
    np.testing.assert_allclose(res[0][4], res[1][4], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("img,tile", [(128, 4), (256, 4), (128, 2)])
def test_batch_norm_linked_into_winograd_transforms_is_bit_identical(hip, img, tile):
    """ops.LINK_BN: the pointwise pass of a batch norm evaluated inside the input transform of the Winograd convolution next to
    it (forward: denet_conv_wino_fwd_fold; backward: denet_conv_wino_dgrad_fold + denet_conv_wino_wgrad_dm, the gradient tensor
    between batch norm and convolution is never written) against the separate kernels: training steps of DeNet-34 skip,
    parameters / momentum / running statistics bit for bit. Reference chain: conv -> BN(+ReLU) -> conv of the residual blocks
    (denet/layer/resnet.py:60-90, batch_norm_relu.py:34-54). Every 3x3 stride-1 layer is put on the un-fused Winograd passes of
    one tile size (all three passes), so that the linked forms run for whole blocks; 128: maps of 4x4 ... 16x16 cells (partial
    tile blocks of the LDS-staged transform), 256: full blocks"""
    res = []

    def build():
        model = zoo.warm_corner_head(zoo.denet34(2, "skip", img, class_num=80, seed=1), 4.0, 0.3)
        model.build_train_func("nesterov")
        return model
    with ops.algorithms() as wino:
        # every launch configuration is decided once, on a throwaway model (the measurement of a first step may pick different
        # implementations from run to run at these sizes); then all eligible layers are put on one Winograd tile
        x, metas = zoo.synthetic_batch(2, img, seed=11)
        with ops.switches(LINK_BN=False):
            build().train_step(x, metas, 0, 0, 0.02, [0.9], 1e-4)
        for (mode, g) in list(wino):
            if ops.conv_wino_ok(g, tile):
                wino[(mode, g)] = tile
        for link in (True, False):
            with ops.switches(LINK_BN=link):
                ops.LINK_COUNT[:] = [0, 0]
                random.seed(7)
                model = build()
                costs = [model.train_step(x, metas, 0, it, 0.02, [0.9], 1e-4)[0] for it in range(3)]
                torch.cuda.synchronize()
                if link:
                    assert ops.LINK_COUNT[0] >= 16 and ops.LINK_COUNT[1] >= 16, ops.LINK_COUNT
                else:
                    assert ops.LINK_COUNT == [0, 0]
                res.append((model.P.clone(), model.M.clone(), model.S.clone(), costs))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(a, b)
    assert res[0][3] == res[1][3]


@pytest.mark.parametrize("img,tile", [(128, 4), (256, 22), (128, 2)])
def test_batch_norm_backward_sums_from_the_data_gradient_pass(hip, img, tile):
    """ops.BWD_SUMS: the output transform of a Winograd data-gradient pass (un-fused F(2x2) / F(4x4): wino_output_kernel; the fused
    64-channel kernel: wino2f_ws_kernel; the 1x1 layers of the RoI head: the implicit-GEMM epilogue) also writes the two backward reductions sum(g), sum(g * xhat) of the batch norm whose
    output gradient it produces, and that layer's backward skips its own reduction pass (bn_bwd_partial_kernel). Reference:
    the gradient of batch_norm.py:50-53 / batch_norm_relu.py:50-54 through model_cnn.py:318. The sums are accumulated per block
    in fp32 before they are widened, so the comparison is numeric: all gradients of one step from identical parameters within
    3e-5 max-norm relative, per parameter range (measured 1.5e-5 ... 2.1e-5 depending on the kernels of the first layer)"""
    res = []

    def build():
        model = zoo.warm_corner_head(zoo.denet34(2, "skip", img, class_num=80, seed=1), 4.0, 0.3)
        model.build_train_func("nesterov")
        return model
    with ops.algorithms() as wino:
        x, metas = zoo.synthetic_batch(2, img, seed=11)
        with ops.switches(BWD_SUMS=0):
            build().train_step(x, metas, 0, 0, 0.02, [0.9], 1e-4)              # decides the launch configurations once
        for (mode, g) in list(wino):
            t = tile if tile != ops.FUSED2 else (ops.FUSED2 if ops.conv_wino2f_ok(mode, g) else 4)
            if (t == ops.FUSED2) or ops.conv_wino_ok(g, t):
                wino[(mode, g)] = t
        for on in (True, False):
            with ops.switches(BWD_SUMS=3 if on else 0):     # Winograd passes and the stride-1 implicit-GEMM passes (1x1 head)
                ops.SUMS_COUNT[0] = 0
                random.seed(7)
                model = build()
                model.train_step(x, metas, 0, 0, 0.0, [0.9], 0.0)              # learning rate 0: the gradients are what is compared
                torch.cuda.synchronize()
                assert (ops.SUMS_COUNT[0] >= 12) if on else (ops.SUMS_COUNT[0] == 0), ops.SUMS_COUNT
                res.append((model, model.G.clone()))
    (m, ga), (_, gb) = res
    worst = 0.0
    for layer, lo, hi in m.layer_weight_range:
        ref = float(gb[lo:hi].abs().max())
        if ref > 0:
            worst = max(worst, float((ga[lo:hi] - gb[lo:hi]).abs().max()) / ref)
    nb = m.n_trainable
    bias_ref = float(gb[m.n_weights:nb].abs().max())
    worst_b = float((ga[m.n_weights:nb] - gb[m.n_weights:nb]).abs().max()) / bias_ref
    assert worst < 3e-5 and worst_b < 3e-5, (worst, worst_b)


def test_cold_detector_hand_off_equals_the_host_path(hip, monkeypatch):
    """With a cold corner detector (no proposals: weights as initialised, the regime of the first training steps)
    the edited RoI list is all random boxes + ground truth. The device-side editing takes such a batch too (no image proposes
    more than the list keeps); a warm detector that proposes more than that takes the fast host hand-off. Three steps with the
    short forms on and off: the same RoI lists (reference loop: denet/layer/denet_sparse.py:184-201), the same parameters bit
    for bit, the generator at the same position afterwards"""
    from denet_amd.layer import roi_handoff as RH
    res = {}
    for warm in (False, True):
        for short in (True, False):
            monkeypatch.setattr(RH, "DEVICE_EDIT", short)
            monkeypatch.setattr(RH, "FAST_HANDOFF", short)
            random.seed(21)
            model = zoo.denet34(2, "skip", 128, class_num=80, seed=1)
            if warm:
                zoo.warm_corner_head(model, 4.0, 0.3)
            model.build_train_func("nesterov")
            dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
            x, metas = zoo.synthetic_batch(2, 128, seed=11)
            lists = []
            for it in range(3):
                model.train_step(x, metas, 0, it, 0.0 if warm else 0.02, [0.9], 1e-4)      # lr 0: the warm head stays warm
                lists.append(dns.sample_bbox_list)
            torch.cuda.synchronize()
            modes = dict(dns.handoff_modes)
            assert sum(modes.values()) == 3, modes
            # (the first step may draw from the generator between the preparation and the hand-off - a layer seed - and
            # then takes the ordinary path, which is the point of the freshness check)
            if not short:
                assert modes == {"device_edit": 0, "fast": 0, "host": 3}, modes
            elif not warm:
                assert modes["device_edit"] >= 1 and modes["host"] <= 1, modes      # (the corner cost warms the head within the three steps)
            res[(warm, short)] = (model.P.clone(), lists, random.random())
    for warm in (False, True):
        a, b = res[(warm, True)], res[(warm, False)]
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], warm




def test_device_side_editing_equals_the_host_list(hip, monkeypatch):
    """The two short forms of the RoI hand-off against the ordinary one. RoiHandoff._device_edit: when no image proposes
    more RoIs than the list keeps (no random.sample), the bbox array is written on the device (denet_edit_samples_device:
    proposals, random boxes from generator outputs drawn ahead, ground truth) and the host's editing runs later for the
    Python-side list. _fast_handoff: every other batch - one native call (sample tuples + editing on the prefetched outputs) and
    the upload, the bookkeeping later. Reference loop: denet/layer/denet_sparse.py:184-201. The device array equals the host's
    float32 array bit for bit; lists, parameters after three steps and the generator's position are identical in all three
    modes; a detector that proposes more than the list keeps does not take the device path; `handoff_modes` says which form
    every step took."""
    from denet_amd.layer import roi_handoff as RH
    res, took = {}, {}
    biases, modes = (5.6, 5.0, 4.0), ((True, True), (False, True), (False, False))
    for bias in biases:          # a few dozen ... more than 519 proposals per image
        for mode in modes:
            monkeypatch.setattr(RH, "DEVICE_EDIT", mode[0])
            monkeypatch.setattr(RH, "FAST_HANDOFF", mode[1])
            random.seed(21)
            model = zoo.warm_corner_head(zoo.denet34(2, "skip", 128, class_num=80, seed=1), bias, 0.3)
            model.build_train_func("nesterov")
            dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
            x, metas = zoo.synthetic_batch(2, 128, seed=11)
            lists, arrays = [], []
            for it in range(3):
                model.train_step(x, metas, 0, it, 0.0, [0.9], 1e-4)      # lr 0: the detector stays as warm as it is
                dev_bbox = dns.sample_bbox.clone()
                lists.append(dns.sample_bbox_list)
                torch.cuda.synchronize()
                assert torch.equal(dev_bbox.cpu().view(-1), torch.from_numpy(dns.sample_bbox_f32.reshape(-1).copy()))
                arrays.append(dev_bbox.cpu())
            assert sum(dns.handoff_modes.values()) == 3, dns.handoff_modes
            took[(bias, mode)] = (dns.handoff_modes["device_edit"], dns.handoff_modes["fast"])
            res[(bias, mode)] = (model.P.clone(), lists, arrays, random.random())
    for bias in biases:
        ref = res[(bias, (False, False))]
        assert took[(bias, (False, False))] == (0, 0)
        for mode in modes[:2]:
            a = res[(bias, mode)]
            assert torch.equal(a[0], ref[0]) and a[1] == ref[1] and a[3] == ref[3], (bias, mode)
            assert all(torch.equal(u, v) for u, v in zip(a[2], ref[2])), (bias, mode)
        assert took[(bias, (False, True))][0] == 0 and took[(bias, (False, True))][1] >= 2, took
    assert any(took[(bias, (True, True))][0] >= 2 for bias in biases), took      # the device path ran
    assert any(took[(bias, (True, True))][0] == 0 and took[(bias, (True, True))][1] >= 2 for bias in biases), took      # too warm for it


def test_acc_mode_accumulates_and_averages(hip):
    """--use-acc-mode (model_cnn.py:374-392): train_begin / F x train_step / train_end = ONE update with the mean gradient and
    the mean of the would-be batch-norm running statistics, every sub-step starting from the same parameters"""
    from denet_amd.model import model_cnn
    B, IMG = 2, 128
    xa, ma = zoo.synthetic_batch(B, IMG, seed=21)
    xb, mb = zoo.synthetic_batch(B, IMG, seed=22)

    def fresh(acc):
        m = zoo.warm_corner_head(zoo.denet34(B, "skip", IMG, class_num=80, seed=1), 4.0, 0.3)
        m.build_train_func("nesterov", use_acc_mode=acc)
        return m
    # (1) two identical sub-steps == one ordinary step on that batch (sum of two equal gradients x 1/2 is exact)
    m1, m2 = fresh(True), fresh(False)
    with pytest.raises(Exception):
        m1.train_step(xa, ma, 0, 0, 0.02, [0.9], 1e-4)           # train_begin is mandatory
    m1.train_begin()
    for _ in range(2):
        random.seed(5)
        m1.train_step(xa, ma, 0, 0, 0.02, [0.9], 1e-4)
    p_mid = m1.P.clone()
    m1.train_end()
    random.seed(5)
    m2.train_step(xa, ma, 0, 0, 0.02, [0.9], 1e-4)
    torch.cuda.synchronize()
    assert torch.equal(p_mid, fresh(False).P)                      # nothing is applied before train_end
    for k in ("P", "M", "S"):
        assert torch.equal(getattr(m1, k), getattr(m2, k)), k
    # (2) two different batches == solver applied to the mean of the two gradients, statistics averaged
    m3, ga, gb = fresh(True), fresh(False), fresh(False)
    m3.train_begin()
    random.seed(6); m3.train_step(xa, ma, 0, 0, 0.02, [0.9], 1e-4)
    random.seed(7); m3.train_step(xb, mb, 0, 0, 0.02, [0.9], 1e-4)
    m3.train_end()
    grads, stats = [], []
    for m, (x, me, seed) in ((ga, (xa, ma, 6)), (gb, (xb, mb, 7))):
        random.seed(seed)
        ctx = m.forward(x, me, train=True)
        m.backward(ctx)
        torch.cuda.synchronize()
        grads.append(m.G.clone()); stats.append(m.S.clone())
    ref = fresh(False)
    g = grads[0] + grads[1]
    ops.solver_step(ref.P[:ref.n_trainable], ref.M[:ref.n_trainable], g[:ref.n_trainable], ref.n_weights, 0.02, 0.9, 0, 1e-4,
                    model_cnn.SOLVER_MODES["nesterov"], 0.5)
    torch.cuda.synchronize()
    assert torch.equal(m3.P, ref.P) and torch.equal(m3.M, ref.M)
    torch.testing.assert_close(m3.S, (stats[0] + stats[1]) * 0.5, rtol=1e-6, atol=1e-7)


def test_adam_solver_vs_oracle(hip):
    """adam updates (denet/model/model_cnn.py:296-305): first / second moments, bias correction, L2 on weights only. The subject is
    the solver, and adam's first steps move every weight by ~lr * sign(g) whatever |g| is - an element whose gradient is rounding
    noise on both sides flips freely - so the convolution passes of THIS test are the direct kernels (their 1e-6 against the
    1e-5 of F(4x4) keeps the flipping elements below the 99.99th percentile the comparison asserts); the Winograd passes'
    gradients are compared in every other whole-network test."""
    # (an emptied table: a decision another file's test left for one of these small geometries would outrank the policy)
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        _generic_step_check("C.B[32,3] BN A nRSN.O[2,32,3] P.A[16] R", (3, 16, 16), 4, solver="adam", steps=3)


def test_augment_and_deconv_layers_vs_oracle(hip):
    """the remaining desc tokens of the operator surface in one training graph: CM (random crop / mirror / flip,
    crop_mirror.py:26-56), B (zero border, border.py:30-33), D (dropout, dropout.py:20-24) and DC (transposed
    convolution with bias, stride 2 and stride 1, deconvolution.py:54-67), forward, gradients and solver update"""
    desc = "CM[14,0.5,0.5] B[1] C.B[32,3] BN A P[2] D[0.3] DC[64,3,2] BNA DC.B[32,3] BNA D[0.5] P.A[16] R"
    model = _generic_step_check(desc, (3, 18, 18), 4, steps=3)
    types = [l.type_name for l in model.layers]
    assert [t for t in types if t in ("crop-mirror", "border", "dropout", "deconv")] == \
        ["crop-mirror", "border", "dropout", "deconv", "deconv", "dropout"]
    dcs = [l for l in model.layers if l.type_name == "deconv"]
    assert dcs[0].output_shape == (4, 64, 16, 16) and dcs[0].use_bias and not dcs[1].use_bias
    # test mode: dropout is the identity, CM takes the centre crop without mirroring
    x = np.random.RandomState(0).uniform(0, 1, (4, 3, 18, 18)).astype(np.float32)
    model.forward(x, None, train=False)
    drop = [l for l in model.layers if l.type_name == "dropout"][0]
    assert drop.output.data is drop.input.data
    cm = model.layers[1]
    got = ops.nhwc_to_nchw(cm.output.data, 3).cpu().numpy()
    assert np.array_equal(got, x[:, :, 2:16, 2:16])
    # JSON surface round trip (deconvolution.py:105-113, dropout.py:36-39, border.py:43-46, crop_mirror.py:72-75)
    j = model.export_json()
    keys = {l["type"]: set(l.keys()) for l in j["layers"]}
    assert {"shape", "stride", "border", "useBias", "bias", "weight"} <= keys["deconv"]
    assert "dropoutRate" in keys["dropout"] and "border" in keys["border"] and {"crop", "mirror", "flip"} <= keys["crop-mirror"]


def test_skip_concat_vs_oracle(hip):
    """SKIP combine mode "concat" (only reachable through the JSON key combineMode, skip.py:93-96)"""
    from denet_amd.model import model_cnn
    B = 4
    np.random.seed(5)
    model = model_cnn.ModelCNN()
    model.batch_size = B
    model.class_num = 10
    model.build("C[32,3] BNA C.B[24,3] A SKIPSRC[0] C.B[40,3] A SKIP[0] C[32,1] BNA P.A[16] R", (3, 16, 16), "relu", "half",
                ["he-backward"])
    j = model.export_json()
    rng = np.random.RandomState(6)
    for i, l in enumerate(j["layers"]):
        if l["type"] == "skip":
            l["combineMode"] = "concat"
            l["layers"] = []
            nxt = j["layers"][i + 1]
            nxt["shape"] = (32, 64, 1, 1)
            nxt["weight"] = rng.normal(0, 0.2, (32, 64, 1, 1)).astype(np.float32)
    model2 = model_cnn.load_from_json(j, B)
    skip = [l for l in model2.layers if l.type_name == "skip"][0]
    assert skip.combine_mode == "concat" and skip.output_shape == (B, 64, 16, 16)
    x = rng.uniform(0, 1, (B, 3, 16, 16)).astype(np.float32)
    metas = [{"image_class": int(rng.randint(0, 10)), "bbox": [], "class": []} for _ in range(B)]
    om = OM.OracleModel(model2.export_json(), B)
    model2.build_train_func("nesterov")
    for it in range(2):
        cost, _ = model2.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
        ocost, _ = _forced_step_check(model2, om, x, metas, it, 0.05, 0.9, 1e-4, "nesterov", None)
        assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


def test_skip_projection_vs_oracle(hip):
    """SKIP with a channel mismatch projects the tap with a 1x1 convolution (denet/layer/skip.py:78-86)"""
    desc = "C[32,3] BNA SKIPSRC[0] C[64,3,2] BNA PI[2] SKIP[0] BNA P.A[16] R"
    model = _generic_step_check(desc, (3, 16, 16), 4, solver="sgd")
    skip = [l for l in model.layers if l.type_name == "skip"][0]
    assert len(skip.layers) == 2 and skip.layers[1].filter_shape == (64, 32, 1, 1)


@pytest.mark.parametrize("head,rule", [("DND.JB[0.5,1,1]", 0), ("DND.B[0.4,2,0.5]", 1), ("DND[0.5,1,1]", 1),
                                       ("DND[0.5,1,1,0.7]", 0), ("DND[0.5,1,0,0.7]", 0)])
def test_denet_head_variants_vs_oracle(hip, head, rule):
    """joint-fitness classes + bounded-IoU box cost (denet_detect.py:180-183, 266-286) and the CUDA tap rule"""
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1, head_desc=zoo.DENET34_SKIP_DESC.replace("DND[0.5,1,1]", head))
    rng = np.random.RandomState(5)
    dconv = model.layers[40].layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    dconv.beta.set_value(rng.normal(0, 0.05, dconv.beta.value.shape))
    model.layers[31].tap_rule = rule
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=3)
    om = OM.OracleModel(model.export_json(), B, tap_rule=rule)
    model.build_train_func("nesterov")
    random.seed(9)
    cost, costs = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    roi_lists = model.layers[31].sample_bbox_list
    ocost, ocosts = _forced_step_check(model, om, x, metas, 0, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
    assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)
    for c, oc in zip(costs, ocosts):
        assert abs(c - oc) <= 1e-4 * max(abs(oc), 1e-6), (costs, ocosts)
    ys, xs = om.taps
    taps_ref = (ys[:, :, None] * (IMG // 8) + xs[:, None, :]).reshape(ys.shape[0], -1)
    assert np.array_equal(model.layers[31]._taps.cpu().numpy(), taps_ref)
    if "J" in head:
        assert model.layers[40].s0 == 401
    if head.endswith("0.7]"):       # independent fitness head (4th argument = its cost factor)
        assert model.layers[40].s2 == 6 and model.layers[40].layers[0].filter_shape[0] == 81 + model.layers[40].s1 + 6


def test_denet_center_corner_variant_vs_oracle(hip):
    """DNC.C (denet_corner.py:62-71 tag C): a fifth 'centre' map in the corner cost, the RoI proposal and its score"""
    B, IMG = 2, 128
    desc = zoo.DENET34_SKIP_DESC.replace("DNC[96,100]", "DNC.C[96,100]")
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1, head_desc=desc)
    dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
    dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
    dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
    assert dnc.corner_num == 5
    rng = np.random.RandomState(5)
    dconv = dnd.layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=3)
    om = OM.OracleModel(model.export_json(), B)
    model.build_train_func("nesterov")
    random.seed(9)
    cost, costs = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    roi_lists = dns.sample_bbox_list
    # the proposal itself: exact against the C++ oracle on the product's own 5-map corner tensor
    lists = OM.oracle_build_samples(dnc.corner_pr.cpu().numpy(), dns.corner_threshold, dns.sample_num, 1024, 0)
    assert sum(len(l) for l in lists) > 0
    random.seed(9)
    ref_lists = OL.edit_samples(lists, metas, dns.sample_count, dns.random_sample, dns.sample_gt)
    assert [[p for p, _ in l] for l in ref_lists] == [[p for p, _ in l] for l in roi_lists]
    ocost, ocosts = _forced_step_check(model, om, x, metas, 0, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
    assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


def _lattice_corner_map(seed, B, H, W, n_tl, n_br):
    """a corner map whose candidate scores are ALL distinct by construction (random continuous maps give ~70 exact fp32 ties among
    the 23 040 best of 10^5 candidates: |pr_f - pr_t| lives on a lattice of ~10^-6). Only top-left and bottom-right corners fire;
    their log-probabilities are distinct multiples of 2^-16 - TL cell i: -(a_i + 1) 2^-16, BR cell j: -512 (b_j + 1) 2^-16, a / b
    random permutations - every other cell holds (log(1-P), log P) = (0, -9). All sums of the reference's score expression
    (denet_sparse.cc:276-306) are then exact in fp32 and |pr_f - pr_t| = 18 + (a_i + 1 + 512 (b_j + 1)) 2^-16 is different for every
    (TL, BR) pair; expf of values 1.5e-5 apart differs by ~250 ulp, so the scores are distinct too."""
    assert n_tl < 512 and 512 * (n_br + 1) / 65536.0 < 4.5
    rng = np.random.RandomState(seed)
    pr = np.zeros((B, 2, 4, H, W), np.float32)
    pr[:, 1] = -9.0
    for b in range(B):
        for c, n, scale in ((0, n_tl, 1.0), (3, n_br, 512.0)):
            cells = rng.choice(H * W, n, replace=False)
            vals = -(rng.permutation(n) + 1.0) * scale / 65536.0
            pr[b, 1, c].reshape(-1)[cells] = vals.astype(np.float32)
    return np.ascontiguousarray(pr)


def _tie_groups_equal(got, ref, what):
    """two ranked lists [n, 5] (pr, box): identical scores, and identical boxes inside every group of equal score (as sets)"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[:, 0], ref[:, 0]), what + ": score sequences differ"
    n, i = len(got), 0
    while i < n:
        j = i
        while j + 1 < n and got[j + 1, 0] == got[i, 0]:
            j += 1
        assert sorted(map(tuple, got[i:j + 1, 1:].tolist())) == sorted(map(tuple, ref[i:j + 1, 1:].tolist())), (what, i, j)
        i = j + 1


@pytest.mark.parametrize("sn_model", [24, 48])
def test_roi_clustering_device_path_vs_oracle(hip, sn_model):
    """DNS nmsThreshold < 1 (apply_cluster, denet_sparse.cc:165-242, 541-542): (1) the device proposal asked for the
    10 * sn^2 best candidates + the native host clustering against the C++ oracle on maps WITHOUT score ties - the clustered lists
    are compared exactly; (2) a DeNet-34 skip training step with `DNS[7,sn,0.01,0.1,0,0.5]`: the layer's RoI lists against the
    oracle's clustering, and the step stays in op-by-op parity. sn = 48 is the RoI grid of the v2 models the reference advertises
    (README.md:132,145; papers/dss/denet101.sh:19): 10 x 2304 = 23 040 candidates per image, more than one LDS sort holds - the
    two-level final sort of csrc/samples.hip (pair_finalize_big_kernel). Its tie-free map is CONSTRUCTED (_lattice_corner_map:
    128x128 cells, every candidate score distinct by design); in (2), where the map is the model's own and holds groups of equal
    scores, the oracle clusters the product's ranked order (the order inside such a group is the one thing the reference leaves to
    std::partial_sort) after that ranking has been checked group by group - there is no branch that skips the list comparison."""
    from tests.test_host import _distinct_corner_map
    sn = 6 if sn_model == 24 else 48
    S = sn * sn
    if sn_model == 24:
        # random continuous maps: ~2 000 candidates per image, an exact fp32 tie among the 360 best is rare - the first seed without
        for seed in range(11, 40):
            pr = _distinct_corner_map(seed, 4, 64, 64, 90)
            top, _, _, tc = OM.oracle_build_samples_raw(pr, 0.01, 19, 1024, 0)
            if all(tc[b] >= 10 * S and len(np.unique(top[b, :10 * S, 0])) == 10 * S for b in range(4)):
                break
    else:
        pr = _lattice_corner_map(11, 2, 128, 128, 420, 420)
    Hm = pr.shape[3]
    d = torch.from_numpy(pr).cuda()
    box, absd, cnt = ops.build_samples(d, 0.01, 10 * S, 1024, 0)
    raw = ops.samples_finish_host(box.cpu(), absd.cpu(), cnt.cpu(), Hm, Hm).numpy()
    assert int(cnt.min()) == 10 * S
    for b in range(pr.shape[0]):
        assert len(np.unique(raw[b, :10 * S, 0])) == 10 * S, "the test map must not produce score ties"
    changed = 0
    for thr in (0.3, 0.6):
        got, gcnt = ops.cluster_samples_host(raw, cnt.cpu().numpy(), thr, S)
        ref, _, _, rcnt = OM.oracle_build_samples_raw(pr, 0.01, sn, 1024, 0, thr)
        plain, _, _, _ = OM.oracle_build_samples_raw(pr, 0.01, sn, 1024, 0)
        assert np.array_equal(gcnt, rcnt)
        for b in range(pr.shape[0]):
            assert np.array_equal(got[b, :gcnt[b]], ref[b, :rcnt[b]]), (thr, b)
            changed += int(not np.array_equal(ref[b], plain[b]))
    assert changed > 0, "clustering changed nothing on the test maps"

    B, IMG = 2, 128
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "DNS[7,%d,0.01,0.1,0,0.5]" % sn_model)
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1, head_desc=desc)
    dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
    dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
    assert dns.cluster and dns.proposal_count == 10 * sn_model * sn_model and dns.export_json()["nmsThreshold"] == 0.5
    rng = np.random.RandomState(5)
    dconv = model.layers[-1].layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 2.5, 0.5)            # a busy detector: more than 576 candidates per image
    x, metas = zoo.synthetic_batch(B, IMG, seed=3)
    om = OM.OracleModel(model.export_json(), B)
    model.build_train_func("nesterov")
    random.seed(9)
    cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    roi_lists = dns.sample_bbox_list
    clustered, ccnt = dns._raw_samples             # what the layer's clustering left (before the editing)
    cmap = dnc.corner_pr.cpu().numpy()
    SC = dns.sample_count
    plain = OM.oracle_build_samples(cmap, dns.corner_threshold, dns.sample_num, 1024, 0)
    assert all(len(l) == SC for l in plain), "the detector must produce more candidates than RoIs"
    # (a) the ranking of the 10 sn^2 best candidates of the product's own map against the oracle's, group by group of equal score
    cbox, cabsd, ccn = ops.build_samples(dnc.corner_pr, dns.corner_threshold, 10 * SC, 1024, 0)
    ranked = ops.samples_finish_host(cbox.cpu(), cabsd.cpu(), ccn.cpu(), cmap.shape[3], cmap.shape[4]).numpy()
    big = int(np.ceil((10 * SC) ** 0.5))
    oranked, _, _, orc = OM.oracle_build_samples_raw(cmap, dns.corner_threshold, big, 1024, 0)
    ties = 0
    lists = []
    for b in range(B):
        n = int(ccn[b])
        assert n == min(int(orc[b]), 10 * SC)
        # (a group cut by the end of the list may keep other members of the boundary score on either side: compared up to it)
        last = n
        if n == 10 * SC:
            while last > 0 and ranked[b, last - 1, 0] == ranked[b, n - 1, 0]:
                last -= 1
        _tie_groups_equal(ranked[b, :last], oranked[b, :last], "ranking of image %d" % b)
        ties += last - len(np.unique(ranked[b, :last, 0]))
        # (b) the ORACLE's grouping (apply_cluster + final ranking) of that ranked list = the layer's clustered proposal
        oc = OM.oracle_cluster_ranked(ranked[b, :n], 0.5, SC)
        assert len(oc) == int(ccnt[b])
        _tie_groups_equal(np.asarray(clustered[b, :len(oc)], np.float32), oc, "clustered list of image %d" % b)
        lists.append([(float(r[0]), tuple(float(v) for v in r[1:5])) for r in clustered[b, :len(oc)]])
    assert any(len(l) for l in lists)
    assert [[p for p, _ in l] for l in lists] != [[p for p, _ in l] for l in plain], "clustering changed nothing"
    print("sn = %d: %d candidates in groups of equal score among the clustering inputs (ranking and grouping compared "
          "group-wise, nothing skipped)" % (sn_model, ties))
    # (c) the training-time editing (denet_sparse.py:184-201) replayed by the oracle on the clustered proposal: exact
    random.seed(9)
    ref_lists = OL.edit_samples(lists, metas, SC, dns.random_sample, dns.sample_gt)
    assert ref_lists == roi_lists, "RoI lists differ from the reference editing of the clustered proposal"
    ocost, _ = _forced_step_check(model, om, x, metas, 0, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
    assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


@pytest.mark.parametrize("IMG", [128, 512])
def test_denet101_wide_train_step_vs_oracle(hip, IMG):
    """BASELINE config 5 at reduced size: ResNet-101 bottleneck backbone, three skip scales (one through a plain
    SKIPSRC), SPLIT points, 48x48 = 2304 RoIs per image, joint-fitness + bounded-IoU head (papers/dss/denet101.sh).
    IMG = 512 (the recipe's resolution, 128x128 corner map, 16x16 last-stage maps): FREE-RUNNING forward as well, judged by an
    fp64 ARBITER (round-5 verdict item 4): the same restatement evaluated in float64 (oracle/model.py: float64_arbiter) is the
    reference, and the product (fp32 HIP kernels) and the fp32 oracle are both measured against it, layer by layer, in both
    rel_close clauses. Measured on MI355X (tools/exp/d101_arbiter.py, 2026-09-30): the product's distance to fp64 is 1.07-1.37x the
    fp32 oracle's at EVERY layer - 6.6e-7 vs 6.2e-7 behind the stem, 3.3e-4 vs 2.6e-4 (element-wise p99.99) at layer 24, 8.5e-4 vs
    6.7e-4 at layer 37, 3.0e-3 vs 2.4e-3 behind the last stage (batch statistics over 256 values at B = 1), 3.7e-3 vs 2.9e-3 at
    the head's last layer; max-norm 1.0e-3 vs 7.6e-4 there. Neither fp32 evaluation of a 101-layer network stays element-wise
    within 1e-3 of the fp64 value beyond layer 37: that is fp32, not a kernel. Asserted, with no allowance of its own: costs 1e-3
    against fp64; layers up to 37 and the corner map: the north star's 1e-3 in both clauses against fp64; every layer, both
    clauses: the product no farther from fp64 than max(1e-3, 1.5 x the fp32 oracle's distance); max-norm <= 1.5e-3 everywhere.
    The op-by-op pass behind it
    (every op on the product's own inputs) holds 2e-4 per op."""
    B = 1           # IMG = 512: the resolution of papers/dss/denet101.sh:19 (BASELINE config 5), 128x128 corner map
    model = zoo.denet101(B, "wide", IMG, class_num=80, seed=1,
                         head_desc=zoo.DENET101_WIDE_DESC.replace("DND[0.5,1,1]", "DND.JB[0.5,1,1]"))
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    dnd, dns = by_type("denet-detect"), by_type("denet-sparse")
    assert dns.sample_count == 2304 and dns.output_shape[1] == 7 * 7 * 128 + 2
    rng = np.random.RandomState(5)
    dconv = dnd.layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=3)
    json_before = model.export_json()                                             # (the weights BEFORE the step)
    om = OM.OracleModel(json_before, B)
    om_free = OM.OracleModel(json_before, B) if IMG == 512 else None
    model.build_train_func("nesterov")
    random.seed(9)
    cost, costs = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
    roi_lists = dns.sample_bbox_list
    assert len(roi_lists[0]) == 2304
    if IMG == 512:
        random.seed(9)
        fcost, fcosts = om_free.forward_costs(x, metas, sample_override=roi_lists)          # the fp32 oracle, forward only
        with OM.float64_arbiter():
            om64 = OM.OracleModel(json_before, B)
            random.seed(9)
            acost, acosts = om64.forward_costs(x, metas, sample_override=roi_lists)         # the arbiter
        assert np.array_equal(om_free.taps[0], om64.taps[0]) and np.array_equal(om_free.taps[1], om64.taps[1])
        assert abs(cost - acost) <= 1e-3 * abs(acost), (cost, acost)
        for c, oc in zip(costs, acosts):
            assert abs(c - oc) <= 1e-3 * max(abs(oc), 1e-6), (costs, acosts)
        table = {}
        acts = _product_acts(model)
        acts["corner_pr"] = by_type("denet-corner").corner_pr.cpu().numpy()
        for i, a in acts.items():
            ref64 = om64.corner_pr if i == "corner_pr" else om64.acts[i]
            ref32 = om_free.corner_pr if i == "corner_pr" else om_free.acts[i]
            p, o = _err_stats(a, ref64), _err_stats(ref32, ref64)
            what = "corner_pr" if i == "corner_pr" else "L%d %s" % (i, model.layers[i].type_name)
            table[what] = {"product_vs_fp64": p, "oracle32_vs_fp64": o}
            for clause, pv, ov in (("element-wise p99.99", p[0], o[0]), ("max-norm", p[1], o[1])):
                assert pv <= max(1e-3, 1.5 * ov), "%s %s: product %.2e from fp64, the fp32 oracle %.2e" % (what, clause, pv, ov)
            assert p[1] <= 1.5e-3, (what, p)
            if i == "corner_pr" or i <= 37:
                assert p[0] <= 1e-3 and p[1] <= 1e-3, "%s: %.2e / %.2e against fp64 (north star: 1e-3)" % (what, p[0], p[1])
        worst = max(table.items(), key=lambda kv: kv[1]["product_vs_fp64"][0])
        print("DeNet-101 wide 512x512 free-running vs the fp64 arbiter, worst layer:", worst)
        out = os.environ.get("D101_ARBITER_REPORT_PATH")
        if out:
            import json
            with open(out, "w") as f:
                json.dump({"test": "test_denet101_wide_train_step_vs_oracle[512]", "columns": "element-wise p99.99, max-norm", "layers": table}, f, indent=1)
        del om_free, om64
    ocost, ocosts = _forced_step_check(model, om, x, metas, 0, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
    assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)
    ys, xs = om.taps
    taps_ref = (ys[:, :, None] * (IMG // 4) + xs[:, None, :]).reshape(ys.shape[0], -1)
    assert np.array_equal(dns._taps.cpu().numpy(), taps_ref)


def test_model_train_cli_trains_and_checkpoints(hip, tmp_path):
    """the model-train flag surface: a few epochs on synthetic data reduce the cost; the .mdl.gz reloads"""
    from denet_amd.model import train as train_mod, model_cnn
    prefix = str(tmp_path / "m")
    args = train_mod.build_parser().parse_args(
        ["--train", "synthetic,samples=32,image=32,classes=10", "--batch-size", "16", "--epochs", "6", "--seed", "3",
         "--solver", "nesterov", "--learn-rate", "0.05", "--learn-momentum", "0.9", "--learn-decay", "1e-4",
         "--learn-anneal", "0.5", "--learn-anneal-epochs", "4", "--border-mode", "half", "--output-prefix", prefix,
         "--model-desc"] + zoo.CIFAR3_DESC.split())
    random.seed(args.seed)
    np.random.seed(args.seed)
    data = train_mod.load_dataset(args.train, args.seed)
    model, costs = train_mod.train(args, data, log=lambda *a: None)
    assert np.isfinite(costs).all() and costs[-1] < 0.7 * costs[0], costs
    m2 = model_cnn.load_from_file(prefix + "_epoch005_final.mdl.gz", 16)
    x, metas, _ = data.export(16)
    p1 = model.predict_output_step(x[:16])
    p2 = m2.predict_output_step(x[:16])
    np.testing.assert_allclose(p1, p2, rtol=1e-5, atol=1e-6)
