"""The batch-norm kernels (csrc/bn.hip with bn_reduce.h and bn_pointwise.h) against float64 on every row mapping.

The arbiter is bn_reference.bn_ref64 (torch float64 on the CPU, autograd); the bounds are bn_reference.bn_bounds: per channel, max
norm, the statistics from the code (float64 sums, one rounding), y / dx / dgamma with constants measured on the host from the
restated float32 expressions (tests/test_bn_reference_host.py) - no number here comes from the device. The case table
(bn_reference.CASES) is built from bn_map so that every first-stage and pointwise kernel runs its row loop once, twice and three
or more times, with a last sweep and a last workgroup of one row, M < RS and M = 1, LC from 1 to 256 and gx up to 5;
test_case_table_is_the_librarys_mapping ties those claims to the built library.

ReLU: an element is undecided when |pre64| is inside the y bound; there the reference takes the device's decision, everywhere
else the device must decide as float64 does, and at most 1e-3 of a case may be undecided."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from denet_amd import ops
import bn_reference as R

pytestmark = pytest.mark.gpu

EPS = R.EPS


def _id(shape):
    return "x".join(str(v) for v in shape)


@functools.lru_cache(maxsize=2)
def _inputs(ci):
    """the host tensors of case ci: made once, shared by the tests (and modes) that run it, never written"""
    return R.bn_case(R.CASES[ci], R.case_seed(ci))


def _cuda(c):
    return {k: (v.cuda() if v is not None else None) for k, v in c.items()}


def _hold(name, got, want, bound, report=None):
    """every element of got within its channel's bound of the float64 value; prints the worst error as a share of the bound"""
    got = got.detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound.expand_as(err), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s: worst error %.3e = %.3f of its bound" % (name, float(err.max()), worst))
    if report is not None:
        report[name] = worst
    assert worst <= 1.0, "%s: %d of %d elements outside the bound, the worst at %.3f of it" % (name, int((ratio > 1).sum()), ratio.numel(), worst)


def _hold_forward(got, ref, b, keys=("y", "mean", "inv", "run_mean", "run_stdinv")):
    for k in keys:
        _hold(k, got[k], ref[k], b[k])


def _decide(ref, b, passed_dev):
    """the module's ReLU rule; returns the mask the float64 backward pass takes"""
    mask, und, wrong = R.relu_decisions(ref["pre"], b["y"], passed_dev)
    print("ReLU: %d of %d undecided" % (int(und.sum()), und.numel()))
    assert not bool(wrong.any()), "%d decided elements pass the ReLU on one side only" % int(wrong.sum())
    assert int(und.sum()) <= R.UNDECIDED_MAX * und.numel(), (int(und.sum()), und.numel())
    return mask


def test_case_table_is_the_librarys_mapping(hip):
    """denet_bn_stats_partial returns the rows of the partial list it wrote = gridDim.y of every pass over that (M, C): the
    restated bn_map, from which the case tables' sweeps are derived, is the library's; and the list it leaves sums to float64's"""
    seen = set()
    for shape in R.CASES + [c[:4] for c in R.POOL_CASES]:
        M, C = int(np.prod(shape[:-1])), shape[-1]
        if (M, C) in seen:
            continue
        seen.add((M, C))
        g = torch.Generator().manual_seed(M + C)
        x = torch.randn(M, C, generator=g)
        ws = ops._bn_ws(M, C)
        rows = ctypes.c_int(-1)
        ops.check(hip.denet_bn_stats_partial(ops.ptr(x.cuda()), ops.ptr(ws), ctypes.byref(rows), M, C, ops.stream_ptr()), "bn_stats_partial")
        torch.cuda.synchronize()
        m = R.bn_map(M, C)
        assert rows.value == m.gy, (shape, rows.value, m)
        assert ws.numel() * ws.element_size() >= max(m.gy, 64) * 2 * C * 8 + 2 * C * 4
        p = torch.empty(m.gy, 2, C, dtype=torch.float64, device="cuda")
        ops.check(hip.denet_bn_stats_partial(ops.ptr(x.cuda()), ops.ptr(p), ctypes.byref(rows), M, C, ops.stream_ptr()), "bn_stats_partial")
        s = p.sum(dim=0).cpu()
        xd = x.double()
        assert float((s[0] - xd.sum(0)).abs().max()) <= 1e-12 * float(xd.abs().sum(0).max()), shape
        assert float((s[1] - (xd * xd).sum(0)).abs().max()) <= 1e-12 * float((xd * xd).sum(0).max()), shape


@pytest.mark.parametrize("mi", range(len(R.MODES)), ids=["relu%d-res%d" % m for m in R.MODES])
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=[_id(s) for s in R.CASES])
def test_training_forward_and_backward_vs_fp64(hip, ci, mi):
    """bn_fwd_train + bn_bwd: y, the saved and the running statistics, dx, dgamma, dbeta inside their bounds, dres exact; channel 0
    has its variance below eps, channel 1 is constant (var = 0, the clamp), channel 2 sits at mean = 300 std; the running
    statistics start away from (0, 1) and meet every momentum. With a ReLU and no residual both mask forms run - from y, and
    recomputed from x with beta - and give the same bits"""
    relu, res = R.MODES[mi]
    mom = R.case_momentum(ci, mi)
    c = _inputs(ci)
    d = _cuda(c)
    C = c["x"].shape[-1]
    rs_h, rs_d = (c["res"], d["res"]) if res else (None, None)
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    y, sm, si = ops.bn_fwd_train(d["x"], d["gamma"], d["beta"], rm, rv, mom, EPS, relu=relu, res=rs_d)
    dgamma, dbeta = torch.full((C,), 7.0).cuda(), torch.full((C,), 7.0).cuda()
    dx, dres, dg, db = ops.bn_bwd(d["x"], y, d["dy"], d["gamma"], sm, si, relu=relu, want_dres=res, dgamma=dgamma, dbeta=dbeta)
    assert dg is dgamma and db is dbeta
    torch.cuda.synchronize()
    run = (c["run_mean"], c["run_stdinv"])
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, relu, rs_h, None if relu else c["dy"], run=run, momentum=mom)
    b = R.bn_bounds(ref, c["gamma"])
    _hold_forward({"y": y, "mean": sm, "inv": si, "run_mean": rm, "run_stdinv": rv}, ref, b)
    if relu:
        mask = _decide(ref, b, y > 0)
        ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, relu, rs_h, c["dy"], mask=mask)
        b = R.bn_bounds(ref, c["gamma"])
    for k, t in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        _hold(k, t, ref[k], b[k])
    if res:
        assert torch.equal(dres.double().cpu().reshape(ref["dres"].shape), ref["dres"])         # a masked copy
    else:
        assert dres is None
    if relu and not res:
        dx2, _, dg2, db2 = ops.bn_bwd(d["x"], None, d["dy"], d["gamma"], sm, si, relu=True, beta=d["beta"])
        assert torch.equal(dx2, dx) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# ------------------------------------------------------------------------------------------------- partial lists made elsewhere
LIST_CASES = (3, 6, 9)          # (3, 5, 7, 24): M < RS; (1, 80, 82, 160): gx = 5, 2 sweeps; (1, 3, 455, 1536): 3 sweeps


@pytest.mark.parametrize("rows", R.FINAL_ROWS)
@pytest.mark.parametrize("ci", LIST_CASES, ids=[_id(R.CASES[i]) for i in LIST_CASES])
def test_forward_from_partial_lists_vs_fp64(hip, ci, rows):
    """bn_fwd_train(pre=(list, rows)) and bn_fwd_train_link (denet_bn_stats_final) + materialise() on a list another pass would
    have left: float64 sums over uneven, partly empty row sets (bn_reference.split_partials). The list is exact, so the
    statistics and y get the bounds of the training test"""
    mi = (ci + rows) % len(R.MODES)
    relu, res = R.MODES[mi]
    mom = R.case_momentum(ci, rows)
    c = _inputs(ci)
    d = _cuda(c)
    rs_h, rs_d = (c["res"], d["res"]) if res else (None, None)
    p = R.split_partials(c["x"], rows, np.random.RandomState(1000 * ci + rows)).cuda()
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, relu, rs_h, run=(c["run_mean"], c["run_stdinv"]), momentum=mom)
    b = R.bn_bounds(ref, c["gamma"])
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    y, sm, si = ops.bn_fwd_train(d["x"], d["gamma"], d["beta"], rm, rv, mom, EPS, relu=relu, res=rs_d, pre=(p, rows))
    _hold_forward({"y": y, "mean": sm, "inv": si, "run_mean": rm, "run_stdinv": rv}, ref, b)
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    link, sm, si = ops.bn_fwd_train_link(d["x"], d["gamma"], d["beta"], rm, rv, (p, rows), mom, EPS, relu=relu, res=rs_d)
    assert link.result is None
    _hold_forward({"y": link.materialise(), "mean": sm, "inv": si, "run_mean": rm, "run_stdinv": rv}, ref, b)


@pytest.mark.parametrize("rows", R.FINAL_ROWS)
@pytest.mark.parametrize("ci", LIST_CASES, ids=[_id(R.CASES[i]) for i in LIST_CASES])
def test_backward_from_partial_lists_vs_fp64(hip, ci, rows):
    """bn_bwd_link(pre=(list, rows)) (denet_bn_bwd_final) + materialise() (denet_bn_bwd_apply) on float64 lists of (sum g,
    sum g * xhat) as a data-gradient pass would have left them: dgamma, dbeta, dx inside the training test's bounds, dres exact"""
    mi = (ci + rows) % len(R.MODES)
    relu, res = R.MODES[mi]
    c = _inputs(ci)
    d = _cuda(c)
    C = c["x"].shape[-1]
    rs_h, rs_d = (c["res"], d["res"]) if res else (None, None)
    y, sm, si = ops.bn_fwd_train(d["x"], d["gamma"], d["beta"], d["run_mean"].clone(), d["run_stdinv"].clone(), 0.9, EPS, relu=relu, res=rs_d)
    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, relu, rs_h)
    mask = _decide(fwd, R.bn_bounds(fwd, c["gamma"]), y > 0) if relu else None
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, relu, rs_h, c["dy"], mask=mask)
    b = R.bn_bounds(ref, c["gamma"])
    p = R.split_partials((ref["g"], ref["g"] * ref["xhat"]), rows, np.random.RandomState(2000 * ci + rows)).cuda()
    dgamma, dbeta = torch.full((C,), 7.0).cuda(), torch.full((C,), 7.0).cuda()
    link, dres = ops.bn_bwd_link(d["x"], y, d["dy"], d["gamma"], sm, si, relu=relu, want_dres=res, dgamma=dgamma, dbeta=dbeta,
                                 beta=d["beta"], pre=(p, rows))
    dx = link.materialise()
    for k, t in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        _hold(k, t, ref[k], b[k])
    if res:
        assert torch.equal(dres.double().cpu().reshape(ref["dres"].shape), ref["dres"])
    else:
        assert dres is None


# ------------------------------------------------------------------------------------------------- BN + ReLU + max pool
def _hold_pooled(ref, tol, yp, arg, shape, k, s, p, need_dead=True):
    """the pooled output of relu(bn(x)) and its taps against the float64 map ref (bn_ref64, relu): values within the y bound tol
    [C] of the window maximum; every tap in bounds and at an element within the bound of that maximum; the float64 argmax where the
    maximum is positive and leads the runner-up by more than twice the bound; value 0 at the first in-bounds tap in scan order where
    the whole window is decidedly <= 0. Returns (flat index of each window's tap in the input [N, OH, OW, C], float64 argmax)"""
    N, H, W, C = shape
    mx, vals, near = R.pool_ref64(ref["y"].reshape(shape), k, s, p, tol)
    ypd, argl = yp.double().cpu(), arg.long().cpu()
    assert ypd.shape == mx.shape and bool(torch.isfinite(ypd).all())
    _hold("y_pool", yp, mx, tol)
    assert int(argl.max()) < k * k
    assert bool(near.gather(-1, argl[..., None]).all()), "a tap outside the map, or at an element further than the bound from the maximum"
    top = vals.topk(2, dim=-1).values
    clear = (mx > 0) & (top[..., 0] - top[..., 1] > 2 * tol)
    assert bool((argl[clear] == vals.argmax(dim=-1)[clear]).all())
    pmx = R.pool_ref64(ref["pre"].reshape(shape), k, s, p, tol)[0]
    dead = pmx < -tol
    first = (vals > -float("inf")).int().argmax(dim=-1)
    assert bool((ypd[dead] == 0).all()) and bool((argl[dead] == first[dead]).all())
    print("windows: %d, a clear float64 argmax in %d, decidedly dead %d" % (mx.numel(), int(clear.sum()), int(dead.sum())))
    if need_dead:
        assert bool(dead.any()) and bool(clear.any())
    return argl


@pytest.mark.parametrize("case", R.POOL_CASES, ids=[_id(c) for c in R.POOL_CASES])
def test_bn_relu_pool_vs_fp64(hip, case):
    """bn_relu_pool_fwd_train(xhat=True), bn_relu_pool_bwd and the pooled-sums route bn_relu_pool_bwd_pooled against float64
    directly (not through bn_fwd_train + maxpool_fwd, to which test_kernels_gpu.py holds them bit for bit). The backward reference
    routes the pooled gradient through the device's taps - validated first - and takes the ReLU decision of a window's target
    element by the module's rule, the device's decision being y_pool > 0. xhat_pool: (x - mean) * inv at the tap, inside
    4 u (|x| + |mean|) inv: the rounding of the float32 mean (u |mean|), of the difference (u |x - mean|), of inv and of the
    product (u |x - mean| each), times inv. The caps of the two grid-strided pooled launches at 65536 workgroups are NOT reached:
    they need more than 16M float4s of pooled output"""
    N, H, W, C, k, s, p = case
    shape = (N, H, W, C)
    c = R.bn_case(shape, sum(case), res=False)
    d = _cuda(c)
    mom = R.MOMENTA[sum(case) % 3]
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    yp, arg, sm, si, xh = ops.bn_relu_pool_fwd_train(d["x"], d["gamma"], d["beta"], rm, rv, k, s, p, mom, EPS, xhat=True)
    g = torch.Generator().manual_seed(sum(case) + 1)
    dyp = torch.randn(yp.shape, generator=g)
    dx, dg, db = ops.bn_relu_pool_bwd(d["x"], dyp.cuda(), arg, d["gamma"], d["beta"], sm, si, k, s, p)
    dg3, db3 = torch.full((C,), 7.0).cuda(), torch.full((C,), 7.0).cuda()
    dx3 = ops.bn_relu_pool_bwd_pooled(d["x"], xh, yp, dyp.cuda(), arg, d["gamma"], d["beta"], sm, si, k, s, p, dg3, db3)
    torch.cuda.synchronize()

    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, True, run=(c["run_mean"], c["run_stdinv"]), momentum=mom)
    b = R.bn_bounds(fwd, c["gamma"])
    _hold_forward({"mean": sm, "inv": si, "run_mean": rm, "run_stdinv": rv}, fwd, b, keys=("mean", "inv", "run_mean", "run_stdinv"))
    argl = _hold_pooled(fwd, b["y"], yp, arg, shape, k, s, p, need_dead=H * W > 1)

    # backward: the pooled gradient through the validated taps; the ReLU decision of each window's target element
    dy_in, flat = R.pool_route64(dyp, argl, shape, k, s, p)
    pre_at = fwd["pre"].reshape(-1)[flat]
    und = pre_at.abs() <= b["y"]
    passed_dev, want = yp.cpu() > 0, pre_at > 0
    assert not bool(((~und) & (passed_dev != want)).any())
    assert int(und.sum()) <= R.UNDECIDED_MAX * und.numel(), (int(und.sum()), und.numel())
    mask = torch.zeros(N * H * W * C, dtype=torch.bool)
    mask[flat.reshape(-1)] = torch.where(und, passed_dev, want).reshape(-1)
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, True, None, dy_in, mask=mask.reshape(-1, C))
    bb = R.bn_bounds(ref, c["gamma"])
    for k_, t in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("dx", dx3), ("dgamma", dg3), ("dbeta", db3)):
        _hold(k_, t, ref[k_], bb[k_])
    x_at = c["x"].double().reshape(-1)[flat]
    xhat_at = ref["xhat"].reshape(-1)[flat]
    _hold("xhat_pool", xh, xhat_at, 4 * R.U * (x_at.abs() + fwd["mean"].abs()) * fwd["inv"])


POOL_LIST_CASES = (2, 6)            # (3, 17, 23, 32, 3, 2, 1), (1, 20, 15, 12, 3, 2, 1)


@pytest.mark.parametrize("rows", (2048,) + R.FOLD_ROWS)
@pytest.mark.parametrize("pi", POOL_LIST_CASES, ids=[_id(R.POOL_CASES[i]) for i in POOL_LIST_CASES])
def test_bn_relu_pool_from_partial_lists_vs_fp64(hip, pi, rows):
    """bn_relu_pool_fwd_train(pre=(list, rows)): 2048 rows go to the final kernel as they are, longer lists through
    bn_stats_fold_kernel first (per = ceil(rows / 64) rows a slice; 2049, 2111 and 4097 end in a short slice of 3, 32 and 2 rows,
    16384 is the stem's full list): statistics and pooled output against float64"""
    case = R.POOL_CASES[pi]
    N, H, W, C, k, s, p = case
    shape = (N, H, W, C)
    c = R.bn_case(shape, sum(case), res=False)
    d = _cuda(c)
    mom = R.MOMENTA[rows % 3]
    pl = R.split_partials(c["x"], rows, np.random.RandomState(rows + pi)).cuda()
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    yp, arg, sm, si = ops.bn_relu_pool_fwd_train(d["x"], d["gamma"], d["beta"], rm, rv, k, s, p, mom, EPS, pre=(pl, rows))
    torch.cuda.synchronize()
    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], EPS, True, run=(c["run_mean"], c["run_stdinv"]), momentum=mom)
    b = R.bn_bounds(fwd, c["gamma"])
    _hold_forward({"mean": sm, "inv": si, "run_mean": rm, "run_stdinv": rv}, fwd, b, keys=("mean", "inv", "run_mean", "run_stdinv"))
    _hold_pooled(fwd, b["y"], yp, arg, shape, k, s, p)


# ------------------------------------------------------------------------------------------------- inference
INFER_CASES = (0, 1, 2, 3, 4, 10)           # the small cases and (1, 25, 41, 2048)


@pytest.mark.parametrize("mi", range(len(R.MODES)), ids=["relu%d-res%d" % m for m in R.MODES])
@pytest.mark.parametrize("ci", INFER_CASES, ids=[_id(R.CASES[i]) for i in INFER_CASES])
def test_inference_vs_fp64(hip, ci, mi):
    """bn_fwd_test against the inference transform with the reference's double epsilon (bn_reference.bn_test64), inside
    bn_test_bound: the y bound at the running statistics plus the 4 u the float32 coefficient kernel costs"""
    relu, res = R.MODES[mi]
    c = _inputs(ci)
    d = _cuda(c)
    rs_h, rs_d = (c["res"], d["res"]) if res else (None, None)
    y = ops.bn_fwd_test(d["x"], d["gamma"], d["beta"], d["run_mean"], d["run_stdinv"], EPS, relu=relu, res=rs_d)
    ref = R.bn_test64(c["x"], c["gamma"], c["beta"], c["run_mean"], c["run_stdinv"], EPS, relu, rs_h)
    _hold("y", y, ref["y"], R.bn_test_bound(c["x"], c["gamma"], c["run_mean"], ref))


def test_inference_coefficient_cache(hip):
    """the layer's `cache` dict: the coefficients are computed once per weights version - a second call reuses them (even when the
    running statistics were changed behind its back: that is the contract, whoever changes them bumps the version), after
    bump_weights_version() the output follows the new statistics, and a fresh cache gives the bits of no cache"""
    c = _inputs(3)
    d = _cuda(c)
    args = (d["x"], d["gamma"], d["beta"])
    rm, rv = d["run_mean"].clone(), d["run_stdinv"].clone()
    plain = ops.bn_fwd_test(*args, rm, rv, EPS, relu=True)
    cache = {}
    first = ops.bn_fwd_test(*args, rm, rv, EPS, relu=True, cache=cache)
    coef, version = cache["test_coef"]
    assert torch.equal(first, plain) and version == ops.WEIGHTS_VERSION and coef.numel() == 2 * c["x"].shape[-1]
    again = ops.bn_fwd_test(*args, rm, rv, EPS, relu=True, cache=cache)
    assert torch.equal(again, plain) and cache["test_coef"][0] is coef
    rm2, rv2 = rm * 0.5 + 0.25, rv * 1.5
    stale = ops.bn_fwd_test(*args, rm2, rv2, EPS, relu=True, cache=cache)
    assert torch.equal(stale, plain) and cache["test_coef"][0] is coef         # reused: no version change was announced
    ops.bump_weights_version()
    fresh = ops.bn_fwd_test(*args, rm2, rv2, EPS, relu=True, cache=cache)
    assert cache["test_coef"][1] == ops.WEIGHTS_VERSION == version + 1
    ref = R.bn_test64(c["x"], c["gamma"], c["beta"], rm2.cpu(), rv2.cpu(), EPS, True)
    _hold("y after the bump", fresh, ref["y"], R.bn_test_bound(c["x"], c["gamma"], rm2.cpu(), ref))
    assert not torch.equal(fresh, plain)
    assert torch.equal(fresh, ops.bn_fwd_test(*args, rm2, rv2, EPS, relu=True))
    assert torch.equal(fresh, ops.bn_fwd_test(*args, rm2, rv2, EPS, relu=True, cache={}))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K,per_k", [(5, 27), (64, 256), (3, 1000), (160, 9 * 96)])
def test_bn_fold_vs_fp64(hip, K, per_k, bias):
    """bn_fold against bn_reference.bn_fold64: filters inside 4 u relative, the bias inside 4 u (|beta| + |mean - b| |s|)"""
    g = torch.Generator().manual_seed(K + per_k + bias)
    w = torch.randn(K, per_k, generator=g)
    cb = torch.randn(K, generator=g) if bias else None
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    rm, rv = torch.randn(K, generator=g), torch.rand(K, generator=g) + 0.5
    w_f, b_f = ops.bn_fold(w.cuda(), cb.cuda() if bias else None, gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), EPS)
    ref = R.bn_fold64(w, cb, gamma, beta, rm, rv, EPS)
    assert w_f.shape == w.shape and b_f.shape == (K,)
    _hold("filters", w_f, ref["w"], 4 * R.U * ref["w"].abs())
    _hold("bias", b_f, ref["b"], 4 * R.U * ref["b_scale"])
