"""Opt-in focal cost of the corner map and the detection head (focalGamma; csrc/focal.hip) on the GPU, against the float64 restatement
of DESIGN.md section 17 in tests/focal_reference.py, evaluated on the fp32 inputs the kernels read. The reference implementation has
no such mode, so the section and that file are the contract.

Tolerance (the form of test_corner_fwd_loss / test_detect_loss): gradients element-wise |err| <= 1e-4 * max|ref| + 1e-4 * |ref|,
costs relative 1e-4. An fp32 numpy evaluation of the same formulas lies about 2e-7 (max-norm) from float64 on such inputs, so the
bound leaves room for expf, powf and expm1f, while a missing or wrong gamma term moves the gradient by order gamma. Every test
prints its largest err / bound (pytest -s); the values are recorded in EXPERIMENTS.md."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focal_reference as FR
from denet_amd import ops
from denet_amd.model import audit, model_cnn, zoo

F32 = np.float32
GAMMAS = (1.0, 2.0, 3.5)
FOCAL_KERNELS = ("corner_focal_loss_kernel", "detect_focal_loss_kernel")


def _check(name, got, ref, cost=False):
    ratio = FR.cost_ratio(got, ref) if cost else FR.grad_ratio(got, ref)
    print("focal %s: largest err / bound = %.3g" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)


# ---- kernel level: the corner cost ----------------------------------------------------------------------------------------------

CORNER_SHAPES = [(3, 5, 7, 4, 128),           # 105 cells: one block, partly filled
                 (2, 16, 20, 5, 128)]         # 640 cells: 2.5 blocks; the five channels of DNC.C


def _corner_case(shape):
    """conv logits 3 * randn with 8 corner logits at +-30, targets rand / (H*W*Cn) with a quarter of the cells dropped (t0 = t1 = 0);
    -> device corner_pr (from corner_fwd) and target, host (l0, l1, t0, t1) in dconv's layout"""
    B, H, W, Cn, CP = shape
    rng = np.random.RandomState(10 + H)
    conv = (3.0 * rng.randn(B, H, W, CP)).astype(F32)
    for k, i in enumerate(rng.choice(B * H * W * Cn, 8, replace=False)):
        b, y, x, c = np.unravel_index(i, (B, H, W, Cn))
        conv[b, y, x, c] = 30.0 if k % 2 == 0 else -30.0
    tgt = (rng.rand(B, 2, Cn, H, W) / (H * W * Cn)).astype(F32)
    drop = rng.rand(B, Cn, H, W) < 0.25
    tgt[:, 0][drop] = 0.0
    tgt[:, 1][drop] = 0.0
    pr = ops.corner_fwd(torch.from_numpy(conv).cuda(), Cn)
    return pr, torch.from_numpy(tgt).cuda(), FR.corner_layout(pr.cpu().numpy(), tgt)


def _run_corner(pr, tgt, shape, gamma, fill=7.0, cost_factor=100.0):
    B, H, W, Cn, CP = shape
    dconv = torch.full((B, H, W, CP), fill).cuda()
    cost = torch.zeros(1).cuda()
    ops.corner_loss_focal(pr, tgt, dconv, cost, cost_factor, gamma)
    return float(cost.cpu()[0]), dconv.cpu().numpy()


@pytest.mark.parametrize("shape", CORNER_SHAPES)
def test_corner_kernel_against_float64(hip, shape):
    B, H, W, Cn, CP = shape
    pr, tgt, (l0, l1, t0, t1) = _corner_case(shape)
    assert (l0.min() < -50 or l1.min() < -50) and ((t0 == 0) & (t1 == 0)).mean() > 0.15
    for gamma in GAMMAS:
        cost_ref, grad_ref = FR.corner_focal(l0, l1, t0, t1, gamma, 100.0, B)
        cost, dconv = _run_corner(pr, tgt, shape, gamma)
        _check("corner %s gamma %g cost" % (shape[:4], gamma), cost, cost_ref, cost=True)
        _check("corner %s gamma %g gradient" % (shape[:4], gamma), dconv[..., :Cn], grad_ref)
        assert np.all(dconv[..., Cn:] == F32(7.0)), "channels beyond the corner logits were written"
        dropped = (t0 == 0) & (t1 == 0)
        assert np.all(dconv[..., :Cn][dropped] == 0.0)
        # the test-mode cost (no gradient array) is the same number
        only = torch.zeros(1).cuda()
        ops.corner_loss_focal(pr, tgt, None, only, 100.0, gamma)
        assert float(only.cpu()[0]) == cost


# ---- kernel level: the detection cost -------------------------------------------------------------------------------------------

DETECT_CASES = [(2, 3, 21, 32, False, 6), (2, 3, 21, 32, True, 0),          # (B, sn, ncls, CP, bounded IoU, nfit)
                (2, 3, 81, 96, False, 0), (2, 3, 81, 96, True, 6),
                (2, 3, 101, 128, False, 0), (2, 3, 101, 128, True, 0)]


def _detect_case(case):
    """the inputs of test_detect_loss at M = B * sn * sn = 18 RoIs: one-hot targets plus a second class on every fifth row,
    normalised; rows 0..3 have the target's logit raised by 30, rows 4..7 another class's"""
    B, sn, ncls, CP, bounded, nfit = case
    S = sn * sn
    M = B * S
    rng = np.random.RandomState(12 + ncls)
    logits = rng.randn(M, CP).astype(F32)
    t = np.zeros((M, ncls), F32)
    cls = rng.randint(0, ncls, M)
    t[np.arange(M), cls] = 1.0
    t[::5, 3] = 1.0
    t = (t / t.sum(1, keepdims=True) / S).astype(F32)
    for r in range(4):
        logits[r, cls[r]] += 30.0
        logits[4 + r, (cls[4 + r] + 1) % ncls] += 30.0
    valid = ((rng.rand(M) > 0.5) / S).astype(F32)

    def boxes():
        bx = rng.rand(M, 4).astype(F32)
        bx[:, 2:] = bx[:, :2] + 0.05 + bx[:, 2:] * 0.5
        return bx

    def cxcywh(bx):
        return np.stack([0.5 * (bx[:, 0] + bx[:, 2]), 0.5 * (bx[:, 1] + bx[:, 3]), bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], 1)

    roi, tb = boxes(), boxes()
    bt = np.concatenate([cxcywh(tb), cxcywh(roi)], 1).astype(F32)
    fit = None
    if nfit:
        fit = np.zeros((M, nfit), F32)
        fit[np.arange(M), rng.randint(0, nfit, M)] = 1.0 / S
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return {"logits": dev(logits), "t": dev(t), "valid": dev(valid), "bt": dev(bt), "roi": dev(roi), "fit": dev(fit),
            "host": (logits, t)}


def _run_detect(c, case, gamma, cost_factor=1.5, bbox_factor=2.0, fit_factor=0.5, fill=5.0):
    """gamma None: the plain entry point"""
    B, sn, ncls, CP, bounded, nfit = case
    dl = torch.full((B * sn * sn, CP), fill).cuda()
    costs = torch.zeros(2).cuda()
    if gamma is None:
        ops.detect_loss(c["logits"], c["t"], c["valid"], c["bt"], c["roi"], dl, costs, B, ncls, 4, cost_factor, bbox_factor, bounded,
                        fit_target=c["fit"], nfit=nfit, fit_factor=fit_factor)
    else:
        ops.detect_loss_focal(c["logits"], c["t"], c["valid"], c["bt"], c["roi"], dl, costs, B, ncls, 4, cost_factor, bbox_factor, gamma,
                              bounded, fit_target=c["fit"], nfit=nfit, fit_factor=fit_factor)
    return costs.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("case", DETECT_CASES)
def test_detect_kernel_against_float64(hip, case):
    B, sn, ncls, CP, bounded, nfit = case
    c = _detect_case(case)
    logits, t = c["host"]
    plain_costs, plain_dl = _run_detect(c, case, None)
    assert plain_costs[1] != 0 and np.all(plain_dl[:, ncls + 4 + nfit:] == 0)
    for gamma in GAMMAS:
        cost_ref, grad_ref = FR.detect_focal(logits[:, :ncls], t, gamma, 1.5, B)
        costs, dl = _run_detect(c, case, gamma)
        name = "detect ncls %d%s%s gamma %g" % (ncls, " bounded" if bounded else "", " nfit %d" % nfit if nfit else "", gamma)
        _check(name + " cost", costs[0], cost_ref, cost=True)
        _check(name + " gradient", dl[:, :ncls], grad_ref)
        # everything but the class part is the plain kernel's, bit for bit
        assert costs[1].tobytes() == plain_costs[1].tobytes()
        assert dl[:, ncls:].tobytes() == plain_dl[:, ncls:].tobytes()
    # the test-mode cost (no gradient array)
    only = torch.zeros(2).cuda()
    ops.detect_loss_focal(c["logits"], c["t"], c["valid"], c["bt"], c["roi"], None, only, B, ncls, 4, 1.5, 2.0, GAMMAS[-1], bounded,
                          fit_target=c["fit"], nfit=nfit, fit_factor=0.5)
    assert only.cpu().numpy().tobytes() == costs.tobytes()


# ---- gamma = 0 called directly, reproducibility ---------------------------------------------------------------------------------

def test_gamma_0_entry_points_agree_with_the_plain_ones(hip):
    """bit equality is not required (the summation is theirs); the reference here is the plain kernel's output"""
    shape = CORNER_SHAPES[1]
    B, H, W, Cn, CP = shape
    pr, tgt, _ = _corner_case(shape)
    cost, dconv = _run_corner(pr, tgt, shape, 0.0)
    pd = torch.full((B, H, W, CP), 7.0).cuda()
    pc = torch.zeros(1).cuda()
    ops.corner_loss(pr, tgt, pd, pc, 100.0)
    _check("corner gamma 0 against corner_loss, cost", cost, float(pc.cpu()[0]), cost=True)
    _check("corner gamma 0 against corner_loss, gradient", dconv[..., :Cn], pd.cpu().numpy()[..., :Cn])
    for case in (DETECT_CASES[0], DETECT_CASES[3]):
        c = _detect_case(case)
        ncls = case[2]
        pcosts, pdl = _run_detect(c, case, None)
        costs, dl = _run_detect(c, case, 0.0)
        _check("detect ncls %d gamma 0 against detect_loss, cost" % ncls, costs[0], pcosts[0], cost=True)
        _check("detect ncls %d gamma 0 against detect_loss, gradient" % ncls, dl[:, :ncls], pdl[:, :ncls])
        assert costs[1].tobytes() == pcosts[1].tobytes() and dl[:, ncls:].tobytes() == pdl[:, ncls:].tobytes()


def test_two_runs_give_the_same_bits(hip):
    shape = CORNER_SHAPES[1]
    pr, tgt, _ = _corner_case(shape)
    a, b = _run_corner(pr, tgt, shape, 3.5), _run_corner(pr, tgt, shape, 3.5)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    case = DETECT_CASES[3]
    c = _detect_case(case)
    a, b = _run_detect(c, case, 3.5), _run_detect(c, case, 3.5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- layer level ----------------------------------------------------------------------------------------------------------------

B_, IMG = 2, 128
FOCAL_DESC = zoo.DENET34_SKIP_DESC.replace("DNC[96,100]", "DNC[96,100,0,2]").replace("DND[0.5,1,1]", "DND[0.5,1,1,0,2]")
assert FOCAL_DESC.count(",2]") == 2


def _model(focal=True, seed=1):
    model = zoo.denet34(B_, "skip", IMG, class_num=80, seed=seed, head_desc=FOCAL_DESC if focal else zoo.DENET34_SKIP_DESC)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    return model, by_type("denet-corner"), by_type("denet-sparse"), by_type("denet-detect")


class _Calls:
    """counts the calls of the four cost wrappers and keeps the tensors of the focal ones (references, no copies: no launch is
    added to the step)"""

    def __init__(self, monkeypatch):
        self.n = {}
        self.args = {}
        for name in ("corner_loss", "detect_loss", "corner_loss_focal", "detect_loss_focal"):
            self.n[name] = 0
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.n[name] += 1
            self.args[name] = (a, k)
            return fn(*a, **k)
        return call


def test_layer_step_runs_the_focal_kernels(hip, monkeypatch):
    """one training step of DeNet-34 skip (B = 2, 128 x 128) with gamma 2 on both cost layers: the kernels the step ran, and the
    gradients and logged costs against the float64 helper on the layers' own corner_pr, targets and logits"""
    calls = _Calls(monkeypatch)
    model, dnc, dns, dnd = _model()
    assert dnc.focal_gamma == 2.0 and dnd.focal_gamma == 2.0
    zoo.warm_corner_head(model, bias=7.5)          # corner probabilities that vary from cell to cell, and detector RoIs
    model.build_train_func("nesterov")
    assert all(f == 1.0 for f in model.cost_factors)
    random.seed(9)
    x, metas = zoo.synthetic_batch(B_, IMG, seed=3)
    with audit.KernelAudit(model) as ka:
        cost, layer_costs = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
        dns.sample_bbox_list
    torch.cuda.synchronize()
    for k in FOCAL_KERNELS:
        assert ka.other.count(k) == 1, ka.other
    assert not [s for s in ka.other if "corner_loss_kernel" in s or "detect_loss_kernel" in s]
    assert calls.n == {"corner_loss": 0, "detect_loss": 0, "corner_loss_focal": 1, "detect_loss_focal": 1}
    assert np.isfinite(cost) and all(np.isfinite(layer_costs))
    terms = model.last_cost_terms
    # corner layer
    Cn = dnc.corner_num
    (pr, tgt, dconv, _, cost_factor, gamma), _ = calls.args["corner_loss_focal"]
    assert pr is dnc.corner_pr and tgt is dnc._target and dconv is dnc.dconv and gamma == 2.0
    l0, l1, t0, t1 = FR.corner_layout(pr.cpu().numpy(), tgt.cpu().numpy())
    cost_ref, grad_ref = FR.corner_focal(l0, l1, t0, t1, 2.0, float(dnc.cost_factor), B_)
    # (the RoI gather's gradient has filled the sampling channels of the same array since: the corner channels are the cost's)
    _check("layer corner gradient", dconv.cpu().numpy()[..., :Cn], grad_ref)
    _check("layer corner cost", terms[model.cost_layers.index(dnc), 0], cost_ref, cost=True)
    # (the comparison tells the two costs apart: the plain gradient of the same inputs is far outside the bound)
    assert FR.grad_ratio(dconv.cpu().numpy()[..., :Cn], FR.corner_plain(l0, l1, t0, t1, float(dnc.cost_factor), B_)[1]) > 10
    # detection layer
    a = calls.args["detect_loss_focal"][0]
    lg, t, dl = a[0], a[1], a[5]
    assert lg.data_ptr() == dnd.conv.output.data.data_ptr() and t is dnd._targets["det"] and a[12] == 2.0
    assert dl.data_ptr() == dnd.conv.output.grad.data_ptr()
    z = lg.cpu().numpy()[:, :dnd.s0]
    cost_ref, grad_ref = FR.detect_focal(z, t.cpu().numpy(), 2.0, float(dnd.cost_factor), B_)
    grad = dl.cpu().numpy()
    _check("layer detect gradient", grad[:, :dnd.s0], grad_ref)
    _check("layer detect cost", terms[model.cost_layers.index(dnd), 0], cost_ref, cost=True)
    assert FR.grad_ratio(grad[:, :dnd.s0], FR.detect_plain(z, t.cpu().numpy(), float(dnd.cost_factor), B_)[1]) > 10
    assert not grad[:, dnd.s0 + dnd.s1 + dnd.s2:].any()
    # the test-mode cost (want_grad=False) is the same definition: the same numbers from the same state
    buf = torch.zeros(4).cuda()
    dnc.loss_backward(None, buf[0:2], want_grad=False)
    dnd.loss_backward(None, buf[2:4], want_grad=False)
    got = buf.cpu().numpy()
    assert got[0] == terms[model.cost_layers.index(dnc), 0] and got[2] == terms[model.cost_layers.index(dnd), 0]
    assert calls.n["corner_loss"] == 0 and calls.n["detect_loss"] == 0


_ALONE = {}


def _train(focal, steps=2, seed=1, lr=0.05):
    from tests.test_cluster_device_gpu import _params_of
    model, dnc, dns, _ = _model(focal, seed)
    model.build_train_func("nesterov")
    random.seed(9)
    costs, launches = [], []
    for it in range(steps):
        x, metas = zoo.synthetic_batch(B_, IMG, seed=3 + it)
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, it, lr, [0.9], 1e-4)
            dns.sample_bbox_list
        costs.append(cost)
        launches.append([s for s in ka.other if s in FOCAL_KERNELS])
    torch.cuda.synchronize()
    return costs, launches, _params_of(model)


def _train_alone(focal):
    """two steps of a model that has the process to itself while it steps; computed once"""
    if focal not in _ALONE:
        _ALONE[focal] = _train(focal)
    return _ALONE[focal]


def test_mode_off_is_untouched(hip, monkeypatch):
    """a default model steps, a focal model is built and takes two steps in the same process, the default model steps again: costs and
    parameters equal those of a default model that took the two steps on its own, bit for bit; its audits hold no focal kernel and
    its layers never call the focal wrappers. (The generators' states are put back after the focal step: its RoI editing draws from
    them.)"""
    from tests.test_cluster_device_gpu import _params_of
    alone_costs, alone_launches, alone_w = _train_alone(False)
    calls = _Calls(monkeypatch)
    model, dnc, dns, dnd = _model(False)
    assert dnc.focal_gamma == 0.0 and dnd.focal_gamma == 0.0
    model.build_train_func("nesterov")
    random.seed(9)
    costs, launches = [], []
    for it in range(2):
        x, metas = zoo.synthetic_batch(B_, IMG, seed=3 + it)
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, it, 0.05, [0.9], 1e-4)
            dns.sample_bbox_list
        costs.append(cost)
        launches.append([s for s in ka.other if s in FOCAL_KERNELS])
        assert calls.n["corner_loss_focal"] == (0 if it == 0 else 2) and calls.n["detect_loss_focal"] == (0 if it == 0 else 2)
        if it == 0:
            torch.cuda.synchronize()
            saved = (random.getstate(), np.random.get_state())
            fcosts, flaunches, fw = _train(True)
            random.setstate(saved[0])
            np.random.set_state(saved[1])
    torch.cuda.synchronize()
    assert calls.n["corner_loss"] == 2 and calls.n["detect_loss"] == 2
    assert launches == [[], []] and alone_launches == [[], []]
    assert costs == alone_costs, (costs, alone_costs)
    w = _params_of(model)
    assert len(w) == len(alone_w) > 0 and all(np.array_equal(a, b) for a, b in zip(w, alone_w))
    # the mode does something: the focal model's parameters after the same two steps are not the default's
    assert all(sorted(l) == sorted(FOCAL_KERNELS) for l in flaunches) and all(np.isfinite(fcosts))
    assert fcosts[0] < alone_costs[0]                 # not renormalised: the focal cost is the smaller one at the same costFactor
    assert any(not np.array_equal(a, b) for a, b in zip(fw, alone_w))


def test_model_file_and_inference(hip, tmp_path):
    """a focal model keeps both gammas through .mdl.gz; inference does not read them: get_detections gives the same detections on
    the same weights with focal_gamma cleared"""
    model, _, _, _ = _model()
    zoo.warm_corner_head(model, bias=7.5)
    fname = str(tmp_path / "focal.mdl.gz")
    model_cnn.save_to_file(model, fname)
    loaded = model_cnn.load_from_file(fname, B_)
    by_type = lambda m, t: [l for l in m.layers if l.type_name == t][0]
    dnc, dnd = by_type(loaded, "denet-corner"), by_type(loaded, "denet-detect")
    assert dnc.focal_gamma == 2.0 and dnd.focal_gamma == 2.0
    assert dnc.export_json()["focalGamma"] == 2.0 and dnd.export_json()["focalGamma"] == 2.0
    x, _ = zoo.synthetic_batch(B_, IMG, seed=11)
    params = {"cornerThreshold": 0.01, "prThreshold": 0.01, "nmsThreshold": 0.5}
    res = dnd.get_detections(loaded, x, None, params)
    assert len(res) == B_ and sum(len(r["detections"]) for r in res) > 0, "the warmed detector detected nothing"
    dnc.focal_gamma = dnd.focal_gamma = 0.0           # (model-modify's way of clearing it, without its reload: the same weights)
    assert "focalGamma" not in dnc.export_json() and "focalGamma" not in dnd.export_json()
    res0 = dnd.get_detections(loaded, x, None, params)
    assert [r["detections"] for r in res0] == [r["detections"] for r in res]
