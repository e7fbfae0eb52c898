"""Global-norm gradient clipping and on-device gradient norms on the GPU (csrc/grad_norm.hip): the reduction
kernel against numpy float64, the coefficient-reading solvers against the plain ones (bit for bit at coef = 1) and against the
float64 formula, a whole clipped step of a small padded stack against the float64 restatement of tests/fp64_model.py, "off means
off" in the kernel audit and in the bits, the accumulated and the adam update, and the device's running record."""
import math

import numpy as np
import pytest
import torch

from denet_amd import ops
from denet_amd.model import audit
from fp64_model import build_model, param_layers, reference, rel as _rel
from test_grad_clip_host import GAP, LENGTHS, RANGES, TOTAL, coef64, laid_out

pytestmark = pytest.mark.gpu

NEW_SYMBOLS = ops.NORM_KERNELS + ops.COEF_SOLVER_KERNELS


# ------------------------------------------------------------------------------------------------- 1. the kernel against float64
def _buffer():
    """the five ranges, each drawn at a scale of its own (1e-3 .. 1e3: a chunk credited to the wrong segment shows), NaN in front
    of, between and behind them: one read outside the table poisons the result"""
    rng = np.random.RandomState(5)
    host = np.full(TOTAL, np.nan, dtype=np.float32)
    scales = np.logspace(-3, 3, len(RANGES))
    for (off, n), s in zip(RANGES, scales):
        host[off:off + n] = (rng.normal(size=n) * s).astype(np.float32)
    seg = np.array([np.sqrt((host[off:off + n].astype(np.float64) ** 2).sum()) for off, n in RANGES])
    total = np.sqrt(sum((host[off:off + n].astype(np.float64) ** 2).sum() for off, n in RANGES))
    return host, seg, total


def _poisoned(nt):
    nt.workspace.fill_(255)                              # NaN as doubles, -1 as indices
    return torch.full((nt.n_segments,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")


def test_kernel_vs_float64(hip):
    host, seg_ref, total_ref = _buffer()
    assert RANGES[0][0] == GAP and TOTAL == sum(LENGTHS) + GAP * (len(LENGTHS) + 1)
    x = torch.from_numpy(host).cuda()
    nt = ops.NormTable(RANGES, TOTAL)
    assert nt.n_chunks == 11 and nt.n_segments == 5 and nt.bytes_read == 4 * sum(LENGTHS)
    seg, out = _poisoned(nt)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    ops.grad_norm(x, nt, 1.0, 0.0, seg_norm=seg, out=out, stats=stats)
    seg_a, out_a = seg.cpu().numpy().copy(), out.cpu().numpy().copy()
    e_seg = float(np.max(np.abs(seg_a.astype(np.float64) - seg_ref) / seg_ref))
    e_tot = abs(float(out_a[0]) - total_ref) / total_ref
    print("segment norms %.2e, total %.2e (device %r, float64 %r)" % (e_seg, e_tot, float(out_a[0]), total_ref))
    # double accumulation of at most 2^25 exact products errs below 1e-8, the final float rounding by 6e-8
    assert e_seg <= 1e-6 and e_tot <= 1e-6
    assert out_a[1] == 1.0                                # clip <= 0: norms only
    # twice: identical bits, from a poisoned workspace again
    seg2, out2 = _poisoned(nt)
    ops.grad_norm(x, nt, 1.0, 0.0, seg_norm=seg2, out=out2, stats=stats)
    assert seg2.cpu().numpy().tobytes() == seg_a.tobytes() and out2.cpu().numpy().tobytes() == out_a.tobytes()
    st = stats.cpu().numpy()
    assert st[0] == 2 and st[1] == 0 and st[2] == 0 and st[3] == 2 * np.float64(out_a[0]) and st[4] == np.float64(out_a[0])
    # the host scale (1 / world size, 1 / accumulated steps)
    ops.grad_norm(x, nt, 0.25, 0.0, seg_norm=seg2, out=out2)
    assert float(np.max(np.abs(seg2.cpu().numpy().astype(np.float64) - 0.25 * seg_ref) / (0.25 * seg_ref))) <= 1e-6
    assert abs(float(out2[0]) - 0.25 * total_ref) <= 1e-6 * 0.25 * total_ref
    # the limit below / above the norm
    for c in (0.5 * total_ref, 0.001 * total_ref):
        c = float(np.float32(c))
        ops.grad_norm(x, nt, 1.0, c, seg_norm=seg2, out=out2)
        norm, coef = out2.cpu().numpy()
        want = coef64(total_ref, c)
        print("clip %g: coef %r (float64 %r)" % (c, float(coef), float(want)))
        assert norm == out_a[0] and abs(float(coef) - float(want)) <= 2 * float(np.spacing(np.float32(want)))
    for c in (float(np.float32(2.0 * total_ref)), 1e30):
        ops.grad_norm(x, nt, 1.0, c, seg_norm=seg2, out=out2)
        assert float(out2[1]) == 1.0


def test_kernel_many_chunks_and_segments(hip):
    """the finishing workgroup's other paths: more segments than it has threads (256), more chunks than one round of its LDS
    staging holds (2048), and a 20-chunk segment that lies across the boundary between two rounds"""
    lengths = [64] * 2040 + [20 * ops.NORM_CHUNK] + [64, 128] * 50
    ranges, total = laid_out(lengths)
    rng = np.random.RandomState(9)
    host = np.full(total, np.nan, dtype=np.float32)
    for k, (off, n) in enumerate(ranges):
        host[off:off + n] = (rng.normal(size=n) * (1.0 + k % 7)).astype(np.float32)
    sums = np.array([(host[off:off + n].astype(np.float64) ** 2).sum() for off, n in ranges])
    nt = ops.NormTable(ranges, total)
    assert nt.n_segments == 2141 and nt.n_chunks == 2160 and nt.first[2040] == 2040 and nt.first[2041] == 2060
    seg, out = _poisoned(nt)
    ops.grad_norm(torch.from_numpy(host).cuda(), nt, 1.0, 0.0, seg_norm=seg, out=out)
    e_seg = float(np.max(np.abs(seg.cpu().numpy().astype(np.float64) - np.sqrt(sums)) / np.sqrt(sums)))
    e_tot = abs(float(out[0]) - math.sqrt(sums.sum())) / math.sqrt(sums.sum())
    print("2141 segments, 2160 chunks: segment norms %.2e, total %.2e" % (e_seg, e_tot))
    assert e_seg <= 1e-6 and e_tot <= 1e-6


def test_kernel_nonfinite_norms(hip):
    """norm = NaN gives coef = 1, norm = inf gives coef = 0: a non-finite gradient is not rescued; the record counts such steps"""
    ranges, total = [(0, 64), (64, 128)], 192
    nt = ops.NormTable(ranges, total)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    x = torch.ones(total, device="cuda")
    ops.grad_norm(x, nt, 1.0, 1.0, stats=stats)
    norm, coef = nt.out.cpu().tolist()
    assert abs(norm - math.sqrt(192.0)) <= 1e-6 * norm and abs(coef - 1.0 / math.sqrt(192.0)) <= 1e-7
    x[70] = float("nan")
    ops.grad_norm(x, nt, 1.0, 1.0, stats=stats)
    norm, coef = nt.out.cpu().tolist()
    seg = nt.seg_norm.cpu().tolist()
    assert math.isnan(norm) and coef == 1.0 and seg[0] == 8.0 and math.isnan(seg[1])
    x[70] = float("inf")
    ops.grad_norm(x, nt, 1.0, 1.0, stats=stats)
    norm, coef = nt.out.cpu().tolist()
    assert math.isinf(norm) and coef == 0.0
    st = stats.cpu().tolist()
    assert st[0] == 3 and st[1] == 2 and st[2] == 2 and st[4] == np.float32(math.sqrt(192.0))


# ------------------------------------------------------------------------------------------------- 2. the solver entries
N, N_DECAY = 4096 + 64, 4096
LR, MU, DECAY, GSCALE = 0.05, 0.9, 5e-4, 1.0 / 3.0
B1, B2 = 0.9, 0.999


def _solver_arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, generator=g).cuda() for _ in range(3)] + [torch.rand(N, generator=g).cuda()]      # p, m, grad, v >= 0


@pytest.mark.parametrize("it", [0, 3])
@pytest.mark.parametrize("solver", ["sgd", "nesterov", "adam"])
def test_solver_coef_one_is_the_plain_solver(hip, solver, it):
    """coef = 1: parameters and momentum bit for bit those of the plain entries, with a gradient scale that is no power of two
    (a compiler that contracted the coefficient's product into the decay FMA would change the last bit)"""
    p, m, grad, v = _solver_arrays(7 + it)
    one = torch.ones(1, device="cuda")
    got, want = [], []
    for coef, dst in ((None, want), (one, got)):
        pc, mc, vc = p.clone(), m.clone(), v.clone()
        if solver == "adam":
            ops.solver_adam(pc, mc, vc, grad, N_DECAY, LR, B1, B2, it, DECAY, GSCALE, coef=coef)
        else:
            ops.solver_step(pc, mc, grad, N_DECAY, LR, MU, it, DECAY, {"sgd": 0, "nesterov": 1}[solver], GSCALE, coef=coef)
        dst += [pc, mc, vc]
    assert not torch.equal(want[0], p)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("solver", ["sgd", "nesterov", "adam"])
def test_solver_coef_vs_float64(hip, solver):
    it, cf = 3, 0.37
    p, m, grad, v = _solver_arrays(19)
    coef = torch.tensor([cf], device="cuda")
    cf = float(coef.cpu()[0])
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    p64, m64, g64, v64 = (t.double().cpu() for t in (p, m, grad, v))
    gv = g64 * float(np.float32(GSCALE)) * cf
    gv[:N_DECAY] += float(np.float32(DECAY)) * p64[:N_DECAY]
    lr, mu = float(np.float32(LR)), float(np.float32(MU))
    if solver == "adam":
        ops.solver_adam(pc, mc, vc, grad, N_DECAY, LR, B1, B2, it, DECAY, GSCALE, coef=coef)
        b1, b2 = float(np.float32(B1)), float(np.float32(B2))
        m_ref = b1 * m64 + (1 - b1) * gv
        v_ref = b2 * v64 + (1 - b2) * gv * gv
        c1, c2 = 1.0 / (1.0 - b1 ** (it + 1)), 1.0 / (1.0 - b2 ** (it + 1))
        upd = -lr * (m_ref * c1) / (torch.sqrt(v_ref * c2) + 1e-8)
        assert _rel(vc, v_ref) <= 1e-5
    elif solver == "nesterov":
        ops.solver_step(pc, mc, grad, N_DECAY, LR, MU, it, DECAY, 1, GSCALE, coef=coef)
        m_ref = mu * m64 + gv
        upd = -lr * (gv + mu * m_ref)
    else:
        ops.solver_step(pc, mc, grad, N_DECAY, LR, MU, it, DECAY, 0, GSCALE, coef=coef)
        m_ref = mu * m64 + (1 - mu) * gv
        upd = -lr * m_ref
    e_u, e_m = _rel(pc.double().cpu() - p64, upd), _rel(mc, m_ref)
    print("%s: update %.2e, momentum %.2e" % (solver, e_u, e_m))
    assert e_u <= 1e-5 and e_m <= 1e-5              # a handful of fp32 roundings


# ------------------------------------------------------------------------------------------------- 3. a whole step against float64
DESC = "C[32,3] BN A P[2] C[20,3] A R"
B, CLS = 4, 10
STEP_LR, STEP_MOM, STEP_DECAY = 0.1, 0.9, 0.0005


def _model(seed=5):
    return build_model(DESC, (3, 32, 32), B, CLS, seed=seed)


def _batch(seed=11):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    return x, cls, [{"image_class": int(c)} for c in cls]


def _flat(model):
    return [p for _, ps in param_layers(model) for p in ps]


def _direct():
    return ops.algorithms(table={}, POLICY=ops.direct_policy)


@pytest.fixture(autouse=True)
def _direct_kernels():
    """every step of this file on the direct kernels: nothing is measured, twins of one seed run the same launches"""
    with _direct():
        yield


@pytest.fixture(scope="module")
def tracked_step(hip):
    """one tracked (unclipped) sgd step of the stack and its float64 restatement (the `BN A P` front runs fused and keeps no
    activation to take the device's ReLU decisions from: float64 makes its own): computed once, read by the tests below. The stack pads channels at the input (3 -> 4), in the middle (20 -> 32) and at the head (10 -> 32)"""
    with _direct():
        model = _model()
        model.track_grad_norm = True
        model.build_train_func("sgd")
        x, cls, metas = _batch()
        before = param_layers(model)
        assert sorted(id(p) for p in _flat(model)) == sorted(id(p) for p in model.trained_params)
        values = {id(l): [p.get_value().copy() for p in ps] for l, ps in before}
        model.train_step(x, metas, 0, 0, STEP_LR, [STEP_MOM], STEP_DECAY)
        torch.cuda.synchronize()
        params = {k: [torch.from_numpy(v).double().requires_grad_(True) for v in vs] for k, vs in values.items()}
        cost_ref, _, _ = reference(model, x, params, cls, True)
        cost_ref.backward()
    g_ref = [t.grad for l, ps in before for t in params[id(l)]]
    p_ref = [torch.from_numpy(v).double() for l, ps in before for v in values[id(l)]]
    norm_ref = math.sqrt(sum(float((g * g).sum()) for g in g_ref))
    return {"model": model, "g_ref": g_ref, "p_ref": p_ref, "norm_ref": norm_ref}


def test_padding_contributes_nothing(hip, tracked_step):
    """the device reduces every array's 64-aligned extent of the padded layout; the logical entries alone (Param.get_grad) give
    the same norms in float64: padded channels, unreal taps and alignment gaps are zero in the gradient buffer"""
    model = tracked_step["model"]
    dev = model._norm.seg_norm.cpu().numpy().astype(np.float64)
    padded = 0
    for p, d in zip(model.trained_params, dev):
        g = p.get_grad().astype(np.float64)
        want = math.sqrt(float((g * g).sum()))
        padded += int(p.dev_size > g.size or p.dev_size % 64 != 0)
        assert want > 0 and abs(d - want) <= 1e-6 * want, (p.name, d, want)
    assert padded >= 3
    rows = model.param_norms()
    assert len(rows) == len(dev) and [r[3] for r in rows] == [float(np.float32(d)) for d in dev]
    for (li, tname, pname, _, wn), p in zip(rows, model.trained_params):
        w = p.get_value().astype(np.float64)
        assert pname == p.name and li > 0 and tname in ("conv", "batchnorm")
        assert abs(wn - math.sqrt(float((w * w).sum()))) <= 1e-6 * max(wn, 1e-30)
    assert _rel(np.array([model.last_grad_norm()[0]]), np.array([tracked_step["norm_ref"]])) <= 1e-3
    assert model.last_grad_norm()[1] == 1.0


def test_clipped_step_vs_float64(hip, tracked_step):
    """gradient_clip = norm_ref / 2: clipping bites by a known factor. Norm, coefficient and every array's update against
    -lr * (0.5 * g_ref + decay * p) within the project's 1e-3 budget"""
    norm_ref = tracked_step["norm_ref"]
    with _direct():
        model = _model()
        model.gradient_clip = norm_ref / 2
        model.build_train_func("sgd")
        x, cls, metas = _batch()
        flat = _flat(model)
        weights = set(id(p) for l in model.layers for p in l.weights())
        for p, v in zip(flat, tracked_step["p_ref"]):
            assert np.array_equal(p.get_value().astype(np.float64), v.numpy())      # the identically seeded twin
        model.train_step(x, metas, 0, 0, STEP_LR, [STEP_MOM], STEP_DECAY)
        torch.cuda.synchronize()
    norm, coef = model.last_grad_norm()
    print("norm %r (float64 %r), coef %r" % (norm, norm_ref, coef))
    assert abs(norm - norm_ref) <= 1e-3 * norm_ref and abs(coef - 0.5) <= 1e-3 * 0.5
    worst = 0.0
    for p, v, g in zip(flat, tracked_step["p_ref"], tracked_step["g_ref"]):
        assert float(g.abs().max()) > 0, p.name
        upd_ref = -STEP_LR * (0.5 * g + (STEP_DECAY if id(p) in weights else 0.0) * v)
        upd = torch.from_numpy(p.get_value().copy()).double() - v
        e = _rel(upd, upd_ref)
        worst = max(worst, e)
        assert e <= 1e-3, (p.name, e)
    print("worst update %.2e over %d arrays" % (worst, len(flat)))
    st = model.grad_norm_stats(reset=False)
    assert st["steps"] == 1 and st["clipped"] == 1 and st["nonfinite"] == 0 and st["limit"] == norm_ref / 2


# ------------------------------------------------------------------------------------------------- 4. off means off
def _two_steps(model, solver="nesterov"):
    model.build_train_func(solver)
    syms = []
    for it, seed in ((0, 11), (1, 12)):
        x, cls, metas = _batch(seed)
        with audit.KernelAudit(model) as ka:
            model.train_step(x, metas, 0, it, STEP_LR, [STEP_MOM], STEP_DECAY)
        syms += [s for r in ka.table for s in r["fwd"] + r["bwd"]] + list(ka.other)
    torch.cuda.synchronize()
    return syms, [t.clone() for t in (model.P, model.M, model.S)]


def test_off_means_off(hip):
    """a plain model's step launches none of the new kernels; a limit the norm never reaches and tracking alone leave parameters,
    momentum and running statistics bit for bit the plain model's after two steps"""
    plain_syms, plain = _two_steps(_model())
    assert plain_syms and not [s for s in plain_syms if s in NEW_SYMBOLS]
    far = _model()
    far.gradient_clip = 1e30
    far_syms, far_state = _two_steps(far)
    assert [s for s in far_syms if s in NEW_SYMBOLS] == ["grad_norm_partial_kernel", "grad_norm_finish_kernel", "solver_coef_kernel"] * 2
    assert [s for s in far_syms if s not in NEW_SYMBOLS] == plain_syms
    tracked = _model()
    tracked.track_grad_norm = True
    tr_syms, tr_state = _two_steps(tracked)
    assert [s for s in tr_syms if s in NEW_SYMBOLS] == ["grad_norm_partial_kernel", "grad_norm_finish_kernel"] * 2      # the plain solver
    for state in (far_state, tr_state):
        for a, b in zip(state, plain):
            assert a.numel() == b.numel() and torch.equal(a, b)
    assert not torch.equal(plain[1], torch.zeros_like(plain[1]))
    assert far.last_grad_norm() == tracked.last_grad_norm() and far.last_grad_norm()[1] == 1.0
    assert far.grad_norm_stats()["clipped"] == 0


# ------------------------------------------------------------------------------------------------- 5. acc mode and adam
def _norm64(G, n, scale):
    g = G[:n].astype(np.float64) * scale
    return math.sqrt(float((g * g).sum()))


def test_acc_mode_clips_the_mean_gradient(hip):
    """train_begin, two steps, train_end with a limit at half the mean accumulated gradient's norm: the one update against the
    float64 formula from host copies of the accumulator and the parameters"""
    model = _model()
    model.build_train_func("nesterov", use_acc_mode=True)
    model.train_begin()
    for it, seed in ((0, 11), (1, 12)):
        x, cls, metas = _batch(seed)
        model.train_step(x, metas, 0, it, STEP_LR, [STEP_MOM], STEP_DECAY)
    torch.cuda.synchronize()
    n, nd = model.n_trainable, model.n_weights
    G = model._acc["G"].cpu().numpy().copy()
    P0 = model.P.cpu().numpy().astype(np.float64)[:n]
    assert not model.M.any()
    norm = _norm64(G, n, 0.5)
    model.gradient_clip = norm / 2
    model.train_end()
    got_norm, got_coef = model.last_grad_norm()
    assert abs(got_norm - norm) <= 1e-6 * norm and abs(got_coef - 0.5) <= 1e-6
    gv = G[:n].astype(np.float64) * 0.5 * coef64(norm, np.float32(norm / 2))
    gv[:nd] += float(np.float32(STEP_DECAY)) * P0[:nd]
    mu, lr = float(np.float32(STEP_MOM)), float(np.float32(STEP_LR))
    upd_ref = -lr * (gv + mu * gv)                    # nesterov at iteration 1 from zero momentum: m' = gv
    upd = model.P.cpu().numpy().astype(np.float64)[:n] - P0
    e = _rel(upd, upd_ref)
    print("acc-mode update %.2e" % e)
    assert e <= 1e-5
    assert model.grad_norm_stats()["steps"] == 1      # the two sub-steps ran no norm pass


def test_adam_step_is_clipped(hip, tracked_step, monkeypatch):
    """one adam step at half the gradient's norm, against the float64 formula from the gradient captured in front of the solver.
    The step runs WITHOUT L2 decay, for a reason of adam's, not of clipping: with decay some entries have coef * g cancel
    decay * p down to |gv| ~ 1e-8, adam's eps, where the update lr * gv / (|gv| + eps) turns a rounding of 6e-8 * |coef * g| into
    up to lr * 6e-8 * |coef * g| / eps, i.e. 1e-4 of the largest update at |coef * g| ~ 2e-5 (measured on this stack: 4.8e-6 and
    2.7e-5 at two limits, worst entries gv = 3.9e-8 and 2.6e-8). Without decay gv = coef * g carries two roundings and the
    sensitivity eps / (|gv| + eps) is at most 1: what is left is the rounding of p' itself, half an ulp of p' (|p| <= 1: a batch norm's
    gamma; 6e-8 at most) against updates of lr = 0.01, 6e-6 (measured 1.6e-6). The decay region of adam_coef_kernel is checked by test_solver_coef_vs_float64"""
    model = _model()
    model.gradient_clip = tracked_step["norm_ref"] / 2
    model.build_train_func("adam")
    seen = {}
    adam0 = ops.solver_adam

    def capture(p, m, v, g, *a, **k):
        torch.cuda.synchronize()
        seen.update(P=p.cpu().numpy().astype(np.float64), G=g.cpu().numpy().copy(), coef=k.get("coef"))
        return adam0(p, m, v, g, *a, **k)

    monkeypatch.setattr(ops, "solver_adam", capture)
    x, cls, metas = _batch()
    model.train_step(x, metas, 0, 0, 0.01, [B1, B2], 0.0)
    torch.cuda.synchronize()
    assert seen["coef"] is not None
    n, nd = model.n_trainable, model.n_weights
    norm = _norm64(seen["G"], n, 1.0)
    got_norm, got_coef = model.last_grad_norm()
    c = float(np.float32(model.gradient_clip))
    assert abs(got_norm - norm) <= 1e-6 * norm and abs(got_coef - c / norm) <= 1e-6 and abs(got_coef - 0.5) <= 1e-2
    gv = seen["G"][:n].astype(np.float64) * (c / norm)
    assert nd < n and float(np.abs(seen["P"]).max()) <= 1.0
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    m_ref, v_ref = (1 - b1) * gv, (1 - b2) * gv * gv
    upd_ref = -float(np.float32(0.01)) * (m_ref / (1 - b1)) / (np.sqrt(v_ref / (1 - b2)) + 1e-8)
    upd = model.P.cpu().numpy().astype(np.float64)[:n] - seen["P"]
    # entries whose gradient is exactly zero (the padding) move by nothing in both; elsewhere |update| ~ lr
    e = _rel(upd, upd_ref)
    print("adam update %.2e" % e)
    assert e <= 1e-5


# ------------------------------------------------------------------------------------------------- 6. the running record
def test_statistics_record(hip):
    """four steps, the limit between the smallest and the largest of their norms (taken from a tracking-only run of an identically
    seeded model; the learning rate is tiny, so the clipped run's norms stay next to them): steps, clipped count, mean and maximum
    equal the host's recount from the per-step norms, reset zeroes the record"""
    lr = 1e-6

    def run(model):
        model.build_train_func("sgd")
        norms = []
        for it in range(4):
            x, cls, metas = _batch(20 + it)
            model.train_step(x, metas, 0, it, lr, [0.0], 0.0)
            norms.append(model.last_grad_norm())
        return norms

    tracked = _model()
    tracked.track_grad_norm = True
    free = [n for n, _ in run(tracked)]
    assert max(free) > 1.01 * min(free), free
    limit = 0.5 * (min(free) + max(free))
    model = _model()
    model.gradient_clip = limit
    pairs = run(model)
    norms = [np.float32(n) for n, _ in pairs]
    clipped = sum(1 for n in norms if np.float64(n) > np.float64(np.float32(limit)))
    assert 0 < clipped < 4, (norms, limit)
    assert [c < 1.0 for _, c in pairs] == [np.float64(n) > np.float64(np.float32(limit)) for n in norms]
    st = model.grad_norm_stats(reset=False)
    total = np.float64(0.0)
    for n in norms:
        total += np.float64(n)
    assert st["steps"] == 4 and st["clipped"] == clipped and st["nonfinite"] == 0
    assert st["mean"] == float(total) / 4 and st["max"] == float(max(norms)) and st["limit"] == limit
    lines = model.grad_norm_log_lines()
    assert len(lines) == 1 and "clipped %i of 4 steps" % clipped in lines[0] and "limit" in lines[0]
    st = model.grad_norm_stats()
    assert st["steps"] == 0 and st["clipped"] == 0 and st["mean"] == 0.0 and st["max"] == 0.0
    free_stats = tracked.grad_norm_stats()
    assert free_stats["steps"] == 4 and free_stats["clipped"] == 0 and free_stats["max"] == max(free)


# ------------------------------------------------------------------------------------------------- the driver
def test_cli_model_train_logs_the_record(hip, tmp_path):
    """model-train --gradient-clip 0.05 --gradient-norms for two epochs of three batches, in a child process: the limit's line at
    the start, one record line per epoch with every step clipped (asserted: the limit lies far below this stack's norms), the per-array table
    behind it at the default verbose level, finite costs"""
    import os
    import re
    import subprocess
    from fp64_model import png_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    train_dir, out = str(tmp_path / "train"), tmp_path / "out"
    png_dataset(train_dir, seed=1)
    out.mkdir()
    cmd = [os.path.join(root, "bin", "model-train"), "--seed", "0", "--solver", "nesterov", "--epochs", "2", "--batch-size", "4",
           "--train", train_dir, "--extension", "png", "--learn-rate", "0.05", "--learn-momentum", "0.9", "--learn-decay", "0.0005",
           "--border-mode", "half", "--model-desc"] + DESC.split() + ["--gradient-clip", "0.05", "--gradient-norms",
                                                                   "--output-prefix", str(out / "model")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "updates are clipped to a global gradient norm of 0.05" in log
    lines = re.findall(r"epoch (\d+) gradient norm: mean (\S+) max (\S+), clipped (\d+) of (\d+) steps \(limit (\S+)\)", log)
    assert [(int(e), int(k), int(n), float(c)) for e, _, _, k, n, c in lines] == [(0, 3, 3, 0.05), (1, 3, 3, 0.05)], log[-3000:]
    assert all(0.05 < float(mean) <= float(mx) and math.isfinite(float(mx)) for _, mean, mx, _, _, _ in lines)
    assert len(re.findall(r"L\d+\s+(?:conv|batchnorm)\s+.+?\s+grad \S+ weight \S+", log)) == 2 * 5, log[-3000:]
    costs = [float(c) for c in re.findall(r"cost: (\S+) \(lr", log)]
    assert len(costs) == 2 and all(math.isfinite(c) for c in costs), log[-3000:]
