"""The exponential moving average of the weights on the GPU (csrc/ema.hip): the update kernel against the
float64 recurrence under a derived bound, its exact properties, the exchange kernel, "the mode only observes" in the bits and in the
kernel audit, the model's average against float64 over whole steps (plain, accumulated, every solver, updates left to the caller),
frozen and padded entries, ema_weights() / save_ema, and the driver.

The bound (tests/test_ema_host.py `bound`): with u = 2^-24 and A = max(|e|, |p|), one update errs by at most 3 u A; n chained
updates by at most 3 n u A_max, because an error already in e is carried with the factor 1 - om <= 1."""
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from denet_amd import ops
from denet_amd.layer.convolution import ConvLayer
from denet_amd.model import audit, model_cnn
from fp64_model import build_model, png_dataset
from test_ema_host import U, bound, ema64, om_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the issue's sizes, and one above 4 x 256 x 2048 floats, where the capped grid of the vector body takes a second pass
SIZES = (1, 3, 4, 255, 256, 257, 1023, 8197, 2 ** 20 + 3, 3 * 2 ** 20 + 5)
# (offset of e / a, offset of p / b) in floats from the allocation: as allocated, both one float on (a 3-float scalar head in front
# of the vectors), and e alone one float on (no vector is aligned on both: the all-scalar path)
OFFSETS = ((0, 0), (1, 1), (1, 0))
OMS = tuple(float(np.float32(v)) for v in (0.9, 0.1, 1e-4))      # the float32 the kernel is handed, as doubles
GUARD = 8                 # guard words on either side (32 bytes: the views keep the allocation's 16-byte phase)
GUARD_VALUE = 12345.0


def _guarded(values, off):
    """a device buffer [guards | off floats | values | guards] and the view of `values` inside it"""
    n = len(values)
    host = np.full(2 * GUARD + off + n, GUARD_VALUE, dtype=np.float32)
    host[GUARD + off:GUARD + off + n] = values
    buf = torch.from_numpy(host).cuda()
    view = buf[GUARD + off:GUARD + off + n]
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * (GUARD + off) and buf.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf, off, n):
    host = buf.cpu().numpy()
    return bool((host[:GUARD + off] == GUARD_VALUE).all() and (host[GUARD + off + n:] == GUARD_VALUE).all())


# ------------------------------------------------------------------------------------------------- 1. the kernel against float64
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_vs_float64(hip, n):
    """one update, and five chained updates with a fresh p each, for every offset pair and every om: |device - float64| within
    3 u max(|e|, |p|) per entry after one update, within 3 * 5 * u * A_max after five"""
    rng = np.random.RandomState(n % 1000)
    e0 = rng.normal(size=n).astype(np.float32)
    ps = [rng.normal(size=n).astype(np.float32) for _ in range(5)]
    a_max = max(float(np.abs(v).max()) for v in [e0] + ps)
    worst1 = worst5 = 0.0
    on_device = {op: [_guarded(p_host, op) for p_host in ps] for op in (0, 1)}      # uploaded once, read by every combination
    for oe, op in OFFSETS:
        for om in OMS:
            ebuf, e = _guarded(e0, oe)
            ref = e0.astype(np.float64)
            for k, p_host in enumerate(ps):
                pbuf, p = on_device[op][k]
                ops.ema_update(e, p, om)
                ref = ema64(ref, p_host, om)
                if k == 0:
                    err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
                    lim = 3.0 * U * np.maximum(np.abs(e0), np.abs(p_host)).astype(np.float64)
                    worst1 = max(worst1, float((err / np.maximum(lim, 1e-300)).max()))
                    assert (err <= lim).all(), (n, oe, op, om, float(err.max()))
            err = float(np.abs(e.cpu().numpy().astype(np.float64) - ref).max())
            worst5 = max(worst5, err / bound(5, a_max))
            assert err <= bound(5, a_max), (n, oe, op, om, err, bound(5, a_max))
            assert _guards_intact(ebuf, oe, n)
    for op, bufs in on_device.items():
        for (pbuf, p), p_host in zip(bufs, ps):
            assert _guards_intact(pbuf, op, n) and p.cpu().numpy().tobytes() == p_host.tobytes()
    print("n = %d: worst error / bound after one update %.3f, after five %.3f" % (n, worst1, worst5))


# ------------------------------------------------------------------------------------------------- 2. the kernel: exact properties
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_exact_properties(hip, n):
    """p == e leaves every bit of e (inputs without negative zeros) and every value (inputs with them); no float outside [0, n) is
    touched on either side of either buffer"""
    rng = np.random.RandomState(7 + n % 1000)
    v = rng.normal(size=n).astype(np.float32)
    assert not (v == 0).any()
    z = v.copy()
    z[::3] = -0.0
    z[1::5] = 0.0
    for oe, op in OFFSETS:
        for om in OMS:
            for values, bits in ((v, True), (z, False)):
                ebuf, e = _guarded(values, oe)
                pbuf, p = _guarded(values, op)
                ops.ema_update(e, p, om)
                got = e.cpu().numpy()
                assert np.array_equal(got, values), (n, oe, op, om)
                if bits:
                    assert got.tobytes() == values.tobytes(), (n, oe, op, om)
                assert p.cpu().numpy().tobytes() == values.tobytes()
                assert _guards_intact(ebuf, oe, n) and _guards_intact(pbuf, op, n)
    # om = 1 lands on p wherever p - e is exact, om = 0 keeps e
    ebuf, e = _guarded(v, 1)
    pbuf, p = _guarded(np.float32(2.0) * v, 1)
    ops.ema_update(e, p, 0.0)
    assert e.cpu().numpy().tobytes() == v.tobytes()
    ops.ema_update(e, p, 1.0)
    assert np.array_equal(e.cpu().numpy(), np.float32(2.0) * v)
    # a non-finite parameter makes the average non-finite
    bad = v.copy()
    bad[n // 2] = np.nan
    pbuf, p = _guarded(bad, 1)
    ops.ema_update(e, p, 0.1)
    assert math.isnan(float(e[n // 2])) and int(torch.isnan(e).sum()) == 1


# ------------------------------------------------------------------------------------------------- 3. the exchange
@pytest.mark.parametrize("n", SIZES)
def test_swap_kernel(hip, n):
    rng = np.random.RandomState(11 + n % 1000)
    # raw bit patterns (NaNs with payloads, denormals, negative zeros among them): bits are moved, nothing is computed
    a_host = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    b_host = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for oa, ob in OFFSETS:
        abuf, a = _guarded(a_host, oa)
        bbuf, b = _guarded(b_host, ob)
        ops.swap(a, b)
        assert a.cpu().numpy().tobytes() == b_host.tobytes() and b.cpu().numpy().tobytes() == a_host.tobytes(), (n, oa, ob)
        assert _guards_intact(abuf, oa, n) and _guards_intact(bbuf, ob, n)
        ops.swap(a, b)
        assert a.cpu().numpy().tobytes() == a_host.tobytes() and b.cpu().numpy().tobytes() == b_host.tobytes(), (n, oa, ob)
        assert _guards_intact(abuf, oa, n) and _guards_intact(bbuf, ob, n)


# ------------------------------------------------------------------------------------------------- the small stack
DESC = "C[32,3] BN A P[2] C[20,3] A R"        # pads channels at the input (3 -> 4), in the middle (20 -> 32), at the head (10 -> 32)
B, CLS = 4, 10
LR, MOM, DECAY = 0.1, 0.9, 0.0005
D = 0.9


def _model(seed=5, ema=0.0, **kw):
    m = build_model(DESC, (3, 32, 32), B, CLS, seed=seed, **kw)
    m.ema_decay = ema
    return m


def _batch(seed=11):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    cls = rng.randint(0, CLS, B)
    return x, [{"image_class": int(c)} for c in cls]


def _step(model, it, seed=None, lr=LR, mom=(MOM,)):
    x, metas = _batch(11 + it if seed is None else seed)
    return model.train_step(x, metas, 0, it, lr, list(mom), DECAY)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


@pytest.fixture(autouse=True)
def _direct_kernels():
    """every step of this file on the direct kernels: nothing is measured, twins of one seed run the same launches"""
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        yield


def _within(dev, ref, n_updates, snapshots, what):
    """|dev - ref| within the derived bound, A_max taken over every snapshot the recurrence read"""
    a_max = max(float(np.abs(s).max()) for s in snapshots)
    err = float(np.abs(dev.astype(np.float64) - ref).max())
    print("%s: error %.3e, bound %.3e (A_max %.3g, %d updates)" % (what, err, bound(n_updates, a_max), a_max, n_updates))
    assert err <= bound(n_updates, a_max), (what, err, bound(n_updates, a_max))


# ------------------------------------------------------------------------------------------------- 4. the mode only observes
def _three_steps(model):
    model.build_train_func("nesterov")
    syms, costs = [], []
    for it in range(3):
        x, metas = _batch(11 + it)
        with audit.KernelAudit(model) as ka:
            costs.append(model.train_step(x, metas, 0, it, LR, [MOM], DECAY))
        syms.append([s for r in ka.table for s in r["fwd"] + r["bwd"]] + list(ka.other))
    torch.cuda.synchronize()
    return syms, costs, [t.clone() for t in (model.P, model.M, model.S)]


def test_mode_only_observes(hip):
    plain_syms, plain_costs, plain = _three_steps(_model())
    ema_syms, ema_costs, state = _three_steps(_model(ema=D))
    for step in plain_syms:
        assert step and not [s for s in step if s in ops.EMA_KERNELS]
    for a, b in zip(ema_syms, plain_syms):
        assert [s for s in a if s in ops.EMA_KERNELS] == ["ema_update_kernel", "ema_update_kernel"]
        assert [s for s in a if s not in ops.EMA_KERNELS] == b
    assert ema_costs == plain_costs and all(math.isfinite(c[0]) for c in plain_costs)
    for a, b in zip(state, plain):
        assert a.numel() == b.numel() and torch.equal(a, b)
    assert plain[1].any() and plain[2].any()


# ------------------------------------------------------------------------------------------------- 5. the model against float64
@pytest.fixture(scope="module")
def averaged(hip):
    """four nesterov steps with the mode on; host snapshots of P and S before step 1 and after every step. Shared, never changed"""
    with ops.algorithms(table={}, POLICY=ops.direct_policy):
        model = _model(ema=D, spread_bn=True, head_scale=0.05)
        model.build_train_func("nesterov")
        assert model.E is None and model.ema_updates == 0
        snaps_p, snaps_s = [_host(model.P)], [_host(model.S)]
        for it in range(4):
            _step(model, it)
            snaps_p.append(_host(model.P))
            snaps_s.append(_host(model.S))
    return {"model": model, "P": snaps_p, "S": snaps_s}


def _recurrence(snaps, d=D):
    e = snaps[0].astype(np.float64)
    for t, p in enumerate(snaps[1:]):
        e = ema64(e, p, om_at(t, d))
    return e


def test_model_average_vs_float64(hip, averaged):
    model = averaged["model"]
    assert model.ema_updates == 4
    assert not np.array_equal(averaged["P"][0], averaged["P"][4]) and not np.array_equal(averaged["S"][0], averaged["S"][4])
    assert model.E.numel() == model.P.numel() and model.ES.numel() == model.S.numel() and model.E.dtype == torch.float32
    _within(_host(model.E), _recurrence(averaged["P"]), 4, averaged["P"], "E")
    _within(_host(model.ES), _recurrence(averaged["S"]), 4, averaged["S"], "ES")
    # the average is neither the weights nor their start
    assert not np.array_equal(_host(model.E), averaged["P"][4]) and not np.array_equal(_host(model.E), averaged["P"][0])


# ------------------------------------------------------------------------------------------------- 6. frozen and padded entries
def test_frozen_and_padded_entries_do_not_drift(hip):
    """the second convolution is frozen (enabled = False): its filter lies behind n_trainable. Those floats and every alignment gap
    of E hold the bits of P after three steps, while the trained entries have moved"""
    model = _model(ema=D)
    convs = [l for l in model.layers if l.type_name == "conv"]
    convs[1].enabled = False
    model.build_train_func("nesterov")
    for it in range(3):
        _step(model, it)
    P, E = _host(model.P), _host(model.E)
    n = model.n_trainable
    assert 0 < n < P.size and model.ema_updates == 3
    assert E[n:].tobytes() == P[n:].tobytes() and np.abs(P[n:]).max() > 0
    gap = np.ones(P.size, dtype=bool)
    for lo, hi in model.param_ranges.values():
        gap[lo:hi] = False
    assert gap.any() and E[gap].tobytes() == P[gap].tobytes() and not P[gap].any()
    assert not np.array_equal(E[:n], P[:n])
    # padded channels inside the trained arrays: wherever P did not move from its start, E did not either
    first = convs[0].omega
    lo, hi = model.param_ranges[id(first)]
    pad = P[lo:hi].reshape(first.dev_shape)[..., 3:]
    assert pad.size and not pad.any() and not E[lo:hi].reshape(first.dev_shape)[..., 3:].any()


# ------------------------------------------------------------------------------------------------- 7. ema_weights()
def test_ema_weights_block(hip, averaged, tmp_path, monkeypatch):
    model = averaged["model"]
    folded = []
    ff0 = ConvLayer.forward_folded

    def counted(layer, *a, **k):
        folded.append(layer)
        return ff0(layer, *a, **k)

    monkeypatch.setattr(ConvLayer, "forward_folded", counted)
    assert ops.INFER_FOLD
    x, metas = _batch(40)
    state = [t.clone() for t in (model.P, model.S, model.E, model.ES)]
    torch.cuda.synchronize()
    before = model.predict_output_step(x)
    assert len(folded) == 1                                # the `C BN A` front runs as one folded pass
    with model.ema_weights() as m:
        assert m is model
        assert torch.equal(model.P, state[2]) and torch.equal(model.S, state[3])
        assert torch.equal(model.E, state[0]) and torch.equal(model.ES, state[1])
        inside = model.predict_output_step(x)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            with model.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            model.train_step(x, metas, 0, 4, LR, [MOM], DECAY)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            model.ema_step()
        assert torch.equal(model.P, state[2])              # the refusals changed nothing
    assert len(folded) == 2
    assert np.isfinite(inside).all() and 0.0 < float(inside.max()) < 1.0 and not np.array_equal(inside, before)
    for t, s in zip((model.P, model.S, model.E, model.ES), state):
        assert torch.equal(t, s)
    after = model.predict_output_step(x)
    assert after.tobytes() == before.tobytes()
    # an exception in the body still exchanges back
    with pytest.raises(KeyError):
        with model.ema_weights():
            assert torch.equal(model.P, state[2])
            raise KeyError("body")
    for t, s in zip((model.P, model.S, model.E, model.ES), state):
        assert torch.equal(t, s)
    assert model.predict_output_step(x).tobytes() == before.tobytes()
    # the average as a model file
    fname = str(tmp_path / "avg.mdl.gz")
    model.save_ema(fname)
    for t, s in zip((model.P, model.S, model.E, model.ES), state):
        assert torch.equal(t, s)
    loaded = model_cnn.load_from_file(fname, B)
    assert loaded.ema_decay == 0.0 and "ema" not in " ".join(loaded.export_json().keys()).lower()
    assert loaded.predict_output_step(x).tobytes() == inside.tobytes()
    assert model.ema_updates == 4


def test_ema_weights_before_any_update(hip):
    model = _model(ema=D)
    model.build_train_func("nesterov")
    with pytest.raises(RuntimeError, match="before the first update"):
        with model.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="before the first update"):
        model.save_ema("never-written.mdl.gz")
    assert not os.path.exists("never-written.mdl.gz")


# ------------------------------------------------------------------------------------------------- 8. acc mode
def test_acc_mode_updates_once(hip):
    model = _model(ema=D)
    model.build_train_func("nesterov", use_acc_mode=True)
    p0, s0 = _host(model.P), _host(model.S)
    model.train_begin()
    for it in range(2):
        _step(model, it)
        assert model.ema_updates == 0
        assert _host(model.E).tobytes() == p0.tobytes() and _host(model.ES).tobytes() == s0.tobytes()
    model.train_end()
    assert model.ema_updates == 1
    p1, s1 = _host(model.P), _host(model.S)
    assert not np.array_equal(p0, p1) and not np.array_equal(s0, s1)
    _within(_host(model.E), ema64(p0, p1, om_at(0, D)), 1, [p0, p1], "E")
    _within(_host(model.ES), ema64(s0, s1, om_at(0, D)), 1, [s0, s1], "ES")


# ------------------------------------------------------------------------------------------------- 9. ema_auto = False
def test_updates_left_to_the_caller(hip):
    model = _model(ema=D)
    model.ema_auto = False
    model.build_train_func("nesterov")
    p0, s0 = _host(model.P), _host(model.S)
    for it in range(2):
        _step(model, it)
    assert model.ema_updates == 0
    assert _host(model.E).tobytes() == p0.tobytes() and _host(model.ES).tobytes() == s0.tobytes()      # copied when step 1 began
    p2, s2 = _host(model.P), _host(model.S)
    assert not np.array_equal(p0, p2)
    model.ema_step()
    assert model.ema_updates == 1
    _within(_host(model.E), ema64(p0, p2, om_at(0, D)), 1, [p0, p2], "E")
    _within(_host(model.ES), ema64(s0, s2, om_at(0, D)), 1, [s0, s2], "ES")
    model.ema_step()
    assert model.ema_updates == 2
    _within(_host(model.E), ema64(ema64(p0, p2, om_at(0, D)), p2, om_at(1, D)), 2, [p0, p2], "E twice")


# ------------------------------------------------------------------------------------------------- 10. every solver branch
@pytest.mark.parametrize("solver,mom,lr", [("sgd", (MOM,), LR), ("adam", (0.9, 0.999), 0.01)])
def test_every_solver_updates(hip, solver, mom, lr):
    model = _model(ema=D)
    model.build_train_func(solver)
    p0, s0 = _host(model.P), _host(model.S)
    _step(model, 0, lr=lr, mom=mom)
    assert model.ema_updates == 1
    p1, s1 = _host(model.P), _host(model.S)
    assert not np.array_equal(p0, p1)
    _within(_host(model.E), ema64(p0, p1, om_at(0, D)), 1, [p0, p1], solver + " E")
    _within(_host(model.ES), ema64(s0, s1, om_at(0, D)), 1, [s0, s1], solver + " ES")
    assert not np.array_equal(_host(model.E), p1) and not np.array_equal(_host(model.E), p0)


# ------------------------------------------------------------------------------------------------- 11. the driver
def test_cli_model_train_writes_the_average(hip, tmp_path):
    """model-train --ema 0.9 --test for two epochs of three batches, in a child process: the start line, the average's model and
    .test files beside the usual ones, one `ema test error` line per epoch, and the average's file loads and predicts"""
    train_dir, test_dir, out = str(tmp_path / "train"), str(tmp_path / "test"), tmp_path / "out"
    png_dataset(train_dir, seed=1)
    png_dataset(test_dir, per_class=2, seed=2)
    out.mkdir()
    cmd = [os.path.join(ROOT, "bin", "model-train"), "--seed", "0", "--solver", "nesterov", "--epochs", "2", "--batch-size", "4",
           "--train", train_dir, "--test", test_dir, "--extension", "png", "--learn-rate", "0.05", "--learn-momentum", "0.9",
           "--learn-decay", "0.0005", "--border-mode", "half", "--model-desc"] + DESC.split() + ["--ema", "0.9", "--output-prefix",
                                                                                              str(out / "model")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "an average of the weights is kept on the device (--ema 0.9)" in log and "min(0.9, (1 + t) / (10 + t))" in log
    assert "not resumed" not in log                          # no --model: nothing was loaded
    names = sorted(os.path.basename(f) for f in glob.glob(str(out / "model_*")) if f.endswith((".mdl.gz", ".test")))
    usual = ["model_epoch000.mdl.gz", "model_epoch000.test", "model_epoch001.mdl.gz", "model_epoch001.test", "model_epoch001_final.mdl.gz"]
    assert names == sorted(usual + [n.replace("_epoch", "_ema_epoch") for n in usual]), names
    assert [int(e) for e in re.findall(r"epoch (\d+) test error: \S+%", log)] == [0, 1], log[-3000:]
    assert [int(e) for e in re.findall(r"epoch (\d+) ema test error: \S+%", log)] == [0, 1], log[-3000:]
    costs = [float(c) for c in re.findall(r"cost: (\S+) \(lr", log)]
    assert len(costs) == 2 and all(math.isfinite(c) for c in costs), log[-3000:]
    assert "Overall Error=" in open(str(out / "model_ema_epoch001.test")).read()
    from denet_amd.model import train_multi
    assert os.path.basename(train_multi.find_restart(str(out / "model"))[0]) == "model_epoch001_final.mdl.gz"
    x = np.random.RandomState(3).uniform(0.0, 1.0, (4, 3, 32, 32)).astype(np.float32)
    avg = model_cnn.load_from_file(str(out / "model_ema_epoch001_final.mdl.gz"), 4)
    last = model_cnn.load_from_file(str(out / "model_epoch001_final.mdl.gz"), 4)
    pr_avg, pr_last = avg.predict_output_step(x), last.predict_output_step(x)
    assert pr_avg.shape == (4, 3) and np.isfinite(pr_avg).all() and np.allclose(pr_avg.sum(axis=1), 1.0, atol=1e-5)
    differ = [not np.array_equal(pa.get_value(), pb.get_value()) for la, lb in zip(avg.layers, last.layers)
              for pa, pb in zip(getattr(la, "all_params", list)(), getattr(lb, "all_params", list)())]
    assert differ and all(differ)                            # the average is not the last iterate
    assert pr_last.shape == pr_avg.shape
