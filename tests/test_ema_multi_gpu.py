"""The weight average under two real ranks on one GPU: the harness of tests/test_multi_gpu.py reused as it
is - its worker script with two statements added (the mode switched on, the average saved), its in-process emulation of the
all-reduce with the mode on in the replica that takes the merged gradient. Every rank keeps its own average from bit-identical
inputs and nothing is communicated, so both ranks' E and ES must hold the same bits, and they must be the single-process result."""
import numpy as np
import pytest
import torch

import test_multi_gpu as tm
from test_ema_host import bound
from test_multi_gpu import heuristic_kernels  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

D = 0.9


def _worker_with_average():
    build, saved = 'model.build_train_func("nesterov")', '"S": model.S.cpu(), '
    assert tm.WORKER.count(build) == 1 and tm.WORKER.count(saved) == 1
    return tm.WORKER.replace(build, "model.ema_decay = %r\n" % D + build).replace(
        saved, saved + '"E": model.E.cpu(), "ES": model.ES.cpu(), "updates": model.ema_updates, ')


def test_two_ranks_keep_the_same_average(hip, tmp_path, monkeypatch, heuristic_kernels):  # noqa: F811
    monkeypatch.setattr(tm, "WORKER", _worker_with_average())
    got = tm._run_two_ranks(tmp_path, "grad")
    for k in ("P", "M", "S", "E", "ES"):
        assert torch.equal(got[0][k], got[1][k]), "ranks diverged in " + k
    assert got[0]["updates"] == got[1]["updates"] == tm.STEPS
    assert not torch.equal(got[0]["E"], got[0]["P"])
    # the single-process result on the all-reduced gradient: the emulation of test_multi_gpu with the mode on in replica 0
    reps = tm._replicas()
    reps[0]["m"].ema_decay = D
    cap = tm._Capture()
    reps[1]["m"].dist = cap
    reps[0]["m"].dist = tm._Merge(cap)
    from denet_amd import ops
    for it in range(tm.STEPS):
        with pytest.raises(tm._Abort):
            tm._step(reps[1], it)
        tm._step(reps[0], it)
        torch.cuda.synchronize()
        for name in ("P", "M", "S"):
            getattr(reps[1]["m"], name).copy_(getattr(reps[0]["m"], name))
        ops.bump_weights_version()
    m0 = reps[0]["m"]
    assert m0.ema_updates == tm.STEPS and reps[1]["m"].E is None
    # test_multi_gpu allows the two-process parameters 1e-6 of their largest entry from the emulation; an average is a convex
    # combination of parameters, so it may differ by that much plus its own rounding (3 n u A_max, test_ema_host.bound)
    for k, src in (("E", "P"), ("ES", "S")):
        ref = getattr(m0, k).cpu()
        a_max = float(getattr(m0, src).abs().max())
        err = float((got[0][k] - ref).abs().max())
        lim = 1e-6 * a_max + bound(tm.STEPS, a_max)
        print("%s: two ranks against the emulation %.3e (allowed %.3e)" % (k, err, lim))
        assert np.isfinite(err) and err <= lim, (k, err, lim)
