"""model-update-bn on the device (denet_amd/model/update_bn.py, csrc/bn_moments.hip) against float64 and the CPU oracle.

The semantics are those of denet/model/update_bn.py:42-70: the batch norms are estimated one after the other from test-mode
forward passes, each from the per-batch mean / biased variance of its raw input averaged over the full batches. After such a
sequential update the statistics are a fixed point: for every layer i, its new mean / variance equal the batch average of the
moments of its input in ONE test-mode forward of the UPDATED model (layers >= i cannot change that input). The oracle
(oracle/model.py, numpy) checks exactly that, and that estimating every layer from the original statistics misses it."""
import os
import subprocess

import numpy as np
import pytest
import torch

from denet_amd import ops
from denet_amd.layer.denet_corner import DeNetCornerLayer
from denet_amd.layer.denet_detect import DeNetDetectLayer
from denet_amd.layer.denet_sparse import DeNetSparseLayer
from denet_amd.model import model_cnn, update_bn, zoo
from oracle import model as OM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN_TYPES = ("batchnorm", "batchnorm-relu")
TOL_MEAN, TOL_VAR = 1e-3, 2e-3


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("M,C", [(1, 32), (37, 64), (4097, 256), (18432, 1536), (524288, 64)])
def test_moments_kernel_vs_fp64(hip, M, C):
    rng = np.random.RandomState(M % 1000 + C)
    mu = rng.normal(0.0, 3.0, C)
    sd = rng.uniform(0.05, 2.0, C)
    mu[C // 2] = 1e4 * sd[C // 2]          # the channel on which E[x^2] - mean^2 loses its digits
    batches = [(mu + sd * rng.standard_normal((M, C))).astype(np.float32) for _ in range(3)]
    ref = np.zeros((2, C))
    for x in batches:
        xd = x.astype(np.float64)
        m = xd.mean(axis=0)
        ref[0] += m
        ref[1] += ((xd - m) ** 2).mean(axis=0)
    dev = [torch.from_numpy(x).cuda() for x in batches]

    def run():
        acc = torch.zeros(2, C, dtype=torch.float64, device="cuda")
        ws = ops.bn_moments_workspace(M, C)
        for x in dev:
            ops.bn_moments_accumulate(x, acc, ws)
        return acc

    acc = run()
    got = acc.cpu().numpy()
    std = np.sqrt(ref[1])
    assert np.all(np.abs(got[0] - ref[0]) <= 1e-12 * (np.abs(ref[0]) + std)), np.max(np.abs(got[0] - ref[0]) / (np.abs(ref[0]) + std))
    assert np.all(np.abs(got[1] - ref[1]) <= 1e-9 * ref[1]), np.max(np.abs(got[1] - ref[1]) / np.maximum(ref[1], 1e-300))
    # run to run: bitwise
    assert np.array_equal(run().cpu().numpy().view(np.uint64), got.view(np.uint64))
    # finish: numpy's float32 formula of update_bn.py:62-66 from the same acc, bit for bit
    mean_dev, stdinv_dev = torch.full((C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")
    v0 = ops.WEIGHTS_VERSION
    ops.bn_moments_finish(acc, 3, mean_dev, stdinv_dev)
    assert ops.WEIGHTS_VERSION == v0 + 1
    m_ref = (got[0] / 3).astype(np.float32)
    var_ref = (got[1] / 3).astype(np.float32)
    s_ref = 1.0 / np.sqrt(var_ref + 1e-5)
    assert s_ref.dtype == np.float32
    assert np.array_equal(mean_dev.cpu().numpy().view(np.uint32), m_ref.view(np.uint32))
    assert np.array_equal(stdinv_dev.cpu().numpy().view(np.uint32), s_ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- helpers
def _oracle_selected(om):
    """the oracle's batch-norm nodes under the rule of update_bn.py:44-51 (top level and the layers of each resnet)"""
    out = []
    for n in om.nodes:
        if n["type"] in BN_TYPES:
            out.append(n)
        elif n["type"] == "resnet":
            out += [s for s in n["layers"] if s["type"] in BN_TYPES]
    return [n for n in out if n["enabled"]]


def _oracle_moments(monkeypatch, json_obj, B, batches):
    """batch-averaged (mean, biased variance) of the input of every selected batch norm in one test-mode oracle forward per
    batch, and the oracle's RoI lists per batch"""
    om = OM.OracleModel(json_obj, B)
    nodes = _oracle_selected(om)
    sums = {id(n): [0.0, 0.0] for n in nodes}
    orig = OM.op_bn

    def spy(x, node, train, relu):
        if id(node) in sums:
            xd = x.v.astype(np.float64)
            m = xd.mean(axis=(0, 2, 3))
            sums[id(node)][0] = sums[id(node)][0] + m
            sums[id(node)][1] = sums[id(node)][1] + ((xd - m[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        return orig(x, node, train, relu)

    monkeypatch.setattr(OM, "op_bn", spy)
    lists = []
    try:
        for x in batches:
            om.forward(x, None, train=False)
            lists.append(om.sample_bbox_list)
    finally:
        monkeypatch.setattr(OM, "op_bn", orig)
    n = len(batches)
    return [(sums[id(nd)][0] / n, sums[id(nd)][1] / n) for nd in nodes], lists


def _miss(mean, var, ref):
    """largest error of (mean, var) against ref = (mean, var), in units of the tolerances"""
    rm, rv = ref
    em = np.abs(mean - rm) / (np.sqrt(rv) + 1e-12) / TOL_MEAN
    ev = np.abs(var - rv) / (rv + 1e-12) / TOL_VAR
    return max(float(em.max()), float(ev.max()))


def _product_stats(layer):
    mean = layer.mean.get_value().astype(np.float64)
    var = 1.0 / layer.stdinv.get_value().astype(np.float64) ** 2 - 1e-5
    return mean, var


def _check_fixed_point(monkeypatch, model, json_before, batches):
    """every selected layer sits on the fixed point of the oracle; the non-sequential estimate (one oracle pass of the original
    model) misses it by > 20x the tolerance on some layer"""
    B = model.batch_size
    layers = update_bn.select_bn_layers(model)
    target, lists = _oracle_moments(monkeypatch, model.export_json(), B, batches)
    assert len(target) == len(layers)
    for i, (layer, ref) in enumerate(zip(layers, target)):
        mean, var = _product_stats(layer)
        assert _miss(mean, var, ref) <= 1.0, (i, layer.layer_index, _miss(mean, var, ref))
    naive, _ = _oracle_moments(monkeypatch, json_before, B, batches)
    assert max(_miss(nm, nv, ref) for (nm, nv), ref in zip(naive, target)) > 20.0
    return lists


def _params(model):
    """every parameter array of the model (nested layers included) by (layer index path, slot)"""
    out = {}
    for li, l in enumerate(model_cnn.walk_layers(model.layers)):
        for pi, p in enumerate(getattr(l, "params", lambda: [])()):
            out[(li, pi)] = (l, p, p.get_value().copy())
    return out


def _write_npy_dataset(path, x):
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "_data.npy"), x)
    np.save(os.path.join(path, "_labels.npy"), np.arange(x.shape[0]) % 3)


# ---------------------------------------------------------------------------------------------------------------- cifar3
def test_cifar3_fixed_point_and_only_statistics_change(hip, monkeypatch, tmp_path):
    """cifar3 (top-level `BN A`) with its middle batch norm disabled, 10 samples at batch size 4: exactly the first two exported
    batches are used, the statistics are the oracle's fixed point on them, nothing else changes, the disabled layer neither"""
    B = 4
    j = zoo.cifar3(B, 10, seed=2).export_json()
    bns = [l for l in j["layers"] if l["type"] == "batchnorm"]
    bns[1]["enabled"] = False
    model = model_cnn.load_from_json(j, B)
    json_before = model.export_json()
    x = np.random.RandomState(4).uniform(-1.0, 2.0, (10, 3, 32, 32)).astype(np.float32)
    _write_npy_dataset(str(tmp_path / "data"), x)
    batches = update_bn.load_batches(str(tmp_path / "data"), "npy", B, seed=5)
    assert len(batches) == 2
    import random
    random.seed(5)
    order = list(range(10))
    random.shuffle(order)
    assert np.array_equal(np.concatenate(batches), x[order[:8]])
    before = _params(model)
    chosen = update_bn.select_bn_layers(model)
    assert len(chosen) == 2
    res = update_bn.update_bn(model, batches)
    assert [r[0] for r in res] == chosen
    stats = set(id(p) for l in chosen for p in (l.mean, l.stdinv))
    for key, (l, p, v) in before.items():
        now = p.get_value()
        if id(p) in stats:
            assert not np.array_equal(now, v), (key, p.name)
        else:
            assert np.array_equal(now.view(np.uint32), v.view(np.uint32)), (key, p.name)
    for layer, old_m, new_m, old_s, new_s in res:
        assert np.array_equal(new_m, layer.mean.get_value()) and np.array_equal(new_s, layer.stdinv.get_value())
    _check_fixed_point(monkeypatch, model, json_before, batches)


def test_cifar3_inference_caches_refreshed(hip, tmp_path):
    """inference before the update fills the fold / test-coefficient caches; after update_bn and save, inference of the same
    model equals that of a fresh model loaded from the saved file, bit for bit"""
    B = 4
    model = zoo.cifar3(B, 10, seed=3)
    rng = np.random.RandomState(6)
    x = rng.uniform(0.0, 1.0, (B, 3, 32, 32)).astype(np.float32)
    batches = [rng.uniform(-1.0, 3.0, (B, 3, 32, 32)).astype(np.float32) for _ in range(3)]
    p0 = model.predict_output_step(x)
    update_bn.update_bn(model, batches)
    fname = str(tmp_path / "updated.mdl.gz")
    model_cnn.save_to_file(model, fname)
    p1 = model.predict_output_step(x)
    fresh = model_cnn.load_from_file(fname, B)
    p2 = fresh.predict_output_step(x)
    assert not np.array_equal(p0, p1)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- DeNet-34
DENET_B, DENET_IMG = 2, 128
DETECT_PARAMS = {"cornerThreshold": 0.01, "prThreshold": 0.01, "nmsThreshold": 0.5}


@pytest.fixture(scope="module")
def denet_updated(hip):
    """DeNet-34 skip (B = 2, 128x128) with a warm corner head: inference first (caches), then update_bn over two batches, with
    the forward calls of the RoI layers counted per estimated layer. The corner bias is the first of a short list for which the
    UPDATED model proposes RoIs in every image (the head batch norms are checked on them)."""
    mp = pytest.MonkeyPatch()
    calls = {"corner": 0, "sparse": 0, "detect": 0}
    for key, cls in (("corner", DeNetCornerLayer), ("sparse", DeNetSparseLayer), ("detect", DeNetDetectLayer)):
        orig = cls.forward

        def counted(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        mp.setattr(cls, "forward", counted)
    per_layer = []
    orig_finish = ops.bn_moments_finish

    def finish(*a, **k):
        per_layer.append(dict(calls))
        return orig_finish(*a, **k)
    mp.setattr(ops, "bn_moments_finish", finish)
    try:
        batches = [zoo.synthetic_batch(DENET_B, DENET_IMG, seed=s)[0] for s in (11, 12)]
        for bias in (7.5, 5.0, 2.5, 10.0):
            model = zoo.warm_corner_head(zoo.denet34(DENET_B, "skip", DENET_IMG, seed=1), bias=bias)
            json_before = model.export_json()
            dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
            dnd.get_detections(model, batches[0], None, DETECT_PARAMS)
            before = _params(model)
            calls.update(corner=0, sparse=0, detect=0)
            del per_layer[:]
            res = update_bn.update_bn(model, batches)
            lists = []
            dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
            for x in batches:
                model.forward(x, None, train=False)
                lists.append(dns.sample_bbox_list)
            if all(len(l) > 0 for ls in lists for l in ls):
                break
        counts = list(per_layer)
    finally:
        mp.undo()
    return dict(model=model, json_before=json_before, batches=batches, res=res, lists=lists, before=before, counts=counts,
                bias=bias)


def test_denet34_fixed_point_vs_oracle(denet_updated, monkeypatch):
    """stem BNA, the 35 batch norms of the resnet blocks (projection shortcuts included), the skip BNAs and the head BNAs
    behind denet-sparse: all on the oracle's fixed point; the RoI lists of product and oracle agree and are not empty"""
    d = denet_updated
    model = d["model"]
    assert all(len(l) > 0 for ls in d["lists"] for l in ls), "the updated model proposes no RoIs (corner bias %g)" % d["bias"]
    assert len(d["res"]) == 42
    lists = _check_fixed_point(monkeypatch, model, d["json_before"], d["batches"])
    # the same boxes in the same order; the scores are products of corner probabilities formed from 40 layers of fp32 (product)
    # and of numpy (oracle) arithmetic: relative 1e-2
    for got, ref in zip(d["lists"], lists):
        assert [[b for _, b in l] for l in got] == [[b for _, b in l] for l in ref]
        for gl, rl in zip(got, ref):
            np.testing.assert_allclose([p for p, _ in gl], [p for p, _ in rl], rtol=1e-2)


def test_denet34_only_statistics_change(denet_updated):
    d = denet_updated
    stats = set(id(p) for r in d["res"] for p in (r[0].mean, r[0].stdinv))
    assert len(stats) == 84
    for key, (l, p, v) in d["before"].items():
        now = p.get_value()
        if id(p) not in stats:
            assert np.array_equal(now.view(np.uint32), v.view(np.uint32)), (key, p.name)


def test_denet34_sweeps_are_truncated(denet_updated):
    """the sweep of a backbone batch norm ends after its top-level layer: while the stem BNA is estimated (and every other
    layer in front of the corner head) neither the corner, the RoI sampling nor the detection layer runs; the head BNAs need
    the RoI sampling but never the detection layer"""
    d = denet_updated
    counts = d["counts"]
    assert len(counts) == 42
    assert counts[0] == {"corner": 0, "sparse": 0, "detect": 0}
    model = d["model"]
    tops = [l for l in model.layers if l.type_name in BN_TYPES]
    dns_index = [i for i, l in enumerate(model.layers) if l.type_name == "denet-sparse"][0]
    head = [l for l in tops if l.layer_index > dns_index]
    assert len(head) == 4
    n_backbone = 42 - len(head)
    assert counts[n_backbone - 1] == {"corner": 0, "sparse": 0, "detect": 0}
    assert counts[-1]["sparse"] == 2 * len(head) and counts[-1]["detect"] == 0


def test_denet34_inference_caches_refreshed(denet_updated, tmp_path):
    """detections of the updated model (whose fold / test-coefficient caches were filled before the update) equal those of a
    fresh model loaded from the saved file, bit for bit"""
    d = denet_updated
    model = d["model"]
    fname = str(tmp_path / "denet.mdl.gz")
    model_cnn.save_to_file(model, fname)
    x = d["batches"][0]
    dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
    r1 = dnd.get_detections(model, x, None, DETECT_PARAMS)
    out1 = [np.asarray(t.cpu().numpy() if torch.is_tensor(t) else t) for t in dnd.last_outputs]
    fresh = model_cnn.load_from_file(fname, DENET_B)
    fdnd = [l for l in fresh.layers if l.type_name == "denet-detect"][0]
    r2 = fdnd.get_detections(fresh, x, None, DETECT_PARAMS)
    out2 = [np.asarray(t.cpu().numpy() if torch.is_tensor(t) else t) for t in fdnd.last_outputs]
    assert [r["detections"] for r in r1] == [r["detections"] for r in r2]
    for a, b in zip(out1, out2):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_end_to_end(hip, tmp_path):
    """bin/model-update-bn on an npy dataset equals update_bn in-process with the same seed; with fewer samples than one batch
    it fails and writes nothing"""
    B = 4
    rng = np.random.RandomState(9)
    data = str(tmp_path / "data")
    _write_npy_dataset(data, rng.uniform(-1.0, 2.0, (11, 3, 32, 32)).astype(np.float32))
    mfile, out = str(tmp_path / "in.mdl.gz"), str(tmp_path / "out.mdl.gz")
    model_cnn.save_to_file(zoo.cifar3(B, 10, seed=4), mfile)
    cmd = [os.path.join(ROOT, "bin", "model-update-bn"), "--model", mfile, "--output", out, "--input", data, "--extension", "npy",
           "--batch-size", str(B), "--seed", "1", "--thread-num", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Found 3 batch norm layers" in r.stdout
    got = model_cnn.load_from_file(out, B)
    ref = model_cnn.load_from_file(mfile, B)
    update_bn.update_bn(ref, update_bn.load_batches(data, "npy", B, seed=1))
    for a, b in zip(update_bn.select_bn_layers(got), update_bn.select_bn_layers(ref)):
        assert np.array_equal(a.mean.get_value(), b.mean.get_value())
        assert np.array_equal(a.stdinv.get_value(), b.stdinv.get_value())
    small = str(tmp_path / "small")
    _write_npy_dataset(small, rng.uniform(0.0, 1.0, (3, 3, 32, 32)).astype(np.float32))
    out2 = str(tmp_path / "never.mdl.gz")
    cmd2 = [c if c not in (data, out) else {data: small, out: out2}[c] for c in cmd]
    r2 = subprocess.run(cmd2, capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0
    assert not os.path.exists(out2)
