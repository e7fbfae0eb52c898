"""Opt-in device-side RoI clustering (csrc/cluster.hip, ops.CLUSTER_DEVICE), the part that needs no GPU: the switch, the driver
flags, the C-ABI surface, and the CLOSED FORM the kernels implement - restated here in numpy (`closed_form_cluster`) and compared
with the sequential apply_cluster of oracle/build_samples_naive.py (denet/layer/denet_sparse.cc:165-242) + the final ranking.
tests/test_cluster_device_gpu.py imports the restatement for the device's tie rule."""
import os

import numpy as np
import pytest

import cabi
from denet_amd import lib as dlib, ops, switches
from oracle import build_samples_naive as NV

F32 = np.float32


def closed_form_edges(boxes, thr):
    """[n, n] bool: fp32 overlap_iou(i, j) > thr (SampleType::overlap_iou, denet_sparse.cc:86-101), no self edges"""
    b = np.ascontiguousarray(boxes, dtype=F32)
    thr = F32(thr)
    n = len(b)
    x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = ((x1 - x0) * (y1 - y0)).astype(F32)
    edge = np.zeros((n, n), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, n, 512):
            s = slice(lo, min(n, lo + 512))
            dx = np.maximum(F32(0), np.minimum(x1[s, None], x1[None, :]) - np.maximum(x0[s, None], x0[None, :])).astype(F32)
            dy = np.maximum(F32(0), np.minimum(y1[s, None], y1[None, :]) - np.maximum(y0[s, None], y0[None, :])).astype(F32)
            ai = (dx * dy).astype(F32)
            au = ((area[s, None] + area[None, :]).astype(F32) - ai).astype(F32)
            edge[s] = (ai / au).astype(F32) > thr
    edge[np.arange(n), np.arange(n)] = False
    return edge


def closed_form_cluster(ranked, thr, output_num):
    """indices (into `ranked` [n, 5] = pr, x0, y0, x1, y1 in rank order) of the clustered, ranked proposal by the closed form:
    1. groups = connected components of the graph "IoU > thr"; 2. a group stands where its youngest creator (a candidate without
    an edge to a smaller index) stood; 3. more than output_num groups: the first output_num by (size descending, key ascending);
    4. ratio = (output_num - G) / (n - G) in double, a kept group gives its 1 + floor(size * ratio) best members; 5. the picked
    candidates ranked and cut to output_num. "Best" and "ranked" by rank = index (the device's tie rule; on distinct scores the same
    as by score)."""
    r = np.asarray(ranked, dtype=F32)
    n = len(r)
    if n <= output_num:
        return np.arange(n)
    edge = closed_form_edges(r[:, 1:5], thr)
    label = np.full(n, -1, dtype=np.int64)
    for i in range(n):                       # single linkage: flood from the smallest index of every component
        if label[i] >= 0:
            continue
        label[i] = i
        front = np.zeros(n, dtype=bool)
        front[i] = True
        while front.any():
            front = edge[front].any(axis=0) & (label < 0)
            label[front] = i
    creator = ~np.tril(edge, -1).any(axis=1)
    roots = np.unique(label)
    size = np.bincount(label, minlength=n)
    key = np.full(n, -1, dtype=np.int64)
    np.maximum.at(key, label[creator], np.nonzero(creator)[0])
    order = sorted((int(g) for g in roots), key=lambda g: key[g])          # the reference's std::list order
    if len(order) > output_num:
        order = sorted(order, key=lambda g: (-size[g], key[g]))[:output_num]
    G = len(order)
    ratio = float(output_num - G) / float(n - G)
    picked = []
    for g in order:
        members = np.nonzero(label == g)[0]                                  # ascending index = best first
        picked.extend(members[:1 + int(np.floor(int(size[g]) * ratio))].tolist())
    return np.array(sorted(picked)[:output_num], dtype=np.int64)


def random_ranked(rng, n, cells, spread, maxsize=None):
    """n integer boxes on a cells x cells map, `spread` per centre on average (so that groups form; 1: anywhere), sides up to
    `maxsize` cells, distinct descending scores"""
    maxsize = maxsize or max(2, cells // 3)
    centres = rng.randint(0, cells, size=(max(2, n // spread), 2))
    c = centres[rng.randint(0, len(centres), n)]
    w, h = rng.randint(0, maxsize, n), rng.randint(0, maxsize, n)
    x0 = np.clip(c[:, 0] + rng.randint(-1, 2, n), 0, cells - 1)
    y0 = np.clip(c[:, 1] + rng.randint(-1, 2, n), 0, cells - 1)
    x1 = np.minimum(x0 + w, cells - 1)
    y1 = np.minimum(y0 + h, cells - 1)
    pr = (0.49 - 0.48 * (np.arange(n) + rng.uniform(0, 0.5, n)) / n).astype(F32)      # strictly decreasing, >= 0.24 / n apart
    assert len(np.unique(pr)) == n
    box = np.stack([x0, y0, x1, y1], axis=1).astype(np.int32)
    fb = np.stack([(x0 / float(cells)), (y0 / float(cells)), ((x1 + 1) / float(cells)), ((y1 + 1) / float(cells))], axis=1).astype(F32)
    return box, np.concatenate([pr[:, None], fb], axis=1).astype(F32)


def naive_cluster_ranked(ranked, thr, output_num):
    """oracle.build_samples_naive.apply_cluster + the final ranking (denet_sparse.cc:547-549) on a ranked list -> indices"""
    samples = [(float(r[0]), i, tuple(F32(v) for v in r[1:5])) for i, r in enumerate(ranked)]
    out = NV.apply_cluster(samples, F32(thr), len(samples), output_num)
    return np.array([s[1] for s in NV.rank(out)[:output_num]], dtype=np.int64)


def test_switch_is_registered_and_off_by_default():
    default, kind, text = switches.SWITCHES["DENET_CLUSTER_DEVICE"]
    assert default == "0" and kind == "kernels" and "OPT-IN" in text
    if "DENET_CLUSTER_DEVICE" not in os.environ:
        assert ops.CLUSTER_DEVICE is False
    was = ops.CLUSTER_DEVICE
    with ops.cluster_device(True):
        assert ops.CLUSTER_DEVICE is True
        with ops.cluster_device(False):
            assert ops.CLUSTER_DEVICE is False
        assert ops.CLUSTER_DEVICE is True
    assert ops.CLUSTER_DEVICE is was


def test_drivers_parse_device_cluster():
    from denet_amd.model import predict, train, train_multi
    for mod, argv in ((train, ["--train", "x"]), (train_multi, ["--train", "x"]), (predict, ["--model", "m", "--input", "x"])):
        parser = mod.build_parser()
        flags = {s for a in parser._actions for s in a.option_strings}
        assert "--device-cluster" in flags and "--device-render" in flags, mod.__name__
        action = [a for a in parser._actions if "--device-cluster" in a.option_strings][0]
        assert action.default is False and action.nargs == 0, mod.__name__


def test_cabi_declares_the_cluster_entries():
    """include/denet_hip.h and lib.SIGNATURES agree on the new entries, argument by argument; the refusals answer before any device
    work"""
    for name in ("denet_cluster_samples_workspace_bytes", "denet_cluster_samples_device"):
        _, restype, declared = cabi.declaration(name)
        res, args = dlib.SIGNATURES[name]
        assert res is restype, name
        assert declared == list(args), (name, declared, args)
    L = dlib.load()
    assert L.denet_cluster_samples_workspace_bytes(2, 5760) >= 2 * 5760 * 40
    assert L.denet_cluster_samples_workspace_bytes(2, 0) == 0
    one = 1
    for thr, what in ((-0.1, b"outside [0, 1)"), (1.0, b"outside [0, 1)")):
        assert L.denet_cluster_samples_device(one, one, one, 1, 8, thr, 4, 16, 16, one, one, one, one, 1 << 20, None) == -1000
        assert what in L.denet_last_error()
    assert L.denet_cluster_samples_device(one, one, one, 1, 8, 0.5, 0, 16, 16, one, one, one, one, 1 << 20, None) == -1000
    assert b"output_num" in L.denet_last_error()
    assert L.denet_cluster_samples_device(one, one, one, 1, 4096, 0.5, 4, 16, 16, one, one, one, one, 1024, None) == -1000
    assert b"workspace" in L.denet_last_error()


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.5, 0.7])
def test_closed_form_equals_the_sequential_reference(thr):
    """the contract of the kernels, pinned on the CPU: components / youngest-creator key / cut / take / rank give the list the
    reference's sequential apply_cluster + ranking gives, on integer-box lists with distinct scores - including lists with more
    groups than outputs (asserted to occur), where the creation order decides which groups survive"""
    rng = np.random.RandomState(int(thr * 10) + 1)
    more_groups = merged = 0
    for case in range(24):
        n = int(rng.randint(60, 260))
        cells = (16, 24, 32)[case % 3]
        _, ranked = random_ranked(rng, n, cells, spread=(8, 3, 1)[case % 3], maxsize=(6, 4, 2)[case % 3])
        out = (4, 9, 16, 36)[case % 4]
        got = closed_form_cluster(ranked, thr, out)
        ref = naive_cluster_ranked(ranked, thr, out)
        assert np.array_equal(got, ref), (thr, case, n, out)
        edge = closed_form_edges(ranked[:, 1:5], thr)
        groups = int((~np.tril(edge, -1).any(axis=1)).sum())          # creators >= groups; a late merge makes it strictly more
        label_count = len(set(_labels(edge)))
        more_groups += int(label_count > out)
        merged += int(groups > label_count)
    assert more_groups >= 4, "no case had more groups than outputs"
    assert merged >= 4, "no case merged two older groups"


def _labels(edge):
    n = len(edge)
    label = np.full(n, -1)
    for i in range(n):
        if label[i] >= 0:
            continue
        label[i] = i
        front = np.zeros(n, dtype=bool)
        front[i] = True
        while front.any():
            front = edge[front].any(axis=0) & (label < 0)
            label[front] = i
    return label.tolist()
