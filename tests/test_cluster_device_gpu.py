"""Opt-in device-side RoI clustering (csrc/cluster.hip, ops.CLUSTER_DEVICE, --device-cluster) on the GPU: the kernels against the
host routine (denet_host_cluster_samples), the C++ oracle (oracle_cluster_ranked) and the numpy restatement of the closed form
(tests/test_cluster_device_host.py) - exactly: boxes, |d| bits, counts - then through the DNS layer, a training step, the mode
switch and model-predict. Parity is list equality, not a tolerance: the problem is closed and integer."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from denet_amd import lib, ops
from denet_amd.model import audit, zoo
from oracle import model as OM
from oracle import layers as OL
from tests.test_cluster_device_host import closed_form_cluster, random_ranked

F32 = np.float32


def _absd(n, step=0.01):
    """|d| of n ranked candidates: ascending, `step` apart - far enough that denet_samples_finish_host's fp32 scores are distinct
    (asserted by _finish)"""
    return (0.5 + step * np.arange(n)).astype(F32)


def _finish(box, absd, cnt, H, W, distinct=True):
    """[B, N, 5] rows of denet_samples_finish_host (pr, fp32 box) of a packed proposal"""
    rows = ops.samples_finish_host(torch.from_numpy(np.ascontiguousarray(box, np.int32)), torch.from_numpy(np.ascontiguousarray(absd, F32)),
                                   torch.from_numpy(np.ascontiguousarray(cnt, np.int32)), H, W).numpy()
    if distinct:
        for b in range(len(cnt)):
            assert len(np.unique(rows[b, :cnt[b], 0])) == cnt[b], "the test list must not hold equal scores"
    return rows


def _device(box, absd, cnt, thr, out, H, W):
    """ops.cluster_samples_device on host arrays -> host arrays (box [B, out, 4], |d| [B, out], count [B])"""
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (box.astype(np.int32), absd.astype(F32), cnt.astype(np.int32))]
    ob, oa, oc = ops.cluster_samples_device(d[0], d[1], d[2], thr, out, H, W)
    torch.cuda.synchronize()
    return ob.cpu().numpy(), oa.cpu().numpy(), oc.cpu().numpy()


def _check_exact(box, absd, cnt, thr, out, H, W, oracle=True):
    """device result == host routine == oracle == closed form, exactly; returns per image whether clustering changed the selection"""
    box, absd, cnt = np.asarray(box, np.int32), np.asarray(absd, F32), np.asarray(cnt, np.int32)
    B, N = absd.shape
    rows = _finish(box, absd, cnt, H, W)
    gb, ga, gc = _device(box, absd, cnt, thr, out, H, W)
    hrows, hcnt = ops.cluster_samples_host(rows, cnt, thr, out)
    assert np.array_equal(gc, hcnt), (gc, hcnt)
    got_rows = _finish(gb, ga, gc, H, W)
    changed = []
    for b in range(B):
        n, m = int(cnt[b]), int(gc[b])
        idx = closed_form_cluster(rows[b, :n], thr, out)
        assert m == len(idx), (b, m, len(idx))
        assert np.array_equal(gb[b, :m], box[b, idx]), "image %d: boxes" % b
        assert np.array_equal(ga[b, :m].view(np.uint32), absd[b, idx].view(np.uint32)), "image %d: |d| bits" % b
        assert not gb[b, m:].any() and not ga[b, m:].any(), "rows past the count must be zero"
        assert np.array_equal(got_rows[b, :m], hrows[b, :m]), "image %d: host routine" % b
        if oracle and n > out:
            oc = OM.oracle_cluster_ranked(rows[b, :n], thr, out)
            assert np.array_equal(got_rows[b, :m], oc), "image %d: oracle" % b
        changed.append(not np.array_equal(idx, np.arange(min(n, out))))
    return changed


def _random_case(seed, n, cells_w, cells_h, spread, maxsize, B=1):
    rng = np.random.RandomState(seed)
    boxes = []
    for _ in range(B):
        box, _ = random_ranked(rng, n, min(cells_w, cells_h), spread, maxsize)
        boxes.append(box)
    return np.stack(boxes), np.stack([_absd(n, 0.001 if n > 1000 else 0.01)] * B), np.full(B, n, np.int32)


CRAFTED = {}


def _crafted(name):
    def reg(fn):
        CRAFTED[name] = fn
        return fn
    return reg


@_crafted("chain")
def _case_chain():
    # A - B and B - C overlap with IoU 1/3, A and C do not touch; rank order A, C, B: B arrives last and merges the two
    boxes = [(0, 0, 3, 3), (4, 0, 7, 3), (2, 0, 5, 3), (10, 10, 11, 11), (13, 13, 14, 14)]
    return np.array([boxes]), _absd(5)[None], np.array([5]), 0.3, 3, 16, 16, [[0, 3, 4]]


@_crafted("youngest_creator")
def _case_key():
    # X = {0, 2, 5}: 5 joins the groups of 0 and 2 (IoU 0.25 each), it stands where 2 stood; Y = {1, 3, 4} stands where 1 stood.
    # Four groups for one output, X and Y both of size 3: Y is first in the reference's list - a key "smallest index" would keep X
    boxes = [(0, 0, 3, 3), (0, 10, 3, 13), (6, 0, 9, 3), (1, 10, 4, 13), (0, 11, 3, 14), (2, 0, 7, 3), (20, 20, 21, 21), (25, 25, 26, 26)]
    return np.array([boxes]), _absd(8)[None], np.array([8]), 0.2, 1, 32, 32, [[1]]


@_crafted("iou_equals_threshold")
def _case_equal():
    # a 2 x 1 box and a 1 x 1 box inside it: IoU = 1/2 exactly on a power-of-two map; `>` must not join them at 0.5
    boxes = [(0, 0, 1, 0), (0, 0, 0, 0), (8, 8, 9, 9)]
    return np.array([boxes]), _absd(3)[None], np.array([3]), 0.5, 2, 16, 16, [[0, 1]]


@_crafted("iou_above_threshold")
def _case_above():
    boxes = [(0, 0, 1, 0), (0, 0, 0, 0), (8, 8, 9, 9)]
    return np.array([boxes]), _absd(3)[None], np.array([3]), 0.49, 2, 16, 16, [[0, 2]]


@_crafted("odd_map")
def _case_odd():
    box, absd, cnt = _random_case(3, 300, 19, 23, 3, 4)
    return box, absd, cnt, 0.4, 40, 23, 19, None


@_crafted("one_more_than_outputs")
def _case_plus1():
    box, absd, cnt = _random_case(4, 61, 24, 24, 3, 4)
    return box, absd, cnt, 0.3, 60, 24, 24, None


@_crafted("pass_through")
def _case_pass():
    box, absd, cnt = _random_case(5, 40, 24, 24, 3, 4)
    return box, absd, cnt, 0.3, 40, 24, 24, [list(range(40))]


@_crafted("threshold_zero")
def _case_zero():
    box, absd, cnt = _random_case(6, 300, 32, 32, 1, 2)
    return box, absd, cnt, 0.0, 30, 32, 32, None


@_crafted("ragged_batch")
def _case_ragged():
    box, absd, _ = _random_case(7, 300, 32, 32, 3, 4, B=3)
    return box, absd, np.array([300, 0, 131]), 0.35, 50, 32, 32, None


for _n in (255, 256, 257, 300):
    def _tile_case(n=_n):
        box, absd, cnt = _random_case(10 + n, n, 32, 32, 2, 3)
        return box, absd, cnt, 0.3, 45, 32, 32, None
    CRAFTED["tile_edge_%d" % _n] = _tile_case


@_crafted("past_one_lds_sort_8410")
def _case_8410():
    box, absd, cnt = _random_case(8, 8410, 64, 64, 4, 6)
    return box, absd, cnt, 0.5, 841, 64, 64, None


_CHANGED = {}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_lists_vs_host_routine_and_oracle(hip, name):
    """every case is the smallest list that can break one rule of the closed form (see the case's comment); exact against the host
    routine on the finished rows, the C++ oracle and the numpy restatement"""
    box, absd, cnt, thr, out, H, W, expect = CRAFTED[name]()
    changed = _check_exact(box, absd, cnt, thr, out, H, W)
    if expect is not None:
        gb, _, gc = _device(np.asarray(box, np.int32), np.asarray(absd, F32), np.asarray(cnt, np.int32), thr, out, H, W)
        for b, idx in enumerate(expect):
            assert int(gc[b]) == len(idx) and np.array_equal(gb[b, :len(idx)], np.asarray(box)[b][idx]), (name, gb[b], idx)
    _CHANGED[name] = any(changed)
    if name == "pass_through":
        assert not any(changed)


def test_clustering_changed_a_selection(hip):
    """(runs behind the crafted cases; on its own it evaluates the two smallest ones)"""
    for name in ("chain", "youngest_creator"):
        if name not in _CHANGED:
            box, absd, cnt, thr, out, H, W, _ = CRAFTED[name]()
            _CHANGED[name] = any(_check_exact(box, absd, cnt, thr, out, H, W))
    assert _CHANGED["chain"] and _CHANGED["youngest_creator"] and any(_CHANGED.values())


@pytest.mark.parametrize("thr", [0.3, 0.6])
def test_random_lists_vs_host_routine(hip, thr):
    box, absd, cnt = _random_case(21, 600, 32, 32, 3, 4, B=4)
    assert any(_check_exact(box, absd, cnt, thr, 60, 32, 32, oracle=False))


@pytest.fixture(scope="module")
def lattice48(hip):
    """the 10 * 48^2 = 23 040 best candidates per image of the tie-free constructed map of tests/test_parity_gpu.py (which shows
    that on this map the host routine equals the oracle and that clustering changes the list), and their finished rows"""
    from tests.test_parity_gpu import _lattice_corner_map
    pr = _lattice_corner_map(11, 2, 128, 128, 420, 420)
    box, absd, cnt = ops.build_samples(torch.from_numpy(pr).cuda(), 0.01, 10 * 2304, 1024, 0)
    assert int(cnt.min()) == 10 * 2304
    rows = _finish(box.cpu().numpy(), absd.cpu().numpy(), cnt.cpu().numpy(), 128, 128)
    return box, absd, cnt, rows


@pytest.mark.parametrize("thr", [0.3, 0.6])
def test_sn48_size_vs_host_routine(hip, lattice48, thr):
    box, absd, cnt, rows = lattice48
    S = 2304
    ob, oa, oc = ops.cluster_samples_device(box, absd, cnt, thr, S, 128, 128)
    hrows, hcnt = ops.cluster_samples_host(rows, cnt.cpu().numpy(), thr, S)
    assert np.array_equal(oc.cpu().numpy(), hcnt)
    got = _finish(ob.cpu().numpy(), oa.cpu().numpy(), oc.cpu().numpy(), 128, 128)
    for b in range(2):
        assert np.array_equal(got[b, :hcnt[b]], hrows[b, :hcnt[b]]), (thr, b)
        assert not np.array_equal(got[b, :S], rows[b, :S]), "clustering changed nothing"


def test_tied_scores_are_taken_in_rank_order(hip):
    """X = two overlapping boxes with ONE |d| (a run of equal scores), Y = two overlapping boxes, two singles; 6 candidates, 5
    outputs: G = 4, ratio = 1/2, X and Y give both members - the whole run is taken, so the host routine and the device hold the same
    members per score; the device's order is rank order; two calls agree bit for bit"""
    from tests.test_parity_gpu import _tie_groups_equal
    boxes = np.array([[(0, 0, 3, 3), (1, 0, 4, 3), (10, 10, 13, 13), (11, 10, 14, 13), (20, 20, 21, 21), (25, 25, 26, 26)]], np.int32)
    absd = np.array([[0.7, 0.7, 0.8, 0.9, 1.0, 1.1]], F32)
    cnt = np.array([6], np.int32)
    rows = _finish(boxes, absd, cnt, 32, 32, distinct=False)
    assert rows[0, 0, 0] == rows[0, 1, 0]
    gb, ga, gc = _device(boxes, absd, cnt, 0.3, 5, 32, 32)
    assert int(gc[0]) == 5 and np.array_equal(gb[0], boxes[0, :5]), "rank order: the first five of the six picked"
    hrows, hcnt = ops.cluster_samples_host(rows, cnt, 0.3, 5)
    assert int(hcnt[0]) == 5
    _tie_groups_equal(_finish(gb, ga, gc, 32, 32, distinct=False)[0, :5], hrows[0, :5], "tied run")
    gb2, ga2, gc2 = _device(boxes, absd, cnt, 0.3, 5, 32, 32)
    assert np.array_equal(gb, gb2) and np.array_equal(ga.view(np.uint32), ga2.view(np.uint32)) and np.array_equal(gc, gc2)


def test_results_do_not_depend_on_scheduling(hip):
    """the random case twice, and once beside a second stream that keeps the memory system busy: bit-identical outputs"""
    box, absd, cnt = _random_case(21, 600, 32, 32, 3, 4, B=4)
    first = _device(box, absd, cnt, 0.3, 60, 32, 32)
    second = _device(box, absd, cnt, 0.3, 60, 32, 32)
    side = torch.cuda.Stream()
    a, b = torch.empty(1 << 24, device="cuda"), torch.empty(1 << 24, device="cuda")
    with torch.cuda.stream(side):
        for _ in range(40):
            b.copy_(a, non_blocking=True)
    third = _device(box, absd, cnt, 0.3, 60, 32, 32)
    side.synchronize()
    for other in (second, third):
        for x, y in zip(first, other):
            assert np.array_equal(x.view(np.uint32) if x.dtype == F32 else x, y.view(np.uint32) if y.dtype == F32 else y)


def test_refusals_at_the_ops_level(hip):
    box, absd, cnt = [torch.from_numpy(a).cuda() for a in _random_case(2, 64, 16, 16, 3, 4)]
    for thr in (-0.1, 1.0):
        with pytest.raises(lib.DenetHipError, match=r"outside \[0, 1\)"):
            ops.cluster_samples_device(box.int(), absd, cnt.int(), thr, 16, 16, 16)
    with pytest.raises(lib.DenetHipError, match="output_num"):
        ops.cluster_samples_device(box.int(), absd, cnt.int(), 0.5, 0, 16, 16)


# ---- through the layer ---------------------------------------------------------------------------------------------------------

def _cluster_model(thr="0.5", B=2, IMG=128, seed=1):
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "DNS[7,24,0.01,0.1,0,%s]" % thr)
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=seed, head_desc=desc)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    return model, by_type("denet-corner"), by_type("denet-sparse"), by_type("denet-detect")


def _warmed_model(thr="0.5"):
    from tests.test_parity_gpu import _warm_corner_head
    model, dnc, dns, dnd = _cluster_model(thr)
    rng = np.random.RandomState(5)
    dconv = dnd.layers[0]
    dconv.omega.set_value(rng.normal(0, 0.05, dconv.omega.value.shape))
    _warm_corner_head(model, 2.5, 0.5)            # a busy detector: more than 576 candidates per image
    return model, dnc, dns


def test_layer_host_and_device_mode_give_the_same_lists(hip):
    """DeNet-34 skip, B = 2, 128 x 128, DNS[7,24,0.01,0.1,0,0.5]; the corner map is replaced by a tie-free constructed one of the
    layer's own size: get_samples in host mode and in device mode return identical (score, box) lists, and in device mode the
    device-to-host buffer is the sn^2 sized one"""
    from tests.test_parity_gpu import _lattice_corner_map
    model, dnc, dns, _ = _cluster_model()
    B, S = 2, dns.sample_count
    Hm, Wm = dnc.height, dnc.width
    assert dns.cluster and dns.proposal_count == 10 * S and (Hm, Wm) == (16, 16)
    dnc.corner_pr = torch.from_numpy(_lattice_corner_map(7, B, Hm, Wm, 70, 70)).cuda()
    box, absd, cnt = ops.build_samples(dnc.corner_pr, dns.corner_threshold, 10 * S, 1024, 0)
    rows = _finish(box.cpu().numpy(), absd.cpu().numpy(), cnt.cpu().numpy(), Hm, Wm)          # (asserts distinct scores)
    assert int(cnt.min()) > S, "the map must propose more candidates than RoIs"
    host = dns.get_samples(None)
    assert dns._res_host.numel() == B * 10 * S * 5 + B and not dns._dev_clustered
    with ops.cluster_device(True):
        dev = dns.get_samples(None)
        assert dns._res_host.numel() == B * S * 5 + B and dns._dev_clustered
    assert dev == host and all(0 < len(l) <= S for l in dev)
    assert host != [[(float(r[0]), tuple(float(v) for v in r[1:5])) for r in rows[b, :S]] for b in range(B)], "clustering changed nothing"
    again = dns.get_samples(None)                  # back in host mode: the wide buffers again
    assert again == host and dns._res_host.numel() == B * 10 * S * 5 + B
    assert dns.cluster and dns.proposal_count == 10 * S and dns.export_json()["nmsThreshold"] == 0.5


def test_training_step_takes_a_short_handoff_and_stays_in_parity(hip):
    """the same model on its own (warmed) corner map, device mode on: the step takes a short form of the hand-off; the clustered
    proposal equals the numpy restatement (device tie rule) of the product's own ranked 10 * sn^2 list, order included; the edited
    RoI lists equal the reference editing of that proposal; the step is in op-by-op parity with the oracle given those lists; the
    audit shows the cluster_* launches"""
    from tests.test_parity_gpu import _forced_step_check
    model, dnc, dns = _warmed_model()
    B, SC = 2, dns.sample_count
    x, metas = zoo.synthetic_batch(B, 128, seed=3)
    om = OM.OracleModel(model.export_json(), B)
    model.build_train_func("nesterov")
    random.seed(9)
    with ops.cluster_device(True), audit.KernelAudit(model) as ka:
        cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
        roi_lists = dns.sample_bbox_list
    assert dns.handoff_modes["device_edit"] + dns.handoff_modes["fast"] == 1 and dns.handoff_modes["host"] == 0, dns.handoff_modes
    for k in ("cluster_init_kernel", "cluster_pairs_kernel", "cluster_label_kernel", "cluster_select_kernel"):
        assert ka.other.count(k) == 1, (k, [s for s in ka.other if s.startswith("cluster_")])
    clustered, ccnt = dns._raw_samples
    cmap = dnc.corner_pr
    cbox, cabsd, ccn = ops.build_samples(cmap, dns.corner_threshold, 10 * SC, 1024, 0)
    ranked = ops.samples_finish_host(cbox.cpu(), cabsd.cpu(), ccn.cpu(), cmap.shape[3], cmap.shape[4]).numpy()
    lists = []
    for b in range(B):
        n = int(ccn[b])
        assert n > SC, "the detector must produce more candidates than RoIs"
        idx = closed_form_cluster(ranked[b, :n], 0.5, SC)
        assert int(ccnt[b]) == len(idx)
        assert np.array_equal(np.asarray(clustered[b, :len(idx)], F32), ranked[b, idx]), "clustered proposal of image %d" % b
        assert not np.array_equal(idx, np.arange(SC)), "clustering changed nothing"
        lists.append([(float(r[0]), tuple(float(v) for v in r[1:5])) for r in ranked[b, idx]])
    random.seed(9)
    ref_lists = OL.edit_samples(lists, metas, SC, dns.random_sample, dns.sample_gt)
    assert ref_lists == roi_lists, "RoI lists differ from the reference editing of the clustered proposal"
    ocost, _ = _forced_step_check(model, om, x, metas, 0, 0.05, 0.9, 1e-4, "nesterov", roi_lists)
    assert abs(cost - ocost) <= 1e-4 * abs(ocost), (cost, ocost)


def _params_of(model):
    """every trained tensor and running statistic of the model, in layer order"""
    out = []

    def walk(layers):
        for l in layers:
            for name in ("omega", "beta", "mean", "stdinv"):
                p = getattr(l, name, None)
                if p is not None and hasattr(p, "get_value"):
                    out.append(np.array(p.get_value(), copy=True))
            walk([s for s in getattr(l, "layers", []) if s.type_name != "initial"])
    walk(model.layers[1:])
    return out


def test_mode_off_is_untouched(hip):
    """model A steps with the mode off before, between and after device-mode steps, model B never sees the mode: costs and
    parameters stay bit-identical, and no cluster_* launch appears while the mode is off. (The device-mode steps themselves cluster
    the model's own corner maps; that their proposals equal the host routine's on these maps - no run of equal scores across a
    boundary - is asserted, not assumed: otherwise the two models would train on different lists from there on.)"""
    runs = []
    for modes in ((False, True, False, True, False), (False,) * 5):
        model, dnc, dns = _warmed_model()
        model.build_train_func("nesterov")
        random.seed(9)
        costs, proposals, launches = [], [], []
        for it, on in enumerate(modes):
            x, metas = zoo.synthetic_batch(2, 128, seed=3 + it)
            with ops.cluster_device(on), audit.KernelAudit(model) as ka:
                # (a small learning rate: the warmed detector stays busy over the five steps)
                cost, _ = model.train_step(x, metas, 0, it, 1e-5, [0.9], 1e-4)
                dns.sample_bbox_list                     # (resolves the step's lazy host share)
            costs.append(cost)
            assert dns._raw_samples is not None, "step %d: the detector proposed nothing" % it
            if on:
                P = dns.proposal_count
                assert int(dns._stage_dev[2 * P * 5:].min()) > dns.sample_count, "step %d: nothing to cluster" % it
            proposals.append((np.array(dns._raw_samples[0], copy=True), np.array(dns._raw_samples[1], copy=True)))
            launches.append(sum(s.startswith("cluster_") for s in ka.other))
        runs.append((costs, proposals, launches, _params_of(model), dict(dns.handoff_modes)))
    (ca, pa, la, wa, ha), (cb, pb, lb, wb, hb) = runs
    assert la == [0, 4, 0, 4, 0] and lb == [0] * 5
    assert ha["host"] == 3 and ha["device_edit"] + ha["fast"] == 2 and hb["host"] == 5
    for it in range(5):
        n = pa[it][1]
        assert np.array_equal(n, pb[it][1]) and all(np.array_equal(pa[it][0][b, :n[b]], pb[it][0][b, :n[b]]) for b in range(2)), \
            "step %d: the device and the host clustered the model's own map differently (a tied run on a boundary)" % it
    assert ca == cb, (ca, cb)
    assert len(wa) == len(wb) > 0 and all(np.array_equal(a, b) for a, b in zip(wa, wb))


def test_layer_with_a_threshold_outside_the_closed_form_uses_the_host_routine(hip):
    from tests.test_parity_gpu import _lattice_corner_map
    model, dnc, dns, _ = _cluster_model("-0.1")
    assert dns.cluster and dns.nms_threshold == -0.1
    dnc.corner_pr = torch.from_numpy(_lattice_corner_map(7, 2, dnc.height, dnc.width, 70, 70)).cuda()
    host = dns.get_samples(None)
    calls = []
    real = ops.cluster_samples_device
    ops.cluster_samples_device = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        with ops.cluster_device(True):
            assert not dns._cluster_on_device()
            dev = dns.get_samples(None)
    finally:
        ops.cluster_samples_device = real
    assert not calls and dev == host and dns._res_host.numel() == 2 * 10 * dns.sample_count * 5 + 2


# ---- model-predict -------------------------------------------------------------------------------------------------------------

def test_model_predict_device_cluster(hip, tmp_path):
    """`model-predict --device-cluster` on the tiny detection fixture of tests/test_pipeline_gpu.py: it runs through the device
    clustering and writes the result files of the run without the flag. The fixture's proposals are checked for runs of equal
    scores FIRST (head calibrations are tried in a fixed order until one is tie-free; none: the test fails) and compared only
    then"""
    from denet_amd import dataset
    from denet_amd.model import model_cnn, predict
    from tests import test_pipeline_gpu as TP
    root = str(tmp_path / "data")
    os.makedirs(root)
    TP.S.build_dataset(root)
    src = os.path.join(root, "voc")
    ext = "voc,2007-test,2012-test,crop=128,scale=128"
    train = dataset.load(src, "voc,2007-trainval,2012-trainval,crop=128,crop_mode=denet,check_center,augment_photo", True, 1)
    test = dataset.load(src, ext, False, 1, train.class_labels)
    B = 2
    desc = zoo.DENET34_SKIP_DESC.replace("DNS[7,24,0.01,0.1]", "DNS[7,24,0.01,0.1,0,0.5]")
    model = zoo.denet34(B, "skip", 128, class_num=train.get_class_num(), seed=1, head_desc=desc)
    model.class_labels = train.class_labels
    dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
    dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
    S = dns.sample_count
    batches = TP._batches(test, B)
    for seed in range(6, 12):
        TP._calibrate_heads(model, batches, np.random.RandomState(seed))
        tie_free, clustered = True, 0
        for x, _, n_real in batches:
            model.forward(x, None, train=False)
            box, absd, cnt = ops.build_samples(dnc.corner_pr, TP.PARAMS["cornerThreshold"], 10 * S, 1024, 0)
            rows = ops.samples_finish_host(box.cpu(), absd.cpu(), cnt.cpu(), dnc.height, dnc.width).numpy()
            for b in range(B):
                n = int(cnt[b])
                tie_free &= len(np.unique(rows[b, :n, 0])) == n
                clustered += int(n > S)
        if tie_free:
            break
    assert tie_free, "no calibration of the fixture's heads gave proposals without equal scores"
    assert clustered > 0, "no image of the fixture proposes more candidates than RoIs: the clustering is not exercised"
    mdl = str(tmp_path / "m.mdl.gz")
    model_cnn.save_to_file(model, mdl)
    calls = []
    real, mode_before = ops.cluster_samples_device, ops.CLUSTER_DEVICE
    assert not mode_before, "this test compares with a run in the product default: unset DENET_CLUSTER_DEVICE"
    ops.cluster_samples_device = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        outs = {}
        for flag in ([], ["--device-cluster"]):
            out = str(tmp_path / ("out" + "_dev" * bool(flag)))
            assert predict.main(["--model", mdl, "--input", src, "--extension", ext, "--batch-size", str(B), "--predict-mode", "detect,voc",
                                 "--results", os.path.join(out, "res"), "--params", TP.PARAMS_STR] + flag) == 0
            outs[bool(flag)] = (out, len(calls))
    finally:
        ops.cluster_samples_device = real
    assert outs[False][1] == 0 and outs[True][1] >= len(batches), "the flag did not route the proposal through the device clustering"
    assert ops.CLUSTER_DEVICE is mode_before, "the driver must restore the mode"
    files = sorted(os.listdir(outs[False][0]))
    assert files == sorted(os.listdir(outs[True][0])) and "detections.json" in files
    for f in files:
        assert open(os.path.join(outs[False][0], f), "rb").read() == open(os.path.join(outs[True][0], f), "rb").read(), f
