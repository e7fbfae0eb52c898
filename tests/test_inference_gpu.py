"""Inference tail: class/fitness/box decode + per-class NMS of the detection head against the oracle
(oracle/layers.py:detect_outputs restates denet_detect.py:76-100,330-349; oracle/build_samples.cc restates
build_detections_nms of denet_detect.cc:99-173). Membership, class, order and boxes are exact on the same decoded
arrays; the decode itself (exp/log) is floating point: 1e-5 relative."""
import ctypes

import numpy as np
import pytest
import torch

from denet_amd import ops
from denet_amd.model import zoo
from oracle import layers as OL
from oracle import model as OM

pytestmark = pytest.mark.gpu


def _oracle_nms(det_pr, fitness, bbox, counts, B, sn, C1, pr_thr, nms_thr, soft):
    """arrays in the product's [B*S, C1] / [B*S, 4] layout -> list[B] of (pr, cls, box) rows from the oracle"""
    S = sn * sn
    det = np.ascontiguousarray(det_pr.reshape(B, sn, sn, C1).transpose(0, 3, 1, 2), dtype=np.float32)
    fit = np.ascontiguousarray(fitness.reshape(B, sn, sn, C1).transpose(0, 3, 1, 2), dtype=np.float32)
    bx = np.ascontiguousarray(bbox.reshape(B, sn, sn, 4), dtype=np.float32)
    num = np.ascontiguousarray(counts, dtype=np.int32)
    max_out = S * (C1 - 1)
    out = np.zeros((B, max_out, 6), np.float32)
    cnt = np.zeros(B, np.int32)
    f = OM.oracle_lib().oracle_build_detections_nms
    f.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    f(pr_thr, nms_thr, int(soft), det.ctypes.data, fit.ctypes.data, bx.ctypes.data, num.ctypes.data, B, C1, sn, max_out,
      out.ctypes.data, cnt.ctypes.data)
    return [out[b, :cnt[b]] for b in range(B)]


def _clustered_boxes(rng, B, S):
    centres = rng.rand(B, 6, 2)
    pick = rng.randint(0, 6, (B, S))
    c = np.take_along_axis(centres, pick[..., None].repeat(2, -1), 1) + rng.normal(0, 0.02, (B, S, 2))
    wh = 0.2 + 0.05 * rng.rand(B, S, 2)
    return np.concatenate([c - wh / 2, c + wh / 2], -1).astype(np.float32)


def _product_lists(keep, fit_h, box_h, B, S):
    res = []
    for b in range(B):
        cls_idx, roi_idx = np.nonzero(keep[b])
        rows = b * S + roi_idx
        res.append(np.concatenate([np.exp(fit_h[rows, cls_idx])[:, None], cls_idx[:, None].astype(np.float32),
                                   box_h[rows]], 1).astype(np.float32).reshape(-1, 6))
    return res


@pytest.mark.parametrize("jointfit", [0, 1])
@pytest.mark.parametrize("sn", [4, 24])
def test_detect_decode_and_nms_vs_oracle(hip, jointfit, sn):
    rng = np.random.RandomState(10 + sn + jointfit)
    B, C, S = 3, 7, sn * sn
    s0 = C * 5 + 1 if jointfit else C + 1
    CP = (s0 + 4 + 31) // 32 * 32
    t0 = 0.5
    logits = np.zeros((B * S, CP), np.float32)
    logits[:, :s0] = rng.normal(0, 2.5, (B * S, s0))
    logits[:, s0:s0 + 4] = rng.normal(0, 0.2, (B * S, 4))
    roi = _clustered_boxes(rng, B, S).reshape(B * S, 4)
    counts = np.array([S, S // 3, 0], np.int32)
    det_pr, fitness, bbox = ops.detect_decode(torch.from_numpy(logits).cuda(), torch.from_numpy(roi).cuda(), C, jointfit, 4, t0)
    det_h, fit_h, box_h = det_pr.cpu().numpy(), fitness.cpu().numpy(), bbox.cpu().numpy()
    # decode against the numpy restatement (NCHW like the reference)
    out_nchw = logits[:, :s0 + 4].reshape(B, sn, sn, s0 + 4).transpose(0, 3, 1, 2)
    o_det, o_fit, o_box = OL.detect_outputs(out_nchw, roi.reshape(B, sn, sn, 4), C, bool(jointfit), t0)
    np.testing.assert_allclose(det_h.reshape(B, sn, sn, C + 1).transpose(0, 3, 1, 2), o_det, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(fit_h.reshape(B, sn, sn, C + 1).transpose(0, 3, 1, 2), o_fit, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(box_h.reshape(B, sn, sn, 4), o_box, rtol=1e-5, atol=1e-6)
    # NMS: exact against the oracle on the SAME decoded arrays
    for pr_thr, nms_thr in ((0.1, 0.5), (0.3, 0.3), (0.1, 1.0), (0.2, 0.0)):
        keep = ops.detect_nms(det_pr, fitness, bbox, torch.from_numpy(counts).cuda(), B, S, C, pr_thr, nms_thr).cpu().numpy()
        got = _product_lists(keep, fit_h, box_h, B, S)
        ref = _oracle_nms(det_h, fit_h, box_h, counts, B, sn, C + 1, pr_thr, nms_thr, False)
        for b in range(B):
            assert got[b].shape == ref[b].shape, (b, pr_thr, nms_thr, got[b].shape, ref[b].shape)
            assert np.array_equal(got[b][:, 1:], ref[b][:, 1:])
            np.testing.assert_allclose(got[b][:, 0], ref[b][:, 0], rtol=2e-6)
        if 0 < nms_thr < 1:
            assert 0 < sum(len(g) for g in got) < int((det_h[:, :C] >= np.log(np.float32(pr_thr))).sum()), "NMS did nothing"
    assert len(got[2]) == 0


@pytest.mark.parametrize("nreg", [4, 0])
def test_detect_decode_independent_fitness_vs_oracle(hip, nreg):
    """independent fitness head at inference (denet_detect.py:396-401): fitness += log E[val]"""
    rng = np.random.RandomState(21 + nreg)
    B, C, sn = 2, 7, 6
    S, s0, nfit, t0 = sn * sn, C + 1, 6, 0.5
    CP = 32
    logits = np.zeros((B * S, CP), np.float32)
    logits[:, :s0] = rng.normal(0, 2.0, (B * S, s0))
    logits[:, s0:s0 + nreg] = rng.normal(0, 0.2, (B * S, nreg))
    logits[:, s0 + nreg:s0 + nreg + nfit] = rng.normal(0, 1.5, (B * S, nfit))
    roi = _clustered_boxes(rng, B, S).reshape(B * S, 4)
    det_pr, fitness, bbox = ops.detect_decode(torch.from_numpy(logits).cuda(), torch.from_numpy(roi).cuda(), C, 0, nreg, t0,
                                              nfit=nfit)
    out_nchw = logits[:, :s0 + nreg + nfit].reshape(B, sn, sn, -1).transpose(0, 3, 1, 2)
    o_det, o_fit, o_box = OL.detect_outputs(out_nchw, roi.reshape(B, sn, sn, 4), C, False, t0, use_bbox_reg=nreg == 4,
                                            nfit=nfit)
    np.testing.assert_allclose(det_pr.cpu().numpy().reshape(B, sn, sn, C + 1).transpose(0, 3, 1, 2), o_det, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(fitness.cpu().numpy().reshape(B, sn, sn, C + 1).transpose(0, 3, 1, 2), o_fit, rtol=1e-5, atol=4e-6)
    assert float(np.abs(o_fit - o_det).max()) > 0.1      # the fitness term is really there


def test_soft_nms_host_vs_oracle(hip):
    rng = np.random.RandomState(3)
    B, sn, C = 1, 12, 1
    S = sn * sn
    box = _clustered_boxes(rng, B, S).reshape(S, 4)
    fit = np.log(rng.uniform(0.02, 1.0, (S, 2))).astype(np.float32)
    counts = np.array([S - 5], np.int32)
    for nms_thr in (0.3, 0.6):
        ref = _oracle_nms(fit, fit, box, counts, B, sn, C + 1, 0.05, nms_thr, True)[0]
        cand = np.arange(counts[0])[fit[:counts[0], 0] >= np.log(np.float32(0.05))]
        order, score = ops.soft_nms_host(fit[cand, 0], box[cand], nms_thr)
        assert len(order) == len(ref) and 0 < len(ref) < len(cand)
        assert np.array_equal(box[cand[order]], ref[:, 2:])
        np.testing.assert_allclose(np.exp(score), ref[:, 0], rtol=2e-6)


@pytest.mark.parametrize("B,sn,C,nms_thr", [(3, 12, 5, 0.4), (2, 24, 80, 0.5), (1, 48, 3, 0.6), (2, 12, 4, 1.5), (2, 12, 4, 0.3)])
def test_soft_nms_device_vs_host_and_oracle(hip, B, sn, C, nms_thr):
    """denet_soft_nms_batch (one wave per (class, image)) against the host call and the C++ oracle: the same detections in the
    same order with the same scores, bit for bit - incl. exact score ties (duplicated candidates), images without candidates,
    a threshold outside (0, 1) (no suppression: list order) and 48x48 RoIs (36 candidates per lane)"""
    rng = np.random.RandomState(11 + sn + C)
    S = sn * sn
    box = _clustered_boxes(rng, B, S).reshape(B * S, 4)
    fit = np.log(rng.uniform(0.005, 1.0, (B * S, C + 1))).astype(np.float32)
    det = (fit + rng.normal(0, 0.3, fit.shape)).astype(np.float32)
    # exact ties: copies of a candidate's score (and of a whole candidate) later in the list
    fit[7::13, 0] = fit[5, 0]
    box[9] = box[5]
    fit[9, :] = fit[5, :]
    det[9, :] = det[5, :]
    counts = np.array([S - 3 * b for b in range(B)], np.int32)
    if B > 1:
        det[S:S + counts[1], C - 1] = -50.0          # an (image, class) pair without candidates
    if nms_thr == 0.3:
        counts[0] = 0                                  # an image without RoIs
    pr_thr = 0.05
    t = lambda a: torch.from_numpy(a).cuda()
    sc_d, cls_d, row_d, per_d = ops.soft_nms_batch(t(det), t(fit), t(box), t(counts), B, S, C, pr_thr, nms_thr)
    sc_h, cls_h, row_h, per_h = ops.soft_nms_batch_host(det, fit, box, counts, B, S, C, pr_thr, nms_thr)
    assert np.array_equal(per_d, per_h) and per_h.sum() > 0
    assert np.array_equal(cls_d, cls_h) and np.array_equal(row_d, row_h)
    assert np.array_equal(sc_d.view(np.uint32), sc_h.view(np.uint32))
    ref = _oracle_nms(det, fit, box, counts, B, sn, C + 1, pr_thr, nms_thr, True)
    lo = 0
    for b in range(B):
        hi = lo + int(per_d[b])
        assert hi - lo == len(ref[b])
        assert np.array_equal(box[row_d[lo:hi]], ref[b][:, 2:]) and np.array_equal(cls_d[lo:hi], ref[b][:, 1].astype(np.int32))
        np.testing.assert_allclose(np.exp(sc_d[lo:hi]), ref[b][:, 0], rtol=2e-6)
        lo = hi


@pytest.mark.parametrize("soft", [0, 1, 2])
def test_denet34_get_detections_vs_oracle(hip, soft, monkeypatch):
    """whole inference path on DeNet-34 skip (128x128): test-mode forward -> corner detector RoIs -> head -> NMS
    (soft = 1: Gaussian soft-NMS as a batch of 2 runs it, on host copies; 2: forced onto the device kernel)"""
    if soft == 2:
        monkeypatch.setenv("DENET_SOFT_NMS_HOST", "0")
        soft = 1
    from tests.test_parity_gpu import _warm_corner_head, rel_close
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=20, seed=1)
    rng = np.random.RandomState(5)
    dnd = model.layers[40]
    dconv = dnd.layers[0]
    dconv.omega.set_value(rng.normal(0, 0.3, dconv.omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=2)
    params = {"prThreshold": 0.08, "nmsThreshold": 0.5, "cornerThreshold": 0.02, "useSoftNMS": soft}
    # test-mode BN on untrained running statistics blows the activations up: rescale the head filters so that the
    # class logits are O(1) and the box regression outputs O(0.1), like a trained head
    dnd.get_detections(model, x, metas, params)
    raw = dnd.conv.output.data.float().cpu().numpy().reshape(-1, dnd.conv.kp)
    s0 = dnd.s0
    w = dconv.omega.get_value().copy()
    w[:s0] *= 2.0 / raw[:, :s0].std()
    w[s0:s0 + 4] *= 0.2 / raw[:, s0:s0 + 4].std()
    dconv.omega.set_value(w)
    _, total = check_detections_vs_oracle(model, x, metas, params)
    assert total > 0, "no detections: the test exercises nothing"


def _assert_proposal_of(corner_pr, got_lists, threshold, dns):
    """the product's RoI lists are the oracle's proposal on the product's corner map (exact; tie groups compared as sets)"""
    lists = OM.oracle_build_samples(corner_pr, threshold, dns.sample_num, 1024, 0)
    assert len(got_lists) == len(lists)
    for g, r in zip(got_lists, lists):        # order inside a group of exactly equal scores is unspecified (std::partial_sort)
        assert [p for p, _ in g] == [p for p, _ in r]
        i = 0
        while i < len(r):
            j = i
            while j + 1 < len(r) and r[j + 1][0] == r[i][0]:
                j += 1
            if not (j + 1 == len(r) and len(r) == dns.sample_count):   # a tie group cut by the top-K boundary
                assert sorted(bx for _, bx in g[i:j + 1]) == sorted(bx for _, bx in r[i:j + 1])
            i = j + 1


def check_detections_vs_oracle(model, x, metas, params, om=None):
    """one batch through the product's get_detections against the oracle, stage by stage (denet_detect.py:316-424):
    RoI proposal exact on the product's corner map (tie groups as sets), test-mode forward of oracle/model.py on the same RoIs
    (corner map 1e-3, decoded class / box arrays 1e-3), threshold + NMS exact on the product's decoded arrays. Returns
    (results, number of detections). `om`: an OracleModel of the same weights (built from model.export_json() when None)."""
    from tests.test_parity_gpu import rel_close
    B = model.batch_size
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    dnd, dns, cl = by_type("denet-detect"), by_type("denet-sparse"), by_type("denet-corner")
    soft = int(params.get("useSoftNMS", 0))
    results = dnd.get_detections(model, x, metas, params)
    # RoI proposal: exact on the product's corner map
    lists = dns.sample_bbox_list
    _assert_proposal_of(cl.corner_pr.cpu().numpy(), lists, params["cornerThreshold"], dns)
    # head: oracle forward in test mode on the same RoIs
    if om is None:
        om = OM.OracleModel(model.export_json(), B)
    om.forward(x, None, train=False, sample_override=lists)
    rel_close(cl.corner_pr.cpu().numpy(), om.corner_pr, 1e-3, "corner_pr (test mode)")
    det_pr, fitness, bbox, counts = dnd.last_outputs
    assert counts.tolist() == [len(l) for l in lists]
    sn = dns.sample_num
    t0 = dnd._thresholds()[0]
    C = dnd.class_num
    o_det, o_fit, o_box = OL.detect_outputs(om.detect_out.v, om.sample_bbox, C, bool(dnd.use_jointfit), t0)
    C1 = C + 1
    valid = (np.arange(sn * sn)[None] < counts[:, None]).reshape(B, 1, sn, sn)
    d = det_pr.cpu().numpy().reshape(B, sn, sn, C1).transpose(0, 3, 1, 2)
    np.testing.assert_allclose(np.where(valid, d, 0), np.where(valid, o_det, 0), rtol=1e-3, atol=1e-3)
    bx = bbox.cpu().numpy().reshape(B, sn, sn, 4)
    v4 = valid.reshape(B, sn, sn, 1)
    np.testing.assert_allclose(np.where(v4, bx, 0), np.where(v4, o_box, 0), rtol=1e-3, atol=1e-4)
    # threshold + NMS: exact on the product's decoded arrays
    ref = _oracle_nms(det_pr.cpu().numpy(), fitness.cpu().numpy(), bbox.cpu().numpy(), counts, B, sn, C1,
                      params["prThreshold"], params["nmsThreshold"], soft)
    total = 0
    for b in range(B):
        dets = results[b]["detections"]
        assert results[b]["meta"] is metas[b]
        assert len(dets) == len(ref[b])
        total += len(dets)
        for (pr, cls, box), r in zip(dets, ref[b]):
            assert cls == int(r[1]) and np.array_equal(np.array(box, np.float32), r[2:])
            assert abs(pr - r[0]) <= 2e-6 * r[0]
    return results, total


def test_inference_bn_folding_matches_unfolded(hip):
    """inference folds every batch norm that sits directly behind a convolution into that convolution's filters
    (denet_bn_fold) and moves ReLU / residual add into its epilogue (denet_conv_fwd_act): same activations as the
    layer-by-layer test-mode pass to rounding, for top-level pairs and inside the residual blocks"""
    from denet_amd import ops
    from tests.test_parity_gpu import _warm_corner_head
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=20, seed=1)
    rng = np.random.RandomState(5)
    _warm_corner_head(model, 4.0, 0.3)
    # non-trivial running statistics and affine parameters so that the fold has something to get wrong
    for l in model_cnn_walk(model):
        if l.type_name in ("batchnorm", "batchnorm-relu"):
            C = l.mean.value.shape[0]
            l.mean.set_value(rng.normal(0, 0.2, C).astype(np.float32))
            l.stdinv.set_value(rng.uniform(0.7, 1.4, C).astype(np.float32))
            l.omega.set_value(rng.uniform(0.5, 1.5, C).astype(np.float32))
            l.beta.set_value(rng.normal(0, 0.2, C).astype(np.float32))
    x, _ = zoo.synthetic_batch(B, IMG, seed=2)
    outs = []
    for fold in (False, True):
        with ops.infer_fold(fold):
            for l in model_cnn_walk(model):
                l.__dict__.pop("_plan", None)
            model.forward(x, None, train=False)
            dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
            res = [l for l in model.layers if l.type_name == "resnet"]
            outs.append([ops.nhwc_to_nchw(a.output.data, a.output_shape[1]).cpu().numpy() for a in (res[0], res[7], res[-1])] +
                        [dnc.corner_pr.cpu().numpy(), ops.nhwc_to_nchw(model.layers[2].output.data, 64).cpu().numpy()])
    for a, b in zip(*outs):
        scale = float(np.abs(a).max())
        assert float(np.abs(a - b).max()) <= 2e-5 * scale + 1e-6, (float(np.abs(a - b).max()), scale)
    assert float(np.abs(outs[0][0]).max()) > 0


COVERAGE_FLOOR = 0.99          # measured: 18 430 of 18 432 RoIs (0.9999)


def test_inference_forward_at_the_batch_of_the_tuned_file(hip):
    """B = 32, 512x512 - the geometry at which the committed tuned file decides the algorithms, including its MODE 3 entries (the
    inference forward pass alone: the tile-parallel fused F(4x4) kernel, csrc/wino4t.hip, on the 128 / 256-channel layers, where
    training keeps the component-walk kernel) and algorithm 44 on the 64-channel stage. The test-mode forward with those decisions
    against the same forward with the tile-parallel kernel switched off (DENET_WINO4T = 0: fused F(2x2) / component-walk F(4x4)
    kernels): corner map and class logits agree to 2e-4 of their scale, the per-layer audit shows the kernels really differ."""
    from denet_amd import ops
    from denet_amd.model import audit
    from tests.test_parity_gpu import _warm_corner_head
    B = 32
    model = zoo.denet34(B, "skip", 512, class_num=80, seed=1)
    _warm_corner_head(model, 4.0, 0.3)
    rng = np.random.RandomState(3)
    dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
    dnc = [l for l in model.layers if l.type_name == "denet-corner"][0]
    dnd.layers[0].omega.set_value(rng.normal(0, 0.02, dnd.layers[0].omega.value.shape))
    x, metas = zoo.synthetic_batch(B, 512, 80, seed=1)
    xd = torch.from_numpy(x).cuda()
    outs, kernels = [], []
    with ops.algorithms() as wino:
        for on in (True, False):
            if not on:
                for k in [k for k, v in wino.items() if v == ops.FUSED4]:
                    del wino[k]                            # (what load_tuned does with entries the switches exclude: decided afresh)
            with ops.switches(WINO4T=ops.WINO4T if on else 0):
                for l in model_cnn_walk(model):
                    l.__dict__.pop("_plan", None)
                with audit.KernelAudit(model) as ka:
                    model.forward(xd, None, train=False)
                    torch.cuda.synchronize()
                kernels.append({g: tuple(e["fwd"]) for g, e in ka.summary().items()})
                dns = [l for l in model.layers if l.type_name == "denet-sparse"][0]
                outs.append((dnc.corner_pr.cpu().numpy().copy(), dnc.conv.output.data.float().cpu().numpy().copy(),
                             dnd.conv.output.data.float().cpu().numpy().copy(), [list(l) for l in dns.sample_bbox_list]))
    used = [g for g, k in kernels[0].items() if any(n.startswith("wino4t_kernel") for n in k)]
    assert len(used) >= 5, kernels[0]                      # the 64-channel stage + the four mode-3 geometries
    assert not any(n.startswith("wino4t_kernel") for k in kernels[1].values() for n in k)
    # corner map and the corner layer's convolution output (corner logits + the sampling features): everything the backbone feeds
    # the detector with; the head's logits row by row only where both runs proposed the same RoI lists (the proposal ranks by
    # scores that differ in the last bits between the two kernel sets)
    for a, b in zip(outs[0][:2], outs[1][:2]):
        scale = float(np.abs(b).max())
        assert float(np.abs(a - b).max()) <= 2e-4 * scale, (float(np.abs(a - b).max()), scale)
    if outs[0][3] == outs[1][3]:
        a, b = outs[0][2], outs[1][2]
        assert float(np.abs(a - b).max()) <= 2e-4 * float(np.abs(b).max())
    # whatever the lists: a head row depends on its RoI's sampled features alone, so every RoI that both runs proposed for an
    # image has its row compared; the intersection must cover most of the proposal (measured on MI355X: see COVERAGE_FLOOR)
    S = dnd.sample_num * dnd.sample_num
    ha, hb = outs[0][2].reshape(B * S, -1), outs[1][2].reshape(B * S, -1)
    ia, ib, n_all = [], [], 0
    for img, (la, lb) in enumerate(zip(outs[0][3], outs[1][3])):
        pos_b = {tuple(bx): j for j, (_, bx) in enumerate(lb)}
        for j, (_, bx) in enumerate(la):
            if tuple(bx) in pos_b:
                ia.append(img * S + j)
                ib.append(img * S + pos_b[tuple(bx)])
        n_all += max(len(la), len(lb))
    coverage = len(ia) / max(1, n_all)
    print("B = 32 inference, RoIs proposed by both kernel sets: %d of %d (%.4f)" % (len(ia), n_all, coverage))
    assert n_all > 0 and coverage >= COVERAGE_FLOOR, (len(ia), n_all)
    a, b = ha[ia], hb[ib]
    assert float(np.abs(a - b).max()) <= 2e-4 * float(np.abs(b).max()), (float(np.abs(a - b).max()), float(np.abs(b).max()))


def model_cnn_walk(model):
    from denet_amd.model.model_cnn import walk_layers
    return walk_layers(model.layers)


def _mode3_geometries(model):
    """the 3x3 stride-1 geometries of `model` with 128 or 256 reduction channels that the tile-parallel F(4x4) kernel covers"""
    from denet_amd.model import audit
    out = set()
    for _, l in audit.conv_layers(model):
        g, _ = audit.layer_geometry(l)
        if g[5:10] == (3, 3, 3, 1, 1) and g[3] in (128, 256) and ops.conv_wino4t_ok(0, g):
            out.add(g)
    return sorted(out)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_inference_after_training_steps_matches_a_fresh_model(hip, k):
    """inference -> k training steps -> inference on one model gives bit for bit what a fresh model loaded from the trained
    model's export_json() gives (same kernels on the same weights). Mode-3 entries (the inference forward pass on the
    tile-parallel fused F(4x4) kernel, csrc/wino4t.hip, where training runs another algorithm) are injected for the 128 / 256-channel
    3x3 geometries of a B = 2, 128x128 DeNet-34: the situation of the B = 32 pass of the tuned file at a small size. k = 1 is the
    case where the filters wino_prefetch_filters transformed at the start of the training step for the algorithm the previous
    INFERENCE pass ran (from the unfolded, pre-update weights) were left unused by the training pass and then taken by the next
    inference pass."""
    from denet_amd.model import audit, model_cnn
    from tests.test_parity_gpu import _warm_corner_head
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=20, seed=1)
    rng = np.random.RandomState(5)
    dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
    dnd.layers[0].omega.set_value(rng.normal(0, 0.05, dnd.layers[0].omega.value.shape))
    _warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, 20, seed=2)
    xd = torch.from_numpy(x).cuda()
    geoms = _mode3_geometries(model)
    assert len(geoms) >= 2, geoms

    def infer(m):
        m.forward(xd, None, train=False)
        d = [l for l in m.layers if l.type_name == "denet-detect"][0]
        c = [l for l in m.layers if l.type_name == "denet-corner"][0]
        s = [l for l in m.layers if l.type_name == "denet-sparse"][0]
        return c.corner_pr.clone(), d.conv.output.data.clone(), [list(l) for l in s.sample_bbox_list]

    with ops.algorithms() as wino:
        for g in geoms:
            wino[(3, g)] = ops.FUSED4
        model.build_train_func("nesterov")
        infer(model)
        assert sum(l._cache().get("fwd_tile") == ops.FUSED4 for _, l in audit.conv_layers(model)) >= len(geoms), \
            "the inference pass did not run the injected mode-3 entries"
        for it in range(k):
            cost, _ = model.train_step(x, metas, 0, it, 0.01, [0.9], 1e-4)
            assert np.isfinite(cost), cost
        got = infer(model)
        fresh = model_cnn.load_from_json(model.export_json(), B)
        want = infer(fresh)
    assert got[2] == want[2], "RoI lists differ"
    assert any(len(l) for l in want[2])
    assert torch.equal(got[0], want[0]), "corner map: %.3e" % float((got[0] - want[0]).abs().max())
    assert torch.equal(got[1], want[1]), "head outputs: %.3e" % float((got[1] - want[1]).abs().max())


@pytest.mark.parametrize("wino4t", [1, 2])
def test_wino4t_switch_routes_the_committed_inference_entries(hip, monkeypatch, wino4t):
    """the committed tuned file reloaded into a cleared decision table under DENET_WINO4T = 1 (forward passes only) / 2 (data
    gradients only): the inference forward pass at a mode-3 geometry runs the tile-parallel kernel exactly when the forward bit is
    set; the data gradient of the 64-channel stage keeps it exactly when the data-gradient bit is set"""
    ops._load_tuned_once()
    committed = dict(ops._WINO)
    m3 = sorted(g for (m, g), t in committed.items() if m == 3 and t == ops.FUSED4)
    d4 = sorted(g for (m, g), t in committed.items() if m == 1 and t == ops.FUSED4)
    assert m3 and d4
    g = min(m3, key=lambda g: g[0] * g[1] * g[2] * (g[3] + g[4]))
    gd = min(d4, key=lambda g: g[0] * g[1] * g[2] * (g[3] + g[4]))
    monkeypatch.setattr(ops, "WINO4T", wino4t)
    gen = torch.Generator().manual_seed(wino4t)
    with ops.algorithms(table={}):
        ops.load_tuned(ops.TUNE_CACHE)
        assert ((3, g) in ops._WINO) == bool(wino4t & 1) and ((1, gd) in ops._WINO) == bool(wino4t & 2)
        N, H, W, C, K = g[:5]
        x = torch.randn(N, H, W, C, generator=gen).cuda()
        w = (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda()
        icache = {}
        ops.conv_fwd(x, w, bias=torch.zeros(K, device="cuda"), stride=1, pad=1, relu=True, cache=icache)
        assert (icache["fwd_tile"] == ops.FUSED4) == bool(wino4t & 1), (wino4t, icache["fwd_tile"])
        assert icache["fwd_tile"] == (ops.FUSED4 if wino4t & 1 else committed[(0, g)])
        del x
        N, H, W, C, K = gd[:5]
        dy = torch.randn(N, H, W, K, generator=gen).cuda()
        w = (torch.randn(K, 3, 3, C, generator=gen) * (2.0 / (9 * C)) ** 0.5).cuda()
        dcache = {"train": True}
        ops.conv_dgrad(dy, w, (N, H, W, C), stride=1, pad=1, cache=dcache)
        assert (dcache["dgrad_tile"] == ops.FUSED4) == bool(wino4t & 2), (wino4t, dcache["dgrad_tile"])


def _chunk_nchw(t, B, sl, shape):
    """the images `sl` of a product activation (rows image-major, channels last and possibly padded) in the oracle's NCHW shape"""
    v = t.reshape(B, -1, t.shape[-1])[sl, :, :shape[1]]
    return v.permute(0, 2, 1).reshape(shape).cpu().numpy()


def test_inference_at_the_batch_of_the_tuned_file_vs_fp64(hip):
    """get_detections at B = 32, 512x512 - the geometry of the committed tuned file's MODE 3 entries (the tile-parallel fused F(4x4)
    kernel on the 128 / 256-channel 3x3 layers of the inference pass alone) - judged by the fp64 arbiter like
    test_denet101_wide_train_step_vs_oracle[512]: oracle/model.py in float64 is the reference, the product and the fp32 oracle are
    both measured against it, per layer and on the corner map, in both _err_stats clauses (1e-3 against fp64; no farther from
    fp64 than max(1e-3, 1.5 x the fp32 oracle)). Test mode treats every image alone, so the oracle runs in chunks of 8 images on
    the product's RoI lists. The batch norms carry the batch statistics of one training-mode forward pass, perturbed by a few
    percent (activations O(1), not zeros or overflow). RoI lists: the oracle's proposal on the product's corner map; class
    log-probabilities and boxes within 1e-3 of fp64; threshold + NMS exact on the product's decoded arrays."""
    import random
    from denet_amd.model import audit
    from denet_amd.model.model_cnn import walk_layers
    from tests.test_parity_gpu import _err_stats, _warm_corner_head
    B, CH, IMG = 32, 8, 512
    model = zoo.denet34(B, "skip", IMG, class_num=80, seed=1)
    _warm_corner_head(model, 4.0, 0.3)
    rng = np.random.RandomState(3)
    by_type = lambda t: [l for l in model.layers if l.type_name == t][0]
    dnd, dns, dnc = by_type("denet-detect"), by_type("denet-sparse"), by_type("denet-corner")
    dnd.layers[0].omega.set_value(rng.normal(0, 0.02, dnd.layers[0].omega.value.shape))
    x, metas = zoo.synthetic_batch(B, IMG, 80, seed=1)
    ops._load_tuned_once()
    assert audit.decisions_cover(model) == []
    m3 = {g for (m, g), t in ops._WINO.items() if m == 3 and t == ops.FUSED4}
    assert len(m3) == 4, sorted(m3)
    # running statistics: the batch statistics of one training-mode pass over the same images, perturbed by up to 5 %
    model.build_train_func("nesterov")
    random.seed(4)
    ctx = model.forward(x, metas, train=True)
    model.backward(ctx)
    torch.cuda.synchronize()
    bns = [l for l in walk_layers(model.layers) if l.type_name in ("batchnorm", "batchnorm-relu") and l.enabled]
    assert len(bns) > 30
    for l in bns:
        assert l._save is not None, l.layer_index
        sm, si = l._save[0].double().cpu().numpy(), l._save[1].double().cpu().numpy()
        C = sm.shape[0]
        l.mean.set_value(sm + 0.05 / si * rng.uniform(-1, 1, C))
        l.stdinv.set_value(si * (1 + 0.05 * rng.uniform(-1, 1, C)))
    # the product: one test-mode pass, RoI proposal, head, decode, NMS
    params = {"prThreshold": 0.05, "nmsThreshold": 0.5, "cornerThreshold": dns.corner_threshold}
    with audit.KernelAudit(model) as ka:
        results = dnd.get_detections(model, x, metas, params)
        torch.cuda.synchronize()
    layer_of = dict(audit.conv_layers(model))
    seen = set()
    for r in ka.table:
        g = audit.layer_geometry(layer_of[r["layer"]])[0]
        if g in m3:
            seen.add(g)
            assert any(n.startswith("wino4t_kernel") for n in r["fwd"]), r
    assert seen == m3
    last = [l for l in model.layers if l.type_name == "resnet"][-1].output.data
    rms = float(last.double().pow(2).mean().sqrt())
    assert 0.1 <= rms <= 10.0, rms
    lists = [list(l) for l in dns.sample_bbox_list]
    corner = dnc.corner_pr.cpu().numpy()
    _assert_proposal_of(corner, lists, params["cornerThreshold"], dns)
    det_pr, fitness, bbox, counts = dnd.last_outputs
    det_h, fit_h, box_h = det_pr.cpu().numpy(), fitness.cpu().numpy(), bbox.cpu().numpy()
    assert counts.tolist() == [len(l) for l in lists]
    sn, C, t0 = dns.sample_num, dnd.class_num, dnd._thresholds()[0]
    C1 = C + 1
    acts = []
    for i, layer in enumerate(model.layers[1:], 1):
        a = layer.output.data
        if a is None or a.dim() != 4:
            continue
        if i + 1 < len(model.layers) and model.layers[i + 1].output.data is a and layer.type_name == "conv":
            continue            # a convolution with its batch norm folded in: the tensor holds the batch norm's output (layer i + 1)
        acts.append(i)
    # the oracle, fp32 and the fp64 arbiter, 8 images at a time on the product's RoI lists
    js = model.export_json()
    om32 = OM.OracleModel(js, CH)
    with OM.float64_arbiter():
        om64 = OM.OracleModel(js, CH)
    table = {}
    for c0 in range(0, B, CH):
        sl = slice(c0, c0 + CH)
        om32.forward(x[sl], None, train=False, sample_override=lists[sl])
        with OM.float64_arbiter():
            om64.forward(x[sl], None, train=False, sample_override=lists[sl])
            o_det, o_fit, o_box = OL.detect_outputs(om64.detect_out.v, om64.sample_bbox, C, bool(dnd.use_jointfit), t0)
        pairs = [("corner_pr", corner[sl], om32.corner_pr, om64.corner_pr)]
        for i in acts:
            pairs.append(("L%d %s" % (i, model.layers[i].type_name), _chunk_nchw(model.layers[i].output.data, B, sl, om64.acts[i].shape),
                          om32.acts[i], om64.acts[i]))
        for what, a, r32, r64 in pairs:
            p, o = _err_stats(a, r64), _err_stats(r32, r64)
            prev = table.get(what)
            if prev is not None:
                p, o = tuple(map(max, p, prev["product_vs_fp64"])), tuple(map(max, o, prev["oracle32_vs_fp64"]))
            table[what] = {"product_vs_fp64": p, "oracle32_vs_fp64": o}
        # head: class log-probabilities and boxes of the valid RoIs against fp64
        cnt = counts[sl]
        valid = (np.arange(sn * sn)[None] < cnt[:, None]).reshape(CH, 1, sn, sn)
        d = det_h.reshape(B, sn, sn, C1)[sl].transpose(0, 3, 1, 2)
        np.testing.assert_allclose(np.where(valid, d, 0), np.where(valid, o_det, 0), rtol=1e-3, atol=1e-3)
        v4 = valid.reshape(CH, sn, sn, 1)
        bx = box_h.reshape(B, sn, sn, 4)[sl]
        np.testing.assert_allclose(np.where(v4, bx, 0), np.where(v4, o_box, 0), rtol=1e-3, atol=1e-4)
    del om32, om64
    for what, e in sorted(table.items(), key=lambda kv: -kv[1]["product_vs_fp64"][0])[:6]:
        print("B = 32 inference vs the fp64 arbiter (element-wise p99.99, max-norm): %-22s product %.2e %.2e   fp32 oracle %.2e %.2e"
              % ((what,) + tuple(e["product_vs_fp64"]) + tuple(e["oracle32_vs_fp64"])))
    for what, e in table.items():
        p, o = e["product_vs_fp64"], e["oracle32_vs_fp64"]
        for clause, pv, ov in (("element-wise p99.99", p[0], o[0]), ("max-norm", p[1], o[1])):
            assert pv <= 1e-3, "%s %s: %.2e against fp64 (north star: 1e-3)" % (what, clause, pv)
            assert pv <= max(1e-3, 1.5 * ov), "%s %s: product %.2e from fp64, the fp32 oracle %.2e" % (what, clause, pv, ov)
    assert len(table) > 20
    # threshold + NMS: exact on the product's decoded arrays
    ref = _oracle_nms(det_h, fit_h, box_h, counts, B, sn, C1, params["prThreshold"], params["nmsThreshold"], False)
    total = 0
    for b in range(B):
        dets = results[b]["detections"]
        assert len(dets) == len(ref[b])
        total += len(dets)
        for (pr, cls, box), r in zip(dets, ref[b]):
            assert cls == int(r[1]) and np.array_equal(np.array(box, np.float32), r[2:])
            assert abs(pr - r[0]) <= 2e-6 * r[0]
    print("B = 32 inference: %d RoIs, %d detections" % (int(counts.sum()), total))
    assert total > 0, "no detections: the NMS comparison checks nothing"
