"""Opt-in bf16 inference (ops.INFER_PRECISION = "bf16", csrc/conv_bf16.hip) on the device.

The numerics contract ("bf16 inference") and the checker that states its bound - fp64 on the operands the kernel really
multiplies - are in tests/bf16_reference.py."""
import numpy as np
import pytest
import torch

from bf16_reference import check_fwd, draw, ties
from denet_amd import ops
from denet_amd.model import audit, model_cnn, update_bn, zoo
from fp64_model import build_model

pytestmark = pytest.mark.gpu

BF16 = "conv_bf16_kernel"


# (N, H, W, C, K physical, K logical, filter, stride, pad, ohw, epilogue)
GEOMS = {
    "one-tile": (1, 8, 8, 32, 32, 32, 3, 1, 1, None, False),
    "odd-strided-partial": (2, 9, 7, 96, 160, 160, 3, 2, 1, None, False),
    "17-chunks-1x1": (3, 12, 12, 544, 128, 128, 1, 1, 0, None, False),
    "epilogue": (1, 16, 16, 64, 64, 64, 3, 1, 1, None, True),
    "even-same-cut": (1, 10, 10, 32, 96, 96, 2, 1, 1, (10, 10), False),
    "pad-channels": (1, 8, 8, 32, 128, 100, 3, 1, 1, None, False),
}


def _operands(name):
    N, H, W, C, K, Kl, k, stride, pad, ohw, epi = GEOMS[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    x = draw(rng, N, H, W, C)
    w = draw(rng, K, k, k, C, scale=(k * k * C) ** -0.5)
    w[Kl:] = 0.0                                     # pad filters are zero, as Param packs them
    bias = add = None
    if epi or Kl != K:
        bias = draw(rng, K, scale=0.5)
        bias[Kl:] = 0.0
    if epi:
        OH = (H + 2 * pad - k) // stride + 1
        add = draw(rng, N, OH, OH, K)
    return x, w, bias, add


def _run(name):
    N, H, W, C, K, Kl, k, stride, pad, ohw, epi = GEOMS[name]
    x, w, bias, add = _operands(name)
    dev = lambda t: None if t is None else t.cuda()
    xd, wd, bd, ad = dev(x), dev(w), dev(bias), dev(add)
    w16 = ops.filter_to_bf16(wd)
    y = ops.conv_fwd_bf16(xd, w16, bias=bd, add=ad, stride=stride, pad=pad, relu=epi, ohw=ohw)
    torch.cuda.synchronize()
    return (x, w, bias, add), y, w16


# -------------------------------------------------------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("name", list(GEOMS))
def test_kernel_against_fp64_on_the_rounded_operands(hip, name):
    N, H, W, C, K, Kl, k, stride, pad, ohw, epi = GEOMS[name]
    (x, w, bias, add), y, w16 = _run(name)
    # the filter copy is the RNE rounding of the fp32 filter, bit for bit
    assert torch.equal(w16.cpu().view(torch.int16), w.bfloat16().view(torch.int16))
    check_fwd(y, x, w, bias, add, relu=epi, stride=stride, pad=pad, ohw=ohw, what=name)
    if ohw is not None:
        assert tuple(y.shape[1:3]) == ohw
    if Kl != K:
        padc = y[..., Kl:].contiguous().view(torch.int32)
        assert int(padc.abs().max()) == 0, "pad channels must be +0 (sign bit clear)"
        assert bool((x < 0).any())                   # (products of either sign entered those sums)


# -------------------------------------------------------------------------------------------------------- 2: the rounding mode
def test_operands_are_rounded_to_nearest_even_bit_for_bit(hip):
    """1x1 identity filter: y is the staged (rounded) x itself. Values exactly halfway between two bf16 neighbours (ties go to the
    even mantissa), and one fp32 ulp either side of them"""
    vals = ties()
    rng = np.random.RandomState(3)
    x = rng.standard_normal((2, 5, 7, 32)).astype(np.float32)
    x.reshape(-1)[:: 3][:vals.size * 8] = np.tile(vals, 8)
    x = torch.from_numpy(x)
    w = torch.eye(32).reshape(32, 1, 1, 32).contiguous()
    y = ops.conv_fwd_bf16(x.cuda(), ops.filter_to_bf16(w.cuda()))
    want = x.bfloat16().float()
    assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------- 3: determinism
def test_two_calls_are_bit_identical(hip):
    _, y0, _ = _run("odd-strided-partial")
    _, y1, _ = _run("odd-strided-partial")
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4: a model, layer by layer
STACK_DESC = "C[32,3] BN A C[64,3] BN A C[64,3,2] BN A C[96,1] BN A P.A[8] R"
RSN_DESC = "C[32,3] BN A RSN[32,3] RSN.O[64,3,2] P.A[8] R"
STACK_B, STACK_IMG, STACK_CLASSES = 4, 16, 10


def _build(desc, seed=5):
    m = build_model(desc, (3, STACK_IMG, STACK_IMG), STACK_B, STACK_CLASSES, seed=seed, head_scale=0.05)
    rng = np.random.RandomState(seed + 1)
    for l in model_cnn.walk_layers(m.layers):
        if l.type_name in ("batchnorm", "batchnorm-relu") and l.enabled:
            C = l.mean.value.shape[0]
            l.mean.set_value(rng.normal(0, 0.2, C).astype(np.float32))
            l.stdinv.set_value(rng.uniform(0.7, 1.4, C).astype(np.float32))
            l.omega.set_value(rng.uniform(0.7, 1.3, C).astype(np.float32))
            l.beta.set_value(rng.normal(0.0, 0.3, C).astype(np.float32))
    return m


def _stack_input(seed=9):
    return np.random.RandomState(seed).uniform(0.0, 1.0, (STACK_B, 3, STACK_IMG, STACK_IMG)).astype(np.float32)


def test_model_layers_against_fp64_on_their_own_inputs(hip):
    model = _build(STACK_DESC)
    model.build_train_func("nesterov")
    x = _stack_input()
    with ops.infer_precision("bf16"), audit.KernelAudit(model) as ka:
        pr = model.predict_output_step(x)
    assert np.isfinite(pr).all() and pr.shape == (STACK_B, STACK_CLASSES)
    rows = ka.table
    assert len(rows) == 5, rows
    for r in (rows[0], rows[-1]):                    # the stem (4 planar channels) and the convolution the softmax reads
        assert r["fwd"] and not any(BF16 in s for s in r["fwd"]), r
    assert [r["fwd"] for r in rows[1:4]] == [[BF16 + "<128, 64>"], [BF16 + "<128, 64>"], [BF16 + "<128, 128>"]], rows
    convs = [l for _, l in audit.conv_layers(model)]
    for i, conv in enumerate(convs[1:4]):
        ent = conv._cache()["fold"]
        bn = ent[1]
        relu = bn.type_name == "batchnorm-relu" or bool(getattr(bn, "act_fused", False))
        check_fwd(conv.output.data, conv.input.data, ent[2], bias=ent[3], relu=relu, stride=conv.stride[0], pad=conv.pad,
                  ohw=conv.ohw, what="stack conv %d" % (i + 1))
    # the distance to fp32 mode is reported, not asserted: rounding flips move a free-running comparison
    pr32 = model.predict_output_step(x)
    print("stack: max |p_bf16 - p_fp32| = %.3e" % float(np.abs(pr - pr32).max()))


def test_residual_blocks_run_on_the_bf16_kernel(hip):
    model = _build(RSN_DESC, seed=6)
    model.build_train_func("nesterov")
    x = _stack_input(10)
    with ops.infer_precision("bf16"), audit.KernelAudit(model) as ka:
        pr = model.predict_output_step(x)
    assert np.isfinite(pr).all()
    assert abs(float(pr.sum()) - STACK_B) < 1e-3
    inner = [r for r in ka.table if ".resnet" in r["layer"]]
    assert len(inner) == 5, ka.table                 # RSN: 2 convolutions; RSN.O with a stride: 2 + the shortcut projection
    for r in inner:
        assert len(r["fwd"]) == 1 and r["fwd"][0].startswith(BF16), r
    for r in (ka.table[0], ka.table[-1]):
        assert r["fwd"] and not any(BF16 in s for s in r["fwd"]), r
    # the residual rides in the epilogue of the last convolution of each block: check that one against fp64 too
    blocks = [l for l in model.layers if l.type_name == "resnet"]
    pre = blocks[0]._main()[-1]
    check_fwd(pre.output.data, pre.input.data, pre._w(), add=blocks[0].input.data, stride=1, pad=pre.pad,
              what="RSN last convolution (+ x)")
    assert blocks[1].__dict__.get("_plan"), "the RSN.O block did not run its folded plan"
    last = [l for l in blocks[1]._main() if l.type_name == "conv"][-1]
    ent = last._cache()["fold"]
    sc = blocks[1]._shortcut()
    check_fwd(last.output.data, last.input.data, ent[2], bias=ent[3], add=sc[-1].output.data, relu=True, stride=1, pad=last.pad,
              what="RSN.O last convolution (+ shortcut, ReLU)")


# ------------------------------------------------------------------------------------------- 5: no leakage, no stale caches
def test_fp32_results_do_not_change_around_a_bf16_call(hip):
    model = _build(STACK_DESC)
    x = _stack_input()
    before = model.predict_output_step(x)
    with ops.infer_precision("bf16"):
        low = model.predict_output_step(x)
        with ops.infer_precision("fp32"):
            inside = model.predict_output_step(x)
    after = model.predict_output_step(x)
    assert np.array_equal(before.view(np.uint32), inside.view(np.uint32))
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert not np.array_equal(before, low), "the bf16 pass ran the fp32 kernels"


def test_bf16_caches_follow_the_weights(hip, tmp_path):
    model = _build(STACK_DESC)
    model.build_train_func("nesterov")
    x, metas = zoo.synthetic_batch(STACK_B, STACK_IMG, STACK_CLASSES, seed=4)
    with ops.infer_precision("bf16"):
        p0 = model.predict_output_step(x)
        with audit.KernelAudit(model) as ka:
            cost, _ = model.train_step(x, metas, 0, 0, 0.05, [0.9], 1e-4)
        assert np.isfinite(cost)
        assert not any(BF16 in s for r in ka.table for s in r["fwd"] + r["bwd"]), "a training step took the bf16 kernel"
        p1 = model.predict_output_step(x)
        fname = str(tmp_path / "trained.mdl.gz")
        model_cnn.save_to_file(model, fname)
        fresh = model_cnn.load_from_file(fname, STACK_B)
        p2 = fresh.predict_output_step(x)
    assert not np.array_equal(p0, p1)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))


def test_update_bn_stays_fp32(hip, monkeypatch):
    rng = np.random.RandomState(8)
    batches = [rng.uniform(-1.0, 2.0, (STACK_B, 3, STACK_IMG, STACK_IMG)).astype(np.float32) for _ in range(2)]
    stats = []
    for precision in ("fp32", "bf16"):
        monkeypatch.setattr(ops, "INFER_PRECISION", precision)
        model = _build(STACK_DESC)
        with audit.KernelAudit(model) as ka:
            res = update_bn.update_bn(model, batches)
        assert not any(BF16 in s for r in ka.table for s in r["fwd"])
        assert ops.INFER_PRECISION == precision
        stats.append([(m.copy(), s.copy()) for _, _, m, _, s in res])
    assert len(stats[0]) == 4
    for (m0, s0), (m1, s1) in zip(*stats):
        assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32)) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- 6: detection
def test_get_detections_in_bf16_mode(hip):
    B, IMG = 2, 128
    model = zoo.denet34(B, "skip", IMG, class_num=20, seed=1)
    rng = np.random.RandomState(5)
    dnd = [l for l in model.layers if l.type_name == "denet-detect"][0]
    dconv = dnd.layers[0]
    dconv.omega.set_value(rng.normal(0, 0.3, dconv.omega.value.shape))
    zoo.warm_corner_head(model, 4.0, 0.3)
    x, metas = zoo.synthetic_batch(B, IMG, seed=2)
    params = {"prThreshold": 0.08, "nmsThreshold": 0.5, "cornerThreshold": 0.02, "useSoftNMS": 0}
    # class logits of order one, like a trained head (test-mode BN on untrained statistics blows the activations up)
    dnd.get_detections(model, x, metas, params)
    raw = dnd.conv.output.data.float().cpu().numpy().reshape(-1, dnd.conv.kp)
    w = dconv.omega.get_value().copy()
    w[:dnd.s0] *= 2.0 / raw[:, :dnd.s0].std()
    w[dnd.s0:dnd.s0 + 4] *= 0.2 / raw[:, dnd.s0:dnd.s0 + 4].std()
    dconv.omega.set_value(w)
    first = dnd.get_detections(model, x, metas, params)
    assert sum(len(r["detections"]) for r in first) > 0
    with ops.infer_precision("bf16"), audit.KernelAudit(model) as ka:
        low = dnd.get_detections(model, x, metas, params)
    n_bf16 = 0
    for i, r in enumerate(ka.table):
        top = r["layer"].split(".")[1]
        if i == 0 or top in ("denet-corner", "denet-detect"):
            assert r["fwd"] and not any(BF16 in s for s in r["fwd"]), r
        else:
            assert r["fwd"] and all(s.startswith(BF16) for s in r["fwd"]), r
            n_bf16 += 1
    assert n_bf16 >= 30, n_bf16
    assert {r["layer"].split(".")[1] for r in ka.table} >= {"denet-corner", "denet-detect", "resnet"}
    assert len(low) == B
    for b, res in enumerate(low):
        assert res["meta"] is metas[b]
        for pr, cls, box in res["detections"]:
            assert 0.0 < pr <= 1.0 and 0 <= cls < 20 and len(box) == 4 and all(np.isfinite(box))
    print("detections fp32 / bf16 per image:", [(len(a["detections"]), len(c["detections"])) for a, c in zip(first, low)])
    again = dnd.get_detections(model, x, metas, params)
    assert [r["detections"] for r in again] == [r["detections"] for r in first]
