"""The float64 batch-norm reference of tests/test_bn_fp64_gpu.py, host side (no device work): its closed form against autograd, what
float32 costs against it (the constants K_Y, K_DX, K_G and the share of undecided ReLU elements written in bn_reference.py are
measured here, from the restated float32 expressions and never from the device), and that the case table reaches every row
mapping of csrc/bn_reduce.h: bn_map and every class of its second stage."""
import numpy as np
import pytest
import torch

import bn_reference as R

SMALL = 1 << 20          # cases below this many elements are measured on three seeds, the larger ones on the GPU test's one


def _seeds(ci, shape):
    n = int(np.prod(shape))
    return [R.case_seed(ci, k) for k in ((0, 1, 2) if n < SMALL else (0,))]


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 1, 3, 4), (2, 3, 5, 12)])
@pytest.mark.parametrize("relu,res", R.MODES)
def test_closed_form_equals_autograd(shape, relu, res):
    """the formulas the kernels implement are the gradients of the float64 arbiter, M = 1 included (var = 0: dx = 0 exactly), and
    with the ReLU's decisions given from outside (some of them flipped against pre > 0)"""
    c = R.bn_case(shape, 5 + shape[-1])
    rs = c["res"] if res else None
    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], R.EPS, relu, rs)
    masks = [None]
    if relu:
        flipped = fwd["pre"] > 0
        flipped.view(-1)[::3] = ~flipped.view(-1)[::3]
        masks.append(flipped)
    for mask in masks:
        a = R.bn_ref64(c["x"], c["gamma"], c["beta"], R.EPS, relu, rs, c["dy"], mask=mask)
        b = R.bn_closed64(c["x"].numpy(), c["gamma"].numpy(), c["beta"].numpy(), R.EPS, relu, rs.numpy() if res else None,
                          c["dy"].numpy(), mask=None if mask is None else mask.numpy())
        for k in ("y", "pre", "mean", "inv", "dx", "dgamma", "dbeta"):
            scale = max(float(a[k].abs().max()), 1.0)
            assert float((a[k] - torch.from_numpy(b[k])).abs().max()) <= 1e-12 * scale, k
        if res:
            assert torch.equal(a["dres"], torch.from_numpy(b["dres"]))
        else:
            assert a["dres"] is None and b["dres"] is None
        if mask is not None:
            assert torch.equal(a["y"], torch.relu(a["pre"]))          # the value stays relu(pre); only the gradient follows the mask
            assert torch.equal(a["dres"] if res else a["g"], R._d(c["dy"]).reshape(-1, shape[-1]) * mask.double())
    if int(np.prod(shape[:-1])) == 1:
        assert not a["dx"].any() and not a["dgamma"].any()
        assert torch.equal(fwd["mean"], c["x"].double().reshape(-1)) and bool((fwd["inv"] == 1.0 / np.sqrt(np.float64(np.float32(R.EPS)))).all())


def test_reference_separates_the_variants_the_bounds_must_see():
    """unbiased variance and eps outside the root move `inv` by far more than its 2 u bound on the table's shapes (M up to 24 581:
    1 / (2 M) = 2e-5 = 340 u; 30 u in the channel whose variance is below eps)"""
    for shape in R.CASES:
        M = int(np.prod(shape[:-1]))
        if M == 1:
            continue
        c = R.bn_case(shape, 1)
        x = c["x"].double().reshape(-1, shape[-1])
        ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], R.EPS)
        eps = float(np.float32(R.EPS))
        unbiased = 1.0 / torch.sqrt(x.var(dim=0, unbiased=True) + eps)
        outside = 1.0 / (torch.sqrt(x.var(dim=0, unbiased=False)) + eps)
        live = torch.arange(shape[-1]) != 1                  # (the constant channel has no variance to be biased)
        assert float(((unbiased - ref["inv"]).abs() / ref["inv"])[live].min()) > 5 * 2 * R.U, shape
        if M >= 100:          # (the two placements of eps agree where std = 1/2, which a sample std over a few rows may come near)
            assert float(((outside - ref["inv"]).abs() / ref["inv"])[live].min()) > 20 * 2 * R.U, shape
        assert float(x.var(dim=0, unbiased=False)[0]) < eps and float(x.var(dim=0, unbiased=False)[1]) == 0.0
        assert float(ref["mean"][2].abs() * ref["inv"][2]) > 200.0


def test_float32_cost_is_inside_the_constants():
    """K_Y, K_DX, K_G are at least twice the worst ratio the restated float32 expressions show against float64 over the whole case
    table (every mode, every seed), none of them is above 8, the statistics of the restatement sit inside their code-derived bounds,
    dres is exact, no decided ReLU element is decided differently and the undecided share stays under UNDECIDED_MAX. The figures
    are printed; bn_reference.py quotes them"""
    worst = dict.fromkeys(("y", "dx", "dgamma", "dbeta", "mean", "inv", "run_mean", "run_stdinv"), 0.0)
    share_max = 0.0
    for ci, shape in enumerate(R.CASES):
        M = int(np.prod(shape[:-1]))
        for seed in _seeds(ci, shape):
            c = R.bn_case(shape, seed)
            n = {k: (v.numpy() if v is not None else None) for k, v in c.items()}
            for mi, (relu, res) in enumerate(R.MODES):
                mom = R.case_momentum(ci, mi)
                rs = c["res"] if res else None
                r32 = R.bn_restate32(n["x"], n["gamma"], n["beta"], R.EPS, relu, n["res"] if res else None, n["dy"],
                                     run=(n["run_mean"], n["run_stdinv"]), momentum=mom)
                mask = None
                if relu:
                    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], R.EPS, relu, rs)
                    mask, und, wrong = R.relu_decisions(fwd["pre"], R.bn_bounds(fwd, c["gamma"])["y"], torch.from_numpy(r32["y"] > 0))
                    assert not wrong.any(), (shape, seed, relu, res, int(wrong.sum()))
                    assert int(und.sum()) <= R.UNDECIDED_MAX * und.numel(), (shape, seed, relu, res, int(und.sum()))
                    share_max = max(share_max, float(und.double().mean()))
                ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], R.EPS, relu, rs, c["dy"], mask=mask,
                                 run=(c["run_mean"], c["run_stdinv"]), momentum=mom)
                unit = R.bn_bounds(ref, c["gamma"], 1.0, 1.0, 1.0)
                for k, v in R.ratios(r32, ref, unit, worst).items():
                    assert np.isfinite(v), (shape, seed, relu, res, k)
                    worst[k] = max(worst[k], v)
                if res:
                    assert np.array_equal(r32["dres"], ref["dres"].numpy().astype(np.float32))
    print("worst error / unit bound:", {k: round(v, 3) for k, v in worst.items()}, "; undecided share %.2e" % share_max)
    for k, const in (("y", R.K_Y), ("dx", R.K_DX), ("dgamma", R.K_G)):
        assert 2.0 * worst[k] <= const <= 8.0, (k, worst[k], const)
        assert const <= 2.0 * worst[k] * 1.25, (k, worst[k], const)        # ... and are not padded beyond the rule
    for k in ("dbeta", "mean", "inv", "run_mean", "run_stdinv"):
        assert worst[k] <= 1.0, (k, worst[k])
    assert share_max <= R.UNDECIDED_MAX


def test_case_table_reaches_every_mapping():
    maps = [R.bn_map(int(np.prod(s[:-1])), s[-1]) for s in R.CASES]
    Ms = [int(np.prod(s[:-1])) for s in R.CASES]
    assert {m.LC for m in maps} >= {1, 2, 8, 16, 32, 128, 256}
    assert {m.gx for m in maps} >= {1, 2, 3, 5}
    assert {min(m.sweeps, 3) for m in maps} == {1, 2, 3}
    assert {m.LC for m in maps if m.sweeps >= 2} >= {8, 16, 32, 128, 256}
    assert any(m.LC == 256 and m.gx > 1 and m.sweeps >= 2 for m in maps)
    # a last sweep of one row: one workgroup, one row slot, one row
    assert any(m.sweeps >= 2 and M - (m.sweeps - 1) * m.gy * m.RS == 1 for m, M in zip(maps, Ms))
    # a single sweep whose last workgroup holds a single row
    assert any(m.sweeps == 1 and m.gy > 1 and M - (m.gy - 1) * m.RS == 1 for m, M in zip(maps, Ms))
    assert any(1 < M < m.RS for m, M in zip(maps, Ms)) and 1 in Ms
    # what the table says of each case
    want = {(1, 1, 3, 4): (1, 256, 1, 1, 1), (1, 1, 1, 64): (16, 16, 1, 1, 1), (1, 20, 15, 12): (1, 256, 3, 2, 1),
            (3, 5, 7, 24): (2, 128, 3, 1, 1), (1, 33, 33, 96): (8, 32, 3, 35, 1), (1, 105, 104, 96): (8, 32, 3, 341, 2),
            (1, 80, 82, 160): (8, 32, 5, 204, 2), (2, 91, 91, 64): (16, 16, 1, 1024, 2), (1, 47, 523, 128): (32, 8, 1, 1024, 4),
            (1, 3, 455, 1536): (128, 2, 3, 341, 3), (1, 25, 41, 2048): (256, 1, 2, 512, 3), (1, 7, 100, 3072): (256, 1, 3, 341, 3)}
    assert {s: tuple(m) for s, m in zip(R.CASES, maps)} == want
    # the shapes of the old kernel test never loop (the gap this table closes)
    for s in [(4, 16, 16, 64), (2, 8, 8, 1536), (3, 5, 7, 768), (2, 32, 32, 128)]:
        assert R.bn_map(int(np.prod(s[:-1])), s[-1]).sweeps == 1
    # the fused layer: both reductions and the general apply kernel loop at the two large maps
    for N, H, W, C, k, s, p in R.POOL_CASES[:2]:
        assert R.bn_map(N * H * W, C).sweeps == 2
    assert all(H % 2 == 0 and W % 2 == 0 for _, H, W, *_ in R.POOL_CASES[:1]) and R.POOL_CASES[1][1] % 2 == 1


def test_partial_lists_reach_every_class_of_the_second_stage():
    """(rounds of the four-in-flight loop, single rows after it, idle lanes) of lane 0 for the list lengths the GPU test feeds,
    and the slices of the fold"""
    assert [R.final_lane0(r) for r in R.FINAL_ROWS] == [(0, 1, 31), (0, 1, 1), (0, 2, 0), (1, 0, 0), (1, 1, 0), (16, 0, 0)]
    assert [R.fold_map(r) for r in R.FOLD_ROWS] == [(33, 63, 3), (33, 64, 32), (65, 64, 2), (256, 64, 256)]
    assert all(R.fold_map(r)[1] <= 64 for r in range(2049, 20000, 7))      # the folded list fits the 64 rows of the workspace
    x = R.bn_case((1, 9, 13, 8), 3)["x"].reshape(-1, 8)
    g, h = torch.randn(117, 8, dtype=torch.float64), torch.randn(117, 8, dtype=torch.float64)
    for rows in R.FINAL_ROWS + R.FOLD_ROWS:
        p = R.split_partials(x, rows, np.random.RandomState(rows))
        assert p.shape == (rows, 2, 8) and p.dtype == torch.float64
        xd = x.double()
        assert float((p[:, 0].sum(0) - xd.sum(0)).abs().max()) <= 1e-12 * float(xd.abs().sum(0).max())
        assert float((p[:, 1].sum(0) - (xd * xd).sum(0)).abs().max()) <= 1e-12 * float((xd * xd).sum(0).max())
        empty = int((p.abs().sum(dim=(1, 2)) == 0).sum())
        assert empty >= (rows // 3 - 2 if rows >= 3 else 0) and (empty > 0 or rows < 9)
        assert float(p[0].abs().sum()) > 0 and float(p[-1].abs().sum()) > 0          # the ends of the list hold data
        if 3 <= rows <= 31:
            counts = p[:, 1, 1] / 0.75 ** 2                   # the constant channel counts the rows of each set
            assert float(counts.max()) >= 3 * float(counts[counts > 0].min())      # uneven
        q = R.split_partials((g, h), rows, np.random.RandomState(rows + 1))
        assert float((q[:, 0].sum(0) - g.sum(0)).abs().max()) <= 1e-12 * 117 and float((q[:, 1].sum(0) - h.sum(0)).abs().max()) <= 1e-12 * 117


def test_pool_reference_on_a_known_map():
    y = torch.arange(16, dtype=torch.float64).reshape(1, 4, 4, 1) - 5.0
    mx, vals, near = R.pool_ref64(torch.relu(y), 3, 2, 1, torch.zeros(1, dtype=torch.float64))
    assert mx.reshape(2, 2).tolist() == [[0.0, 2.0], [8.0, 10.0]]
    assert vals.shape == (1, 2, 2, 1, 9) and bool(torch.isinf(vals[0, 0, 0, 0, :4]).all()) and float(vals[0, 0, 0, 0, 4]) == 0.0
    assert near[0, 0, 0, 0].tolist() == [False, False, False, False, True, True, False, True, True]
    assert near[0, 1, 1, 0].tolist() == [False] * 8 + [True]
    arg = torch.tensor([4, 8, 8, 8], dtype=torch.uint8).reshape(1, 2, 2, 1)
    routed, flat = R.pool_route64(torch.tensor([1.0, 2.0, 3.0, 4.0]).reshape(1, 2, 2, 1), arg, (1, 4, 4, 1), 3, 2, 1)
    assert flat.reshape(-1).tolist() == [0, 7, 13, 15] and routed.reshape(-1)[[0, 7, 13, 15]].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert float(routed.sum()) == 10.0
