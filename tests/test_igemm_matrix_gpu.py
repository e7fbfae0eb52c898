"""All 27 instantiations of csrc/igemm.hip's kernel text (4 modes x tiles x NBUF 1 / 2 / 3) through the C ABI at the rows of
tests/igemm_matrix.py: one case per pass and geometry, the float64 reference (CPU) computed once, then every (tile, loop structure)
record imported in turn - denet_conv_last_config read after every launch. Each result within 1e-5 of float64 (max|a - b| / max|b|,
the bound of the direct fp32 kernels), and the bit equalities the kernel promises: one geometry gives the same bits under every
(tile, NBUF), MODE_DGRAD / MODE_DGRAD_T / the 1x1 forward form give each other's bits (dx, dx + add, the backward sums), a repeated
launch gives the same bits, filter gradients of equal split agree across NBUF. Outputs lie in sentinel-filled buffers."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import igemm_matrix as M
from igemm_matrix import Guarded, _TunedTable

pytestmark = pytest.mark.gpu

BOUND = 1e-5
TOTALS = {}                       # pass -> [launches checked, largest error against float64]


def _count(what, n=1, err=0.0):
    t = TOTALS.setdefault(what, [0, 0.0])
    t[0] += n
    t[1] = max(t[1], err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print("\nigemm matrix: %.1f s, %d launches checked" % (time.time() - t0, sum(v[0] for v in TOTALS.values())))
    for what, (n, err) in sorted(TOTALS.items()):
        print("igemm matrix: %-12s %5d launches, largest error against float64 %.2e" % (what, n, err))


def _ids(cases):
    return [c.id for c in cases]


def _check_ran(L, case, rec):
    want = [M.KERNEL_MODE[case.code]] + list(M.intended(case, rec))
    got = M.ran(L)
    assert got == want, (case.id, rec, "ran", got, "intended", want)


def _err(what, a, ref, bound=BOUND):
    e = M.rel_err(a, ref)
    assert e <= bound, (what, e, bound)
    return e


def _same_bits(outs, what):
    first = next(iter(outs))
    for k, v in outs.items():
        for name in v:
            assert torch.equal(v[name], outs[first][name]), "%s: %s under %s differs from %s" % (what, name, k, first)


def _stats_view(buf, rows, cols):
    return buf.t[:rows * 2 * cols].view(rows, 2, cols)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def _fwd(L, g, t, y, bias=None, add=None, relu=0, stats=None):
    from denet_amd.ops import ptr, stream_ptr
    if stats is not None:
        rows = ctypes.c_int(0)
        rc = L.denet_conv_fwd_stats(ptr(t["x"]), ptr(t["w"]), ptr(bias), ptr(add), ptr(y), ptr(stats), stats.numel() * 8,
                                    ctypes.byref(rows), *g, stream_ptr())
        assert rc == 0, (g, rc, L.denet_last_error())
        return rows.value
    if relu:
        rc = L.denet_conv_fwd_act(ptr(t["x"]), ptr(t["w"]), ptr(bias), ptr(add), ptr(y), 1, *g, stream_ptr())
    else:
        rc = L.denet_conv_fwd(ptr(t["x"]), ptr(t["w"]), ptr(bias), ptr(add), ptr(y), *g, stream_ptr())
    assert rc == 0, (g, rc, L.denet_last_error())


@pytest.mark.parametrize("case", M.cases_of(M.FWD), ids=_ids(M.cases_of(M.FWD)))
def test_forward(hip, case):
    """plain, bias + add + ReLU, and the batch-norm column sums of the stored output (rows beyond M contribute nothing)"""
    g = case.g
    N, H, W, C, K = g[:5]
    t = M.tensors(g)
    ref = M.ref_fwd(t, g)
    ref_act = (ref + t["bias"].double().cpu() + t["add_y"].double().cpu()).clamp_min(0)
    rows_m = ref.numel() // K
    y, st = Guarded(ref.shape), Guarded((-(-rows_m // 128) * 2 * K,), torch.float64)
    outs = {}
    with _TunedTable() as L:
        for rec in case.records:
            M.import_record(L, *M.record_key(case), *rec)
            o = {}
            for rep in range(2):
                _fwd(L, g, t, y.arm())
                _check_ran(L, case, rec)
                assert y.intact()
                o.setdefault("y", y.t.clone())
                assert torch.equal(o["y"], y.t), (case.id, rec, "a repeated launch differs")
                _fwd(L, g, t, y.arm(), bias=t["bias"], add=t["add_y"], relu=1)
                _check_ran(L, case, rec)
                assert y.intact()
                o.setdefault("act", y.t.clone())
                assert torch.equal(o["act"], y.t), (case.id, rec, "a repeated launch differs (bias + add + ReLU)")
                y.arm(), st.arm()
                rows = _fwd(L, g, t, y.t, add=t["add_y"], stats=st.t)
                _check_ran(L, case, rec)
                assert y.intact() and st.intact() and rows == -(-rows_m // 128)
                o.setdefault("y_add", y.t.clone())
                o.setdefault("sums", _stats_view(st, rows, K).clone())
                assert torch.equal(o["y_add"], y.t) and torch.equal(o["sums"], _stats_view(st, rows, K)), (case.id, rec, "sums repeat")
            e = max(_err((case.id, rec, "y"), o["y"], ref), _err((case.id, rec, "act"), o["act"], ref_act),
                    _err((case.id, rec, "y + add"), o["y_add"], ref + t["add_y"].double().cpu()))
            _count("fwd", 6, e)
            yd = o["y_add"].double().reshape(-1, K)
            part = o["sums"].sum(0)
            torch.testing.assert_close(part[0], yd.sum(0), rtol=1e-5, atol=1e-4)
            torch.testing.assert_close(part[1], (yd * yd).sum(0), rtol=1e-5, atol=1e-4)
            outs[rec] = o
    _same_bits(outs, case.id)


# ---- data gradients ----------------------------------------------------------------------------------------------------------------
def _bn_of(g):
    """a ReLU batch norm over the data gradient's tensor: input, output, parameters and saved statistics, seeded by the geometry"""
    N, H, W, C = g[:4]
    gen = torch.Generator().manual_seed(M.seed_of(g) + 104729)
    xb = torch.randn(N, H, W, C, generator=gen) * 1.5 + 0.3
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    mean, invstd = xb.reshape(-1, C).mean(0), 1.0 / xb.reshape(-1, C).std(0)
    yb = torch.relu((xb - mean) * invstd * gamma + beta)
    return {k: v.cuda() for k, v in dict(x=xb, y=yb, gamma=gamma, beta=beta, mean=mean, invstd=invstd).items()}


def _link(bn):
    from denet_amd import ops
    return ops._bn_link_struct(bn["x"], None, bn["y"], bn["gamma"], bn["beta"], bn["mean"], bn["invstd"], None, None, 1)


def _dgrad(L, code, g, t, dx, add=None, bn=None, stats=None):
    """pass 1 (denet_conv_dgrad / _sums), 5 (denet_conv_dgrad_t) or 6 (denet_conv_dgrad_1x1t); with bn: returns the rows of sums"""
    from denet_amd.ops import ptr, stream_ptr
    N, H, W, C, K = g[:5]
    rows = ctypes.c_int(0)
    link = _link(bn) if bn is not None else None
    lp = ctypes.byref(link) if link is not None else None
    sb = stats.numel() * 8 if stats is not None else 0
    rp = ctypes.byref(rows) if link is not None else None
    if code == M.DGRAD and bn is None:
        rc = L.denet_conv_dgrad(ptr(t["dy"]), ptr(t["w"]), ptr(add), ptr(dx), *g, stream_ptr())
    elif code == M.DGRAD:
        rc = L.denet_conv_dgrad_sums(ptr(t["dy"]), ptr(t["w"]), ptr(add), ptr(dx), lp, ptr(stats), sb, rp, *g, stream_ptr())
    elif code == M.DGRAD_T:
        rc = L.denet_conv_dgrad_t(ptr(t["dy"]), ptr(t["wt"]), ptr(add), ptr(dx), lp, ptr(stats), sb, rp, *g, stream_ptr())
    else:
        rc = L.denet_conv_dgrad_1x1t(ptr(t["dy"]), ptr(t["wt"]), ptr(add), ptr(dx), lp, ptr(stats), sb, rp, N, H, W, C, K, stream_ptr())
    assert rc == 0, (code, g, rc, L.denet_last_error())
    return rows.value


def _dgrad_three(L, case, rec, t, bn, dx, st, what):
    """dx, dx + add and dx + add with the backward sums of one configuration, each launched twice; {name: tensor}"""
    g = case.g
    C, stride = g[3], g[8]
    rows_want = stride * stride * -(-M.rows_cols(case)[0] // 128)
    o = {}

    def keep(name, now):
        o.setdefault(name, now.clone())
        assert torch.equal(o[name], now), (what, name, "a repeated launch differs")

    for rep in range(2):
        _dgrad(L, case.code, g, t, dx.arm())
        _check_ran(L, case, rec)
        assert dx.intact()
        keep("dx", dx.t)
        _dgrad(L, case.code, g, t, dx.arm(), add=t["add_x"])
        _check_ran(L, case, rec)
        assert dx.intact()
        keep("dx_add", dx.t)
        dx.arm(), st.arm()
        rows = _dgrad(L, case.code, g, t, dx.t, add=t["add_x"], bn=bn, stats=st.t)
        _check_ran(L, case, rec)
        assert dx.intact() and st.intact() and rows == rows_want, (what, rows, rows_want)
        keep("dx_sums", dx.t)
        keep("sums", _stats_view(st, rows, C))
    assert torch.equal(o["dx_add"], o["dx_sums"]), (what, "the request for sums changed the gradient")
    return o


@pytest.mark.parametrize("case", M.cases_of(M.DGRAD), ids=_ids(M.cases_of(M.DGRAD)))
def test_data_gradient(hip, case):
    """MODE_DGRAD under all six records, MODE_DGRAD_T as its rule runs it and, for 1x1 stride 1, the forward form over the transposed
    filter under all six records of the swapped forward key: float64, and one set of bits for all of them"""
    g = case.g
    N, H, W, C, K, R, S, _, stride, pad = g[:10]
    name = case.id[len("dgrad_"):]
    t = M.tensors(g)
    bn = _bn_of(g)
    ref = M.ref_dgrad(t, g)
    ref_add = ref + t["add_x"].double().cpu()
    gm = torch.where(bn["y"].double().cpu() > 0, ref_add, torch.zeros_like(ref_add)).reshape(-1, C)
    xhat = ((bn["x"] - bn["mean"]) * bn["invstd"]).double().cpu().reshape(-1, C)
    sums_ref = torch.stack([gm.sum(0), (gm * xhat).sum(0)])
    scale = float(gm.abs().sum(0).max())
    dx = Guarded(ref.shape)
    st = Guarded((stride * stride * -(-M.rows_cols(case)[0] // 128) * 2 * C,), torch.float64)
    runs = [(case, rec) for rec in case.records] + [(M.BY_ID["dgrad_t_" + name], None)]
    if "dgrad_1x1t_" + name[4:] in M.BY_ID and name.startswith("1x1_k"):
        c6 = M.BY_ID["dgrad_1x1t_" + name[4:]]
        runs += [(c6, rec) for rec in c6.records]
    outs = {}
    with _TunedTable() as L:
        for c, rec in runs:
            if rec is not None:
                M.import_record(L, *M.record_key(c), *rec)
            what = (c.id, rec)
            o = _dgrad_three(L, c, rec, t, bn, dx, st, what)
            e = max(_err((what, "dx"), o["dx"], ref), _err((what, "dx + add"), o["dx_add"], ref_add))
            es = float((o["sums"].sum(0).cpu() - sums_ref).abs().max()) / scale
            assert es <= 5e-5, (what, "backward sums", es)
            _count({M.DGRAD: "dgrad", M.DGRAD_T: "dgrad_t", M.DGRAD_1X1T: "dgrad_1x1t"}[c.code], 6, e)
            _count("bwd sums", 2, es)
            outs[what] = o
    _same_bits(outs, case.id)
    any_o = next(iter(outs.values()))
    if name == "1x1_s2":              # the three parity classes without a tap: exact zeros, and the bits of `add` with it
        for py, px in ((0, 1), (1, 0), (1, 1)):
            assert not any_o["dx"][:, py::2, px::2].any()
            assert torch.equal(any_o["dx_add"][:, py::2, px::2], t["add_x"][:, py::2, px::2])


def test_data_gradient_t_instantiations_only_a_switch_reaches(hip, tmp_path):
    """MODE_DGRAD_T 128x128 / NBUF 1, 128x128 / 3, 128x64 / 3 and 128x128 / 2 at short reductions: DENET_DGRAD_T_TILE / _NBUF are read
    once per process, so each setting runs tests/igemm_matrix.py in a fresh child, one after another, the first failure ends it.
    The children's dx and dx + add of every data-gradient geometry are the bits of this process's MODE_DGRAD."""
    mine = {}
    with _TunedTable() as L:
        for case in M.cases_of(M.DGRAD):
            t = M.tensors(case.g)
            dx = Guarded(t["dx"].shape)
            o = {}
            for key, addt in (("dx", None), ("dxa", t["add_x"])):
                _dgrad(L, M.DGRAD, case.g, t, dx.arm(), add=addt)
                o[key] = dx.t.cpu().numpy().copy()
            assert M.ran(L)[0] == 1
            mine[case.id[len("dgrad_"):]] = o
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "igemm_matrix.py")
    for tile, nbuf in M.DGRAD_T_CHILDREN:
        out = str(tmp_path / ("dgrad_t_%d_%d.npz" % (tile, nbuf)))
        env = dict(os.environ, DENET_DGRAD_T_TILE=str(tile), DENET_DGRAD_T_NBUF=str(nbuf))
        r = subprocess.run([sys.executable, script, "--dgrad-t-child", out], env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, ("child", tile, nbuf, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        got = np.load(out)
        for case in M.cases_of(M.DGRAD_T, switch=True):
            if case.switch != (tile, nbuf):
                continue
            name = case.id.split("_", 2)[2]
            want = [M.KERNEL_MODE[case.code]] + list(M.intended(case, None))
            assert list(got["cfg_" + name]) == want, (case.id, list(got["cfg_" + name]), want)
            for key in ("dx", "dxa"):
                assert np.array_equal(got[key + "_" + name].view(np.uint32), mine[name][key].view(np.uint32)), (case.id, key)
            _count("dgrad_t", 2)


# ---- filter gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.cases_of(M.WGRAD), ids=_ids(M.cases_of(M.WGRAD)))
def test_filter_gradient(hip, case):
    """every tile x NBUF x rounds record: float64; equal splits give equal bits; the last 5 channels of dy and the last 3 of x are
    zero (padding channels): their rows and columns of dw are exact zeros"""
    from denet_amd.ops import ptr, stream_ptr
    g = case.g
    K, C = g[4], g[3]
    t = M.tensors(g)
    t["x"][..., C - 3:] = 0
    t["dy"][..., K - 5:] = 0
    ref = M.ref_wgrad(t, g)
    dw = Guarded(ref.shape)
    ws = t["ws"] if case.ws else None
    assert ws is None or ws.numel() * 4 == case.ws
    outs = {}
    with _TunedTable() as L:
        for rec in case.records:
            M.import_record(L, *M.record_key(case), *rec)
            for rep in range(2):
                rc = L.denet_conv_wgrad(ptr(t["x"]), ptr(t["dy"]), ptr(dw.arm()), ptr(ws), case.ws, *g, stream_ptr())
                assert rc == 0, (case.id, rec, rc, L.denet_last_error())
                _check_ran(L, case, rec)
                assert dw.intact()
                if rep == 0:
                    first = dw.t.clone()
                assert torch.equal(first, dw.t), (case.id, rec, "a repeated launch differs")
            _count("wgrad", 2, _err((case.id, rec), first, ref))
            assert not first[K - 5:].any() and not first[..., C - 3:].any(), (case.id, rec, "padding channels are not exact zeros")
            outs.setdefault(M.intended(case, rec)[3], {})[rec] = {"dw": first}
    for splits, same in outs.items():
        _same_bits(same, "%s, %d slices" % (case.id, splits))


# ---- the batched products of the un-fused F(2x2) route -------------------------------------------------------------------------------
def _traced(L, fn):
    """fn() with the launch trace on: its result and the (mode, bm, bn, nbuf) of the implicit-GEMM launches it made"""
    assert L.denet_conv_profile(2) == 0
    try:
        out = fn()
        n = L.denet_conv_profile_count()
        ms, v = ctypes.c_float(), [ctypes.c_int() for _ in range(4)]
        seen = []
        for i in range(n):
            assert L.denet_conv_profile_read(i, ctypes.byref(ms), *[ctypes.byref(x) for x in v]) == 0
            seen.append(tuple(x.value for x in v))
    finally:
        L.denet_conv_profile(0)
    return out, [s for s in seen if s[0] <= 3]


def test_batched_products(hip):
    """ops.conv_wino_fwd / _dgrad / _wgrad with tile = 2 at batch 2, 8 x 12, 64 -> 160 channels (48 tiles, 16 members; the fused
    F(2x2) kernel takes 64 -> 64 only): plan codes 3 and 4 under every record, the bounds test_conv_winograd_vs_direct holds the
    route to (2e-5, filter gradient 6e-5)"""
    from denet_amd import ops
    N, H, W, C, K = 2, 8, 12, 64, 160
    g = M.geom(N, H, W, C, K, 3, 1, 1)
    t = M.tensors(g)
    ref_y, ref_dx, ref_dw = M.ref_fwd(t, g), M.ref_dgrad(t, g), M.ref_wgrad(t, g)
    runs = (("gemm_b_fwd", lambda: ops.conv_wino_fwd(t["x"], t["w"], tile=2), ref_y, 2e-5),
            ("gemm_b_dgrad", lambda: ops.conv_wino_dgrad(t["dy"], t["w"], tile=2), ref_dx, 2e-5),
            ("wgrad_b", lambda: ops.conv_wino_wgrad(t["x"], t["dy"], tile=2), ref_dw, 6e-5))
    with _TunedTable() as L:
        for cid, fn, ref, bound in runs:
            case = M.BY_ID[cid]
            outs = {}
            for rec in case.records:
                M.import_record(L, *M.record_key(case), *rec)
                bm, bn, nbuf, _ = M.intended(case, rec)
                for rep in range(2):
                    out, seen = _traced(L, fn)
                    assert seen == [(M.KERNEL_MODE[case.code], bm, bn, nbuf)], (cid, rec, seen)
                    if rep == 0:
                        first = out.clone()
                    assert torch.equal(first, out), (cid, rec, "a repeated launch differs")
                _count(cid, 2, _err((cid, rec), first, ref, bound))
                outs[rec] = {"out": first}
            _same_bits(outs, cid)
