"""Batch normalisation (csrc/bn.hip, bn_reduce.h, bn_pointwise.h) restated in float64 on the host. A helper module: it holds no test.

The contract is the reference's layer (denet/layer/batch_norm.py, batch_norm_relu.py, resnet.py): x NHWC seen as [M][C], statistics
per channel over the M rows (BIASED variance, eps INSIDE the root), y = relu?(gamma * (x - mean) * inv + beta [+ res]), running
`mean` and `stdinv` updated as run <- m * run + (1 - m) * batch, the inference transform with the reference's double epsilon
inv = 1 / sqrt((1 / stdinv)^2 + eps). The ARBITER is `bn_ref64`: torch float64 on the CPU, the gradients by autograd.
`bn_closed64` is the closed-form backward the kernels implement, which the host test holds against autograd. `bn_restate32` is
the kernels' own float32 expressions in numpy: it measures what float32 costs (the constants K_Y, K_DX, K_G below) and is never
a reference for the device.

eps and momentum reach the library as C floats, so the references take float32(eps) and float32(momentum) widened: against a
channel whose variance is below eps the difference to the decimal 1e-5 (0.6 u relative) would eat a third of the 2 u bound.

Bounds (per channel, max norm, u = 2^-24): `bn_bounds`. The statistics bounds follow from the code (float64 sums, one correctly
rounded conversion). K_Y, K_DX, K_G are TWICE the worst ratio error / (bound with k = 1) that bn_restate32 showed against
bn_ref64 over the whole case table (tests/test_bn_reference_host.py::test_float32_cost_is_inside_the_constants measures them
again on every run and holds them under the constants), twice because numpy's operation order and the compiler's FMA contraction
differ."""
import collections

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-5

# measured worst ratios (host test, every case x mode x seed of the table below): y 2.299, dx 2.625, dgamma 2.837 (dgamma at the
# three rows of (1, 1, 3, 4), where sum |g * xhat| has three terms; 1.6 at most from (3, 5, 7, 24) on). The statistics for
# comparison, against bounds that need no constant: dbeta 0.47, mean 0.50, inv 0.50, running mean / stdinv 0.45
K_Y = 4.6
K_DX = 5.3
K_G = 5.7
# the largest share of undecided ReLU elements of a case the host test saw with these constants: 2.9e-5; the rule allows
UNDECIDED_MAX = 1e-3

# (N, H, W, C) of the kernel-level cases: what each is in the table for is asserted through bn_map by the host test
CASES = [(1, 1, 3, 4),          # M < RS, LC = 1
         (1, 1, 1, 64),         # M = 1
         (1, 20, 15, 12),       # LC = 1, gx = 3
         (3, 5, 7, 24),         # LC = 2, M < RS
         (1, 33, 33, 96),       # LC = 8: the last workgroup holds one row
         (1, 105, 104, 96),     # LC = 8, 2 sweeps
         (1, 80, 82, 160),      # LC = 8, gx = 5, 2 sweeps
         (2, 91, 91, 64),       # LC = 16, M = 16562, 2 sweeps
         (1, 47, 523, 128),     # LC = 32, M = 3 * 8192 + 5, 4 sweeps
         (1, 3, 455, 1536),     # LC = 128, M = 2 * 682 + 1, 3 sweeps, the last of one row
         (1, 25, 41, 2048),     # LC = 256, gx = 2, M = 512 + 512 + 1, 3 sweeps
         (1, 7, 100, 3072)]     # LC = 256, gx = 3, 3 sweeps
MODES = [(False, False), (True, False), (True, True), (False, True)]      # (relu, res)
MOMENTA = (0.9, 0.5, 0.0)
# (N, H, W, C, k, s, p) of the BN + ReLU + max pool cases
POOL_CASES = [(2, 92, 92, 64, 3, 2, 1),       # even map: the quad kernel; the POOL reduction takes 2 sweeps
              (1, 129, 129, 64, 3, 2, 1),     # odd map: the general POOL apply kernel takes 2 sweeps
              (3, 17, 23, 32, 3, 2, 1),
              (2, 16, 16, 128, 2, 2, 0),
              (1, 15, 15, 32, 3, 1, 1),
              (1, 1, 1, 32, 3, 2, 1),
              (1, 20, 15, 12, 3, 2, 1)]
FINAL_ROWS = (1, 31, 33, 97, 129, 2048)       # partial lists: the classes of bnf_reduce_partials
FOLD_ROWS = (2049, 2111, 4097, 16384)         # lists long enough for bn_stats_fold_kernel; 2111: a short last slice


def case_seed(ci, k=0):
    """the seed of case ci; k = 0 is the one the GPU test runs, the host test measures k = 1, 2 as well where the case is small"""
    return 100 * ci + k + 1


def case_momentum(ci, mi):
    """every momentum meets every mode and every mapping class somewhere in the table"""
    return MOMENTA[(ci + mi) % len(MOMENTA)]


BnMap = collections.namedtuple("BnMap", "LC RS gx gy sweeps")


def bn_map(M, C, target=1024):
    """csrc/bn_reduce.h: bn_map, and how often a workgroup's row loop runs: sweeps = ceil(M / (gy * RS))"""
    c4 = C // 4
    lc = 1
    while lc < 256 and c4 % (lc * 2) == 0:
        lc *= 2
    RS = 256 // lc
    gx = c4 // lc
    row_blocks = (M + RS - 1) // RS
    gy = min(max(target // gx, 1), row_blocks)
    return BnMap(lc, RS, gx, gy, -(-M // (gy * RS)))


def final_lane0(rows, lanes=32):
    """bnf_reduce_partials for the lane with jl = 0: (rounds of the four-loads-in-flight loop, rows added one by one after it,
    lanes that get no row at all)"""
    j, rounds = 0, 0
    while j + 3 * lanes < rows:
        rounds, j = rounds + 1, j + 4 * lanes
    tail = len(range(j, rows, lanes))
    return rounds, tail, max(lanes - rows, 0)


def fold_map(rows):
    """denet_bn_relu_pool_fwd_train's two-stage fold of a list of more than 2048 rows: (per, slices, rows of the last slice)"""
    per = (rows + 63) // 64
    slices = (rows + per - 1) // per
    return per, slices, rows - (slices - 1) * per


def bn_case(shape, seed, res=True):
    """float32 host tensors of one case: x = randn * 2 + 0.5 with channel 0 at std 1e-3 (variance below eps), channel 1 constant,
    channel 2 at mean = 300 * std; running statistics that start at non-trivial values. |beta| >= 0.5: a channel without spread
    (channel 1; every channel at M = 1) has pre = beta in every row, and the y bound is relative to the channel's max |pre|"""
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = torch.randn(shape, generator=g) * 2 + 0.5
    x[..., 0] = 0.5 + 1e-3 * torch.randn(shape[:-1], generator=g)
    x[..., 1] = 0.75
    x[..., 2] = 2.0 * (300.0 + torch.randn(shape[:-1], generator=g))
    gamma = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    beta = torch.where(b < 0, b - 0.5, b + 0.5)
    r = torch.randn(shape, generator=g) if res else None
    if res and x.numel() == C:
        # M = 1: a channel's only element is pre = beta + res, and the rounding of mean * gamma * inv (inv = 1 / sqrt(eps), not
        # small) does not shrink where the two cancel, as the y bound - relative to |pre| - would ask: res takes beta's sign
        r = r.abs() * torch.sign(beta)
    return {"x": x, "gamma": gamma, "beta": beta, "res": r,
            "dy": torch.randn(shape, generator=g), "run_mean": torch.randn(C, generator=g),
            "run_stdinv": torch.rand(C, generator=g) + 0.5}


def _d(t):
    return None if t is None else t.detach().double().cpu()


def bn_ref64(x, gamma, beta, eps, relu=False, res=None, dy=None, mask=None, run=None, momentum=0.9):
    """x, res, dy: [..., C] tensors of any float dtype; run = (run_mean, run_stdinv) before the pass. Returns a dict of float64
    tensors: y, pre (the value in front of the ReLU) [M, C]; mean, inv [C]; with run also run_mean, run_stdinv after the update;
    with dy also dx, dres (None without res), g (the gradient behind the ReLU), xhat [M, C] and dgamma, dbeta [C]. mask ([M, C] or
    x's shape, bool): the ReLU's decisions where the caller has them from elsewhere; the gradient then passes where mask is set
    instead of where pre > 0 (y stays relu(pre))"""
    C = x.shape[-1]
    eps = float(np.float32(eps))
    xd = _d(x).reshape(-1, C).requires_grad_(True)
    gd, bd = _d(gamma).requires_grad_(True), _d(beta).requires_grad_(True)
    rd = _d(res).reshape(-1, C).requires_grad_(True) if res is not None else None
    mean = xd.mean(dim=0)
    var = ((xd - mean) ** 2).mean(dim=0)                  # biased
    inv = 1.0 / torch.sqrt(var + eps)                     # eps inside the root
    pre = (xd - mean) * inv * gd + bd
    if rd is not None:
        pre = pre + rd                                    # the ReLU comes after the residual add
    passed = None
    if relu:
        passed = (pre.detach() > 0) if mask is None else mask.reshape(-1, C).cpu().bool()
    out = {"y": torch.relu(pre.detach()) if relu else pre.detach(), "pre": pre.detach(), "mean": mean.detach(), "inv": inv.detach()}
    if run is not None:
        m = float(np.float32(momentum))
        out["run_mean"] = m * _d(run[0]) + (1.0 - m) * out["mean"]
        out["run_stdinv"] = m * _d(run[1]) + (1.0 - m) * out["inv"]
        out["run_terms"] = [((m * _d(r)).abs() + ((1.0 - m) * out[k]).abs()) for r, k in zip(run, ("mean", "inv"))]
    if dy is not None:
        dyd = _d(dy).reshape(-1, C)
        y = pre * passed.double() if relu else pre
        y.backward(dyd)
        out.update(dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad, dres=rd.grad if rd is not None else None,
                   g=dyd * passed.double() if relu else dyd, xhat=((xd - mean) * inv).detach(), dy_max=dyd.abs().amax(dim=0))
    return out


def bn_closed64(x, gamma, beta, eps, relu=False, res=None, dy=None, mask=None):
    """the formulas the kernels implement, in numpy float64 on [M][C]: dx = gamma * inv * (g - mean(g) - xhat * mean(g * xhat)),
    dgamma = sum g * xhat, dbeta = sum g, dres = g, g = dy where the ReLU passed"""
    C = np.shape(x)[-1]
    x = np.asarray(x, np.float64).reshape(-1, C)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = x.mean(axis=0)
    inv = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=0) + np.float64(np.float32(eps)))
    xhat = (x - mean) * inv
    pre = xhat * gamma + beta
    if res is not None:
        pre = pre + np.asarray(res, np.float64).reshape(-1, C)
    out = {"y": np.maximum(pre, 0.0) if relu else pre, "pre": pre, "mean": mean, "inv": inv}
    if dy is not None:
        g = np.asarray(dy, np.float64).reshape(-1, C)
        if relu:
            g = g * ((pre > 0) if mask is None else np.asarray(mask, bool).reshape(-1, C))
        A, B = g.sum(axis=0), (g * xhat).sum(axis=0)
        out.update(dx=gamma * inv * (g - A / len(x) - xhat * (B / len(x))), dgamma=B, dbeta=A, dres=g if res is not None else None)
    return out


def bn_restate32(x, gamma, beta, eps, relu=False, res=None, dy=None, mask=None, run=None, momentum=0.9):
    """the kernels' expressions (bn_pointwise.h, bnf_finish_stats, bnf_finish_sums) in numpy float32, the reductions in float64,
    fmaf as a float64 product-sum rounded once. Same keys as bn_ref64, float32 arrays. ONLY a measure of what float32 costs"""
    f, d = np.float32, np.float64
    C = np.shape(x)[-1]
    x = np.asarray(x, f).reshape(-1, C)
    M = len(x)
    gamma, beta = np.asarray(gamma, f), np.asarray(beta, f)
    x64 = x.astype(d)
    mean = x64.sum(axis=0) / d(M)
    var = np.maximum((x64 * x64).sum(axis=0) / d(M) - mean * mean, 0.0)
    mu, inv = mean.astype(f), (1.0 / np.sqrt(var + d(f(eps)))).astype(f)
    sc = gamma * inv
    sh = beta - mu * sc
    pre = (x64 * sc.astype(d) + sh.astype(d)).astype(f)
    if res is not None:
        pre = pre + np.asarray(res, f).reshape(-1, C)
    y = np.maximum(pre, f(0)) if relu else pre
    out = {"y": y, "pre": pre, "mean": mu, "inv": inv}
    if run is not None:
        m = f(momentum)
        om = f(1.0 - d(m))
        out["run_mean"] = m * np.asarray(run[0], f) + om * mu
        out["run_stdinv"] = m * np.asarray(run[1], f) + om * inv
    if dy is not None:
        g = np.asarray(dy, f).reshape(-1, C)
        if relu:
            g = np.where((y > 0) if mask is None else np.asarray(mask, bool).reshape(-1, C), g, f(0))
        xh = (x - mu) * inv
        s, ss = g.astype(d).sum(axis=0), (g.astype(d) * xh.astype(d)).sum(axis=0)
        mg, mgx = (s / d(M)).astype(f), (ss / d(M)).astype(f)
        out.update(dx=sc * (g - mg - xh * mgx), dgamma=ss.astype(f), dbeta=s.astype(f), dres=g if res is not None else None)
    return out


def bn_bounds(ref, gamma, k_y=K_Y, k_dx=K_DX, k_g=K_G):
    """{quantity: per-channel bound [C] float64} of a bn_ref64 result (those of the backward pass where it holds one)"""
    ga = _d(gamma).abs()
    amp = 1.0 + ref["mean"].abs() * ref["inv"]
    b = {"mean": 2 * U * ref["mean"].abs(), "inv": 2 * U * ref["inv"], "y": k_y * U * amp * ref["pre"].abs().amax(dim=0)}
    if "run_terms" in ref:
        b["run_mean"], b["run_stdinv"] = 4 * U * ref["run_terms"][0], 4 * U * ref["run_terms"][1]
    if "dx" in ref:
        b["dx"] = k_dx * U * amp * ga * ref["inv"] * ref["dy_max"]
        b["dgamma"] = k_g * U * amp * (ref["g"] * ref["xhat"]).abs().sum(dim=0)
        b["dbeta"] = 2 * U * ref["g"].abs().sum(dim=0)
    return b


def ratios(got, ref, bounds, keys):
    """{key: worst error / bound over the tensor} (0 where both are 0; inf where an error stands against a zero bound)"""
    out = {}
    for k in keys:
        err = (_d(got[k] if torch.is_tensor(got[k]) else torch.from_numpy(np.ascontiguousarray(got[k]))).reshape(ref[k].shape) - ref[k]).abs()
        bd = bounds[k].expand_as(err)
        r = torch.where(err > 0, err / bd, torch.zeros_like(err))      # (x / 0 = inf for x > 0)
        out[k] = float(r.max()) if r.numel() else 0.0
    return out


def relu_decisions(pre, y_bound, passed_dev):
    """the mask rule: an element is UNDECIDED when |pre64| <= the y bound of its channel. Returns (mask, undecided, wrong): the
    float64 decisions with the device's own (passed_dev = y_dev > 0) on undecided elements, the undecided elements, and the
    DECIDED elements on which the device disagrees with float64 (there must be none)"""
    passed_dev = passed_dev.reshape(pre.shape).cpu().bool()
    und = pre.abs() <= y_bound
    want = pre > 0
    return torch.where(und, passed_dev, want), und, (~und) & (passed_dev != want)


def bn_test64(x, gamma, beta, run_mean, run_stdinv, eps, relu=False, res=None):
    """inference: the reference feeds var = (1 / stdinv)^2 to a transform that adds eps again. Returns y, pre [M, C], inv [C]"""
    C = x.shape[-1]
    inv = 1.0 / torch.sqrt((1.0 / _d(run_stdinv)) ** 2 + float(np.float32(eps)))
    pre = (_d(x).reshape(-1, C) - _d(run_mean)) * (_d(gamma) * inv) + _d(beta)
    if res is not None:
        pre = pre + _d(res).reshape(-1, C)
    return {"y": torch.relu(pre) if relu else pre, "pre": pre, "inv": inv}


def bn_test_bound(x, gamma, run_mean, ref, k_y=K_Y):
    """the y bound with the running statistics in place of the batch's, plus what the inference coefficient costs:
    bn_test_coef_kernel forms inv in float32 - 1 / stdinv (u), its square (2u + u), + eps (u), the root (halves: 2u, + u), the
    quotient (u): 4u relative on inv, which reaches y through gamma * (x - mean) * inv"""
    C = x.shape[-1]
    amp = 1.0 + _d(run_mean).abs() * ref["inv"]
    spread = ((_d(x).reshape(-1, C) - _d(run_mean)) * (_d(gamma) * ref["inv"])).abs().amax(dim=0)
    return k_y * U * amp * ref["pre"].abs().amax(dim=0) + 4 * U * spread


def bn_fold64(w, conv_bias, gamma, beta, run_mean, run_stdinv, eps):
    """conv(x, w) + b followed by the inference transform == conv(x, w * s[k]) + (beta - (mean - b) * s), s = gamma * inv.
    w: [K, ...]. Returns w_out, b_out, s, and the bias bound's scale |beta| + |mean - b| * |s|"""
    K = w.shape[0]
    inv = 1.0 / torch.sqrt((1.0 / _d(run_stdinv)) ** 2 + float(np.float32(eps)))
    s = _d(gamma) * inv
    b = _d(conv_bias) if conv_bias is not None else torch.zeros(K, dtype=torch.float64)
    return {"w": _d(w).reshape(K, -1) * s[:, None], "b": _d(beta) - (_d(run_mean) - b) * s, "s": s,
            "b_scale": _d(beta).abs() + (_d(run_mean) - b).abs() * s.abs()}


def pool_taps(H, W, k, s, p):
    """OH, OW and for each tap t = ky * k + kx the (rows, columns) it reads for every window, with their in-bounds flags"""
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    taps = []
    for ky in range(k):
        for kx in range(k):
            iy, ix = torch.arange(OH) * s - p + ky, torch.arange(OW) * s - p + kx
            taps.append((iy, ix, (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)))
    return OH, OW, taps


def pool_ref64(y, k, s, p, tol):
    """max pool of y [N, H, W, C] float64 (padded taps skipped). Returns (mx [N, OH, OW, C], vals [N, OH, OW, C, k * k] with -inf at
    out-of-bounds taps, near: the in-bounds taps whose value is within tol [C] of the window's maximum)"""
    N, H, W, C = y.shape
    OH, OW, taps = pool_taps(H, W, k, s, p)
    vals = torch.full((N, OH, OW, C, k * k), -float("inf"), dtype=torch.float64)
    for t, (iy, ix, oky, okx) in enumerate(taps):
        v = y[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
        ok = (oky[:, None] & okx[None, :])[None, :, :, None]
        vals[..., t] = torch.where(ok, v, vals[..., t])
    mx = vals.amax(dim=-1)
    return mx, vals, vals >= (mx - tol)[..., None]


def pool_route64(dyp, arg, shape, k, s, p):
    """the pooled gradient dyp [N, OH, OW, C] sent to the input pixel each window's tap `arg` names: float64 [N, H, W, C]. Every
    tap must be in bounds (the caller has checked it)"""
    N, H, W, C = shape
    OH, OW = dyp.shape[1:3]
    arg = arg.long().cpu()
    oy, ox = torch.arange(OH)[None, :, None, None], torch.arange(OW)[None, None, :, None]
    iy, ix = oy * s - p + arg // k, ox * s - p + arg % k
    n, c = torch.arange(N)[:, None, None, None], torch.arange(C)[None, None, None, :]
    flat = ((n * H + iy) * W + ix) * C + c
    out = torch.zeros(N * H * W * C, dtype=torch.float64)
    out.index_add_(0, flat.reshape(-1), _d(dyp).reshape(-1))
    return out.reshape(shape), flat


def split_partials(x_or_pairs, rows, rng):
    """a partial list float64 [rows][2][C] as another pass would leave it: the sums over `rows` disjoint, uneven row sets that
    cover all M rows; from three sets on about a third of them is empty (all-zero list rows), the first and the last never. x [M, C]: (sum x, sum x^2); a pair
    (a, b) of [M, C] tensors: (sum a, sum b), e.g. (g, g * xhat). rng: numpy RandomState"""
    if isinstance(x_or_pairs, (tuple, list)):
        a, b = (_d(t).reshape(-1, t.shape[-1]) for t in x_or_pairs)
    else:
        a = _d(x_or_pairs).reshape(-1, x_or_pairs.shape[-1])
        b = a * a
    M, C = a.shape
    live = rows if rows < 3 else rows - rows // 3
    sets = rng.permutation(rows)[:live]
    w = rng.random_sample(live) ** 3 + 1e-3
    owner = sets[rng.choice(live, size=M, p=w / w.sum())].astype(np.int64)
    owner[0], owner[-1] = 0, rows - 1          # the first and the LAST list row hold data: a reader that drops its tail is seen
    owner = torch.from_numpy(owner)
    out = torch.zeros(rows, 2, C, dtype=torch.float64)
    out[:, 0].index_add_(0, owner, a)
    out[:, 1].index_add_(0, owner, b)
    return out
