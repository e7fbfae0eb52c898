"""Float64 numpy restatement of the opt-in focal costs (csrc/focal.hip) and of their gradients, evaluated on
the fp32 inputs the kernels read. The reference implementation has no such mode: this file and the section are the contract.
Shared by tests/test_focal_host.py (which checks the gradients here against central differences of the costs here) and
tests/test_focal_gpu.py."""
import numpy as np

LN2 = np.log(2.0)


# ---- corner map ---------------------------------------------------------------------------------------------------------------

def corner_logpr(x):
    """the two log-probabilities of the softmax over [x, -x]: l0 = -log(1 + exp(-2x)), l1 = -log(1 + exp(2x)), float64"""
    x = np.asarray(x, np.float64)
    return -np.logaddexp(0.0, -2.0 * x), -np.logaddexp(0.0, 2.0 * x)


def corner_focal(l0, l1, t0, t1, gamma, cost_factor, batch):
    """(cost, dcost/dx) of the focal corner cost; l_k, t_k of any one shape, dcost/dx of the same shape.
    cost = cost_factor / (B ln 2) * sum -(t0 p1^g l0 + t1 p0^g l1); p_k^g = exp(g l_k), never 1 - p"""
    l0, l1, t0, t1 = (np.asarray(a, np.float64) for a in (l0, l1, t0, t1))
    p0, p1 = np.exp(l0), np.exp(l1)
    w0, w1 = np.exp(gamma * l1), np.exp(gamma * l0)
    scale = cost_factor / (batch * LN2)
    cost = scale * -np.sum(t0 * w0 * l0 + t1 * w1 * l1)
    grad = scale * (t0 * w0 * (2.0 * gamma * p0 * l0 - 2.0 * p1) + t1 * w1 * (2.0 * p0 - 2.0 * gamma * p1 * l1))
    return cost, grad


def corner_plain(l0, l1, t0, t1, cost_factor, batch):
    """the plain cost and gradient as dss.hip's corner_loss_kernel states them"""
    l0, l1, t0, t1 = (np.asarray(a, np.float64) for a in (l0, l1, t0, t1))
    p0, p1 = np.exp(l0), np.exp(l1)
    scale = cost_factor / (batch * LN2)
    return scale * -np.sum(t0 * l0 + t1 * l1), scale * ((t0 + t1) * (p0 - p1) - (t0 - t1))


def corner_layout(pr, tgt):
    """[B, 2, Cn, H, W] arrays of the layer -> (l0, l1, t0, t1), each [B, H, W, Cn]: the layout of dconv's corner channels"""
    pr, tgt = np.asarray(pr), np.asarray(tgt).reshape(np.asarray(pr).shape)
    nhwc = lambda a: a.transpose(0, 2, 3, 1)
    return nhwc(pr[:, 0]), nhwc(pr[:, 1]), nhwc(tgt[:, 0]), nhwc(tgt[:, 1])


# ---- detection head, class part -----------------------------------------------------------------------------------------------

def class_logpr(z):
    """log-softmax lp, p = exp(lp) and q = 1 - p of the rows of z in float64, without cancellation: q_c is the sum of the OTHER
    classes' probabilities (all terms >= 0), and lp_c = log1p(-q_c) where p_c is the large one"""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    se = e.sum(1, keepdims=True)
    n = z.shape[1]
    q = (e @ (1.0 - np.eye(n))) / se
    lp_direct = (z - z.max(1, keepdims=True)) - np.log(se)
    lp = np.where(q < 0.5, np.log1p(-np.minimum(q, 0.5)), lp_direct)
    return lp, np.exp(lp), q


def detect_focal(z, t, gamma, cost_factor, batch):
    """(DET cost, dcost/dz) of the focal class cost over logits z [M, ncls] with soft targets t [M, ncls]:
    det_err = -sum_c t_c q_c^g lp_c / ln(ncls), cost = cost_factor * sum(det_err) / batch"""
    t = np.asarray(t, np.float64)
    lp, p, q = class_logpr(z)
    ncls = t.shape[1]
    w = q ** gamma
    cost = cost_factor / batch * np.sum(-(t * w * lp)) / np.log(ncls)
    qg1 = q ** (gamma - 1.0) if gamma != 0.0 else np.zeros_like(q)         # (its factor gamma is 0 then; q may be 0)
    a = t * (w - gamma * qg1 * p * lp)
    A = a.sum(1, keepdims=True)
    return cost, cost_factor / batch / np.log(ncls) * (p * A - a)


def detect_plain(z, t, cost_factor, batch):
    """the plain class cost and gradient as dss.hip's detect_loss_kernel states them"""
    t = np.asarray(t, np.float64)
    lp, p, _ = class_logpr(z)
    ncls = t.shape[1]
    cost = cost_factor / batch * np.sum(-(t * lp)) / np.log(ncls)
    return cost, cost_factor / batch / np.log(ncls) * (t.sum(1, keepdims=True) * p - t)


# ---- the tolerance of the kernel tests (the form of test_corner_fwd_loss / test_detect_loss) -------------------------------------

def grad_ratio(got, ref):
    """largest |err| / bound, bound = 1e-4 * max|ref| + 1e-4 * |ref| element-wise"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = 1e-4 * np.abs(ref).max() + 1e-4 * np.abs(ref)
    return float(np.max(np.abs(got - ref) / bound))


def cost_ratio(got, ref):
    """|err| / (1e-4 * |ref|)"""
    return float(abs(float(got) - float(ref)) / (1e-4 * abs(float(ref))))
