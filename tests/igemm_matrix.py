"""Every instantiation of csrc/igemm.hip's one kernel text (4 modes x their tiles x the loop structures NBUF = 1, 2, 3: 27 kernels)
at the smallest geometries that reach the edges of its loops - shared by tests/test_igemm_matrix_host.py (the plans, no device)
and tests/test_igemm_matrix_gpu.py (the launches): the case table, the float64 references (CPU), the record import and the read
back of what ran. Also home of the three helpers tests/test_kernels_gpu.py drives the C ABI with.

Run as a script (`python tests/igemm_matrix.py --dgrad-t-child OUT.npz`) it is the child process of the MODE_DGRAD_T cases that
only DENET_DGRAD_T_NBUF / DENET_DGRAD_T_TILE reach: the switches are read once per process."""
import ctypes
import os
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BK = 32                                                  # reduction chunk of the kernel
FWD, DGRAD, WGRAD, GEMM_B, WGRAD_B, DGRAD_T, DGRAD_1X1T = range(7)        # denet_conv_plan's pass codes
KERNEL_MODE = {FWD: 0, DGRAD: 1, WGRAD: 2, GEMM_B: 0, WGRAD_B: 2, DGRAD_T: 3, DGRAD_1X1T: 0}   # MODE of the kernel a pass runs
TILES = {0: ((128, 128), (128, 64)), 1: ((128, 128), (128, 64)), 3: ((128, 128), (128, 64)), 2: ((128, 128), (64, 64), (64, 128))}
INSTANTIATIONS = {(m, bm, bn, nb) for m, tl in TILES.items() for bm, bn in tl for nb in (1, 2, 3)}
assert len(INSTANTIATIONS) == 27


# ---- the helpers of tests/test_kernels_gpu.py ------------------------------------------------------------------------------------
class _TunedTable:
    """the process's table of measured launch configurations, emptied for the test and put back afterwards"""

    def __enter__(self):
        import ctypes
        from denet_amd import ops
        self.L = ops._L()
        self.n = self.L.denet_tune_export(None, 0)
        self.saved = (ctypes.c_int * (14 * max(self.n, 1)))()
        assert self.L.denet_tune_export(self.saved, self.n) == self.n
        assert self.L.denet_tune_clear() == 0
        return self.L

    def __exit__(self, *exc):
        assert self.L.denet_tune_clear() == 0
        assert self.L.denet_tune_import(self.saved, self.n) == 0
        assert self.L.denet_tune_export(None, 0) == self.n


def _igemm_pass(L, code, g, t, ws_bytes):
    """runs pass `code` (denet_conv_plan's codes) of geometry g on the tensors t through the C ABI; returns the output tensor"""
    from denet_amd.ops import ptr, stream_ptr
    N, H, W, C, K = g[:5]
    if code == 0:
        rc, out = L.denet_conv_fwd(ptr(t["x"]), ptr(t["w"]), None, None, ptr(t["y"]), *g, stream_ptr()), t["y"]
    elif code == 1:
        rc, out = L.denet_conv_dgrad(ptr(t["dy"]), ptr(t["w"]), None, ptr(t["dx"]), *g, stream_ptr()), t["dx"]
    elif code == 5:
        rc, out = L.denet_conv_dgrad_t(ptr(t["dy"]), ptr(t["wt"]), None, ptr(t["dx"]), None, None, 0, None, *g, stream_ptr()), t["dx"]
    elif code == 6:
        rc, out = L.denet_conv_dgrad_1x1t(ptr(t["dy"]), ptr(t["wt"]), None, ptr(t["dx"]), None, None, 0, None, N, H, W, C, K,
                                          stream_ptr()), t["dx"]
    else:
        rc, out = L.denet_conv_wgrad(ptr(t["x"]), ptr(t["dy"]), ptr(t["dw"]), ptr(t["ws"]), ws_bytes, *g, stream_ptr()), t["dw"]
    assert rc == 0, (code, g, rc, L.denet_last_error())
    return out


def _igemm_tensors(g, seed):
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = g
    gen = torch.Generator().manual_seed(seed)
    t = {"x": torch.randn(N, H, W, C, generator=gen).cuda(), "w": (torch.randn(K, R, S, C, generator=gen) * 0.1).cuda(),
         "dy": torch.randn(N, OH, OW, K, generator=gen).cuda()}
    t["wt"] = t["w"].reshape(K, R * S * C).t().contiguous()            # [R][S][C][K]
    t["y"], t["dx"], t["dw"] = torch.empty_like(t["dy"]), torch.empty_like(t["x"]), torch.empty_like(t["w"])
    t["ws"] = torch.empty(64 * t["w"].numel(), device="cuda")            # room for 64 split slices
    return t


# ---- the case table ----------------------------------------------------------------------------------------------------------------
# id; code: the pass (denet_conv_plan's codes); g: the 12 geometry ints of the C ABI (a batched product: its batched_geom);
# batch: members of a batched product, else 1; ws: bytes of split workspace the filter gradient is given (0: none);
# records: the (tile, nbuf, rounds) imported one after another under the row's key; want: what the row is there for -
#   filter gradients (bm, bn, splits), MODE_DGRAD_T (bn, nbuf) - its rule or, with `switch`, the switches decide, no record;
# switch: (DENET_DGRAD_T_TILE, DENET_DGRAD_T_NBUF) of the child process a MODE_DGRAD_T row runs in, None: this process
Case = namedtuple("Case", "id code g batch ws records want switch")

ALL6 = [(tile, nbuf, 0) for tile in (0, 1) for nbuf in (1, 2, 3)]
NARROW = [(0, 3, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0)]       # fewer than 128 columns: 128 x 64 whatever tile the record asks for
WG9 = [(0, nbuf, rounds) for nbuf in (1, 2, 3) for rounds in (1, 2, 6)]
DGRAD_T_CHILDREN = [(1, 1), (1, 3), (2, 3), (1, 2)]        # 128x128 / 1, 128x128 / 3, 128x64 / 3, 128x128 / 2 (at a short reduction)


def geom(N, H, W, C, K, R, stride=1, pad=0):
    return (N, H, W, C, K, R, R, R, stride, pad, (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1)


def batched_geom(rows, C, K):
    return (1, 1, rows, C, K, 1, 1, 1, 1, 0, 1, rows)


def _cases():
    rows = []

    def add(id, code, g, records, want=None, batch=1, ws=0, switch=None):
        rows.append(Case(id, code, g, batch, ws, list(records), want, switch))

    # forward: 198 rows = one full tile + 70; 160 columns = 128 + 32 or 64 + 64 + 32; 1 ... 5 chunks, then 9 and 18
    for C in (32, 64, 96, 128, 160):
        add("fwd_1x1_c%d" % C, FWD, geom(2, 9, 11, C, 160, 1), ALL6)
    add("fwd_3x3_c32", FWD, geom(2, 9, 11, 32, 160, 3, 1, 1), ALL6)              # a new tap every chunk, padding at every border
    add("fwd_3x3_c64_k96", FWD, geom(2, 9, 11, 64, 96, 3, 1, 1), NARROW)         # two chunks per tap; 96 columns = 64 + 32
    add("fwd_3x3_35rows_k32", FWD, geom(1, 5, 7, 32, 32, 3, 1, 1), NARROW)       # fewer rows than a tile
    add("fwd_1x1_35rows", FWD, geom(1, 5, 7, 64, 160, 1), ALL6)                  # the same on the 128 x 128 tile
    add("fwd_3x3_s2", FWD, geom(2, 10, 12, 64, 160, 3, 2, 1), ALL6)
    # data gradient: the columns are C = 160; the reduction runs over K
    dg = [("1x1_k%d" % K, geom(2, 9, 11, 160, K, 1)) for K in (32, 64, 96, 128, 160)]
    dg += [("3x3_k32", geom(2, 9, 11, 160, 32, 3, 1, 1)),
           ("3x3_s2_k32", geom(5, 10, 12, 160, 32, 3, 2, 1)),                    # 150 rows per parity class, 1 / 2 / 2 / 4 taps
           ("3x3_s2_k64", geom(5, 10, 12, 160, 64, 3, 2, 1)),
           ("1x1_s2", geom(2, 10, 12, 160, 64, 1, 2, 0)),                        # three classes without a tap: 0 steps
           ("2x2_s2", geom(2, 10, 12, 160, 32, 2, 2, 0)),                        # one tap per class
           ("3x3_s2_k384", geom(2, 10, 12, 160, 384, 3, 2, 1)),                  # 27 chunks per class on average: MODE_DGRAD_T pipelines
           ("3x3_k96", geom(2, 9, 11, 160, 96, 3, 1, 1))]                        # 27 chunks
    for name, g in dg:
        add("dgrad_" + name, DGRAD, g, ALL6)
    for name, g in dg:
        add("dgrad_t_" + name, DGRAD_T, g, [], want=(64, 2 if name in ("3x3_s2_k384", "3x3_k96") else 1))
    for tile, nbuf in DGRAD_T_CHILDREN:
        for name, g in dg:
            add("dgrad_t%d%d_%s" % (tile, nbuf, name), DGRAD_T, g, [], want=(128 if tile == 1 else 64, nbuf), switch=(tile, nbuf))
    for name, g in dg[:5]:
        add("dgrad_1x1t_" + name[4:], DGRAD_1X1T, g, ALL6)
    # filter gradient: (K, C, R) fixes the tile; the pixels fix chunks and slices
    def wg(name, N, H, W, K, C, R, stride, with_ws, splits):
        g = geom(N, H, W, C, K, R, stride, 1 if R == 3 else 0)
        cols = R * R * C
        add("wgrad_k%d_c%d_r%d_%s" % (K, C, R, name), WGRAD, g, WG9, ws=64 * K * cols * 4 if with_ws else 0,
            want=(128 if K >= 128 else 64, 64 if K < 128 and cols <= 64 else 128, splits))

    for K, C, R in ((160, 32, 3), (64, 64, 1), (64, 96, 1), (64, 32, 3)):
        wg("n3", 3, 9, 11, K, C, R, 1, True, 2)                   # 297 pixels: 10 chunks, slices of 5 + 5, the last chunk 9 pixels
        wg("n4", 4, 9, 11, K, C, R, 1, True, 3)                   # 396 pixels: 13 chunks as 5 + 5 + 3, the last chunk 12 pixels
        wg("n4_nows", 4, 9, 11, K, C, R, 1, False, 1)             # one slice of 13
        wg("5x6", 1, 5, 6, K, C, R, 1, True, 1)                   # 30 pixels: one partial chunk
        wg("5x7", 1, 5, 7, K, C, R, 1, True, 1)                   # 35 pixels: 2 chunks
        wg("9x11", 1, 9, 11, K, C, R, 1, True, 1)                 # 99 pixels: 4 chunks
    for K, C in ((96, 64), (32, 64), (96, 96), (32, 96), (64, 32)):       # 64-row tiles: 64 + 32 rows, 32 rows; 32 of 64 columns
        wg("n3", 3, 9, 11, K, C, 1, 1, True, 2)
    wg("s2", 3, 10, 12, 160, 32, 3, 2, True, 1)                   # 90 pixels of a strided output: 3 chunks
    # the batched products of the un-fused F(2x2) route: 16 members, 48 tile rows, 64 -> 160 channels
    add("gemm_b_fwd", GEMM_B, batched_geom(48, 64, 160), ALL6, batch=16)
    add("gemm_b_dgrad", GEMM_B, batched_geom(48, 160, 64), NARROW, batch=16)
    add("wgrad_b", WGRAD_B, batched_geom(48, 64, 160), [(tile, nbuf, 1) for tile in (0, 1) for nbuf in (1, 2, 3)], batch=16,
        ws=64 * 16 * 160 * 64 * 4, want=(128, 128, 1))
    assert len({r.id for r in rows}) == len(rows)
    return rows


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def cases_of(code, switch=False):
    return [c for c in CASES if c.code == code and (c.switch is not None) == switch]


def rows_cols(case):
    """GEMM rows (of one parity class / batch member) and columns of the launch"""
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = case.g
    if case.code in (FWD, GEMM_B):
        return N * OH * OW, K
    if case.code in (DGRAD, DGRAD_T, DGRAD_1X1T):
        return N * (H // stride) * (W // stride), C
    return K, R * S * C


def intended(case, rec):
    """(bm, bn, nbuf, splits) the row's record (None for MODE_DGRAD_T) is there to run"""
    cols = rows_cols(case)[1]
    stride = case.g[8]
    if case.code in (WGRAD, WGRAD_B):
        return (case.want[0], case.want[1], min(rec[1], 3), case.want[2])
    if case.code == DGRAD_T:
        return (128, case.want[0], case.want[1], stride * stride)
    bn = 128 if rec[0] == 0 and cols >= 128 else 64
    return (128, bn, min(rec[1], 3), {FWD: 1, DGRAD: stride * stride, DGRAD_1X1T: 1, GEMM_B: case.batch}[case.code])


def steps(case, splits=1):
    """the reduction chunks of every kind of workgroup of the launch: one entry per parity class (data gradients) or split slice
    (filter gradients)"""
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = case.g
    if case.code in (FWD, GEMM_B):
        return [R * S * C // BK]
    if case.code == DGRAD_1X1T:
        return [K // BK]
    if case.code in (DGRAD, DGRAD_T):
        out = []
        for py in range(stride):
            for px in range(stride):
                r0, s0 = (py + pad) % stride, (px + pad) % stride
                rc = -(-(R - r0) // stride) if R > r0 else 0
                sc = -(-(S - s0) // stride) if S > s0 else 0
                out.append(rc * sc * (K // BK))
        return out
    npix = W if case.code == WGRAD_B else N * OH * OW
    ksteps = -(-npix // BK)
    per = -(-ksteps // splits)
    return [min(per, ksteps - i * per) for i in range(splits)]


def npix(case):
    return case.g[2] if case.code == WGRAD_B else case.g[0] * case.g[10] * case.g[11]


def record_key(case):
    """(mode, the 10 geometry ints) a record of this row is imported under; None: the pass reads no record"""
    N, H, W, C, K = case.g[:5]
    if case.code in (FWD, DGRAD, WGRAD):
        return case.code, tuple(case.g[:10])
    if case.code == DGRAD_1X1T:                                   # the forward key with C and K swapped
        return 0, (N, H, W, K, C, 1, 1, 1, 1, 0)
    if case.code in (GEMM_B, WGRAD_B):
        return case.code, (case.batch, 1, W, C, K, 1, 1, 1, 1, 0)
    return None


def import_record(L, mode, geom10, tile, nbuf, rounds):
    rec = (ctypes.c_int * 14)(mode, *geom10, tile, nbuf, rounds)
    assert L.denet_tune_import(rec, 1) == 0, L.denet_last_error()


def plan(L, case):
    v = [ctypes.c_int() for _ in range(4)]
    rc = L.denet_conv_plan(case.code, *case.g, case.batch, case.ws, *[ctypes.byref(x) for x in v])
    assert rc == 0, (case.id, rc, L.denet_last_error())
    return tuple(x.value for x in v)


def ran(L):
    """denet_conv_last_config: [mode, bm, bn, nbuf, splits] of the last launch of this thread"""
    v = [ctypes.c_int() for _ in range(5)]
    assert L.denet_conv_last_config(*[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]


# ---- tensors and float64 references (CPU) ------------------------------------------------------------------------------------------
def seed_of(g):
    return zlib.crc32(repr(tuple(g)).encode()) & 0xFFFF


def tensors(g):
    """_igemm_tensors seeded by the geometry (a child process makes the same ones) + bias and the two epilogue addends"""
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = g
    t = _igemm_tensors(g, seed_of(g))
    gen = torch.Generator().manual_seed(seed_of(g) + 7919)
    t["bias"] = torch.randn(K, generator=gen).cuda()
    t["add_y"] = torch.randn(N, OH, OW, K, generator=gen).cuda()
    t["add_x"] = torch.randn(N, H, W, C, generator=gen).cuda()
    return t


def _nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def ref_fwd(t, g):
    """float64 NHWC: the filters are KRSC and already flipped - the kernel computes a correlation, as conv2d does"""
    stride, pad = g[8], g[9]
    return Fn.conv2d(_nchw64(t["x"]), _nchw64(t["w"]), None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def ref_dgrad(t, g):
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = g
    out = Fn.conv_transpose2d(_nchw64(t["dy"]), _nchw64(t["w"]), stride=stride, padding=pad,
                              output_padding=((H + 2 * pad - R) % stride, (W + 2 * pad - S) % stride))
    assert tuple(out.shape) == (N, C, H, W)
    return out.permute(0, 2, 3, 1).contiguous()


def ref_wgrad(t, g):
    N, H, W, C, K, R, S, _, stride, pad, OH, OW = g
    return torch.nn.grad.conv2d_weight(_nchw64(t["x"]), (K, C, R, S), _nchw64(t["dy"]), stride=stride,
                                       padding=pad).permute(0, 2, 3, 1).contiguous()


def rel_err(a, b64):
    """max|a - b| / max|b| against a float64 CPU tensor"""
    return float((a.detach().double().cpu() - b64).abs().max() / b64.abs().max())


SENTINEL = -1.2345e30


class Guarded:
    """an output tensor inside a larger buffer filled with a sentinel: arm() before a launch, intact() after it"""
    GUARD = 1024

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + 2 * self.GUARD, dtype=dtype, device="cuda")
        self.t = self.buf[self.GUARD:self.GUARD + n].view(*shape)

    def arm(self):
        self.buf.fill_(SENTINEL)
        return self.t

    def intact(self):
        return bool((self.buf[:self.GUARD] == SENTINEL).all()) and bool((self.buf[-self.GUARD:] == SENTINEL).all())


# ---- the child process of the switch-only MODE_DGRAD_T cases -----------------------------------------------------------------------
def _dgrad_t_child(path):
    """every data-gradient geometry of the table through denet_conv_dgrad_t under this process's DENET_DGRAD_T_* switches: dx,
    dx + add and what ran, into an .npz the parent compares with its own MODE_DGRAD results"""
    import numpy as np
    from denet_amd import ops
    from denet_amd.ops import ptr, stream_ptr
    assert torch.cuda.is_available(), "the child needs the GPU its parent has"
    L = ops._L()
    out = {}
    for case in cases_of(DGRAD_T):
        t = tensors(case.g)
        dx = Guarded(t["dx"].shape)
        for key, addt in (("dx", None), ("dxa", t["add_x"])):
            rc = L.denet_conv_dgrad_t(ptr(t["dy"]), ptr(t["wt"]), ptr(addt), ptr(dx.arm()), None, None, 0, None, *case.g, stream_ptr())
            assert rc == 0, (case.id, rc, L.denet_last_error())
            out["cfg_" + case.id[8:]] = np.array(ran(L), dtype=np.int32)
            torch.cuda.synchronize()
            assert dx.intact(), case.id
            out[key + "_" + case.id[8:]] = dx.t.cpu().numpy().copy()
    np.savez(path, **out)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--dgrad-t-child", sys.argv
    _dgrad_t_child(sys.argv[2])
