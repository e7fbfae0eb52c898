"""Grouped convolutions restated in float64 on the host. A helper module: it holds no test.

The contract ("Grouped convolutions"): a layer with g groups on C -> K channels has the reference-layout filter
(K, Cg, R, S), Cg = C / g, Kg = K / g; output channel k reads the input channels [(k // Kg) * Cg, (k // Kg + 1) * Cg) only. The
arbiter of the kernel checks is PyTorch's CPU `conv2d(..., groups=g)` in float64 on the flipped filter (conv64_grouped). A whole
model needs no restatement of its own: `dilated_reference.reference` takes every filter from `params`, so it is handed the DENSE
TWIN of a grouped filter, expand_ref(w, g) - the block-diagonal (K, C, R, S) filter whose off-diagonal blocks are zero - as a leaf
tensor, and the grouped gradient is compact_ref of the twin's gradient (the diagonal blocks). In float64 the twin's `conv2d` and
`conv2d(groups=)` agree exactly: the other blocks add zeros."""
import torch
import torch.nn.functional as Fn

from dilated_reference import conv_padding


def expand_ref(w_ref, g):
    """(K, Cg, R, S) -> the block-diagonal dense (K, Cg * g, R, S): rows of group i = k // (K / g) hold w_ref in the channels
    [i * Cg, (i + 1) * Cg) and zeros elsewhere"""
    K, Cg, R, S = w_ref.shape
    assert K % g == 0, (K, g)
    Kg = K // g
    out = torch.zeros(K, Cg * g, R, S, dtype=w_ref.dtype)
    for i in range(g):
        out[i * Kg:(i + 1) * Kg, i * Cg:(i + 1) * Cg] = w_ref[i * Kg:(i + 1) * Kg]
    return out


def compact_ref(dw_dense, g):
    """the inverse of expand_ref on the diagonal blocks: (K, C, R, S) -> (K, C / g, R, S)"""
    K, C, R, S = dw_dense.shape
    assert K % g == 0 and C % g == 0, (K, C, g)
    Kg, Cg = K // g, C // g
    out = torch.zeros(K, Cg, R, S, dtype=dw_dense.dtype)
    for i in range(g):
        out[i * Kg:(i + 1) * Kg] = dw_dense[i * Kg:(i + 1) * Kg, i * Cg:(i + 1) * Cg]
    return out


def conv64_grouped(h, w_ref, stride, border, g):
    """float64 conv2d with g groups of the reference-layout filter w_ref (K, Cg, R, S): a true convolution, the filter is flipped"""
    R, S = w_ref.shape[2:]
    y = Fn.conv2d(h, w_ref.flip(2, 3), stride=tuple(stride), padding=conv_padding(border, R, S), groups=g)
    if border == "same":
        y = y[:, :, :h.shape[2], :h.shape[3]]
    return y
