// Opt-in bilinear RoI sampling of the DNS layer (tapRule 2, `DNS.I`). The reference has no counterpart: it
// reads every tap from the nearest cell (denet/layer/denet_sparse.py:72-84, denet_sparse_op.py:65-71; csrc/dss.hip here).
//   sparse_bilinear_fwd_kernel   a tap reads its four surrounding cells, weighted (1 - t, t) per axis
//   sparse_bilinear_bwd_kernel   a cell sums weight * dy row over the (roi, tap, corner) slots that read it, in ascending slot order
// The slots are grouped by cell with the counting sort of dss.hip (denet_sparse_sort sees n keys per image and nothing else; it is
// called with 4 * rois_per_image): no second sort, no floating-point atomics, bit-identical from run to run.
// The gradient kernel's body and the sort workspace's layout are the default path's own (dss.h).
// This file is compiled with -ffp-contract=off: coordinates, weights and sums are defined operation by operation.
#include "dss.h"
#include "../../include/denet_hip.h"
#include <limits.h>

namespace {

// one axis of a tap: rule 0's coordinate (dss.hip tap_index) BEFORE rounding, its two cells and their weights
__device__ __forceinline__ void tap_axis(float p0, float extent, int i, int gs, int size, int* i0, int* i1, float* w0, float* w1) {
    const float p = p0 + ((float)i * extent) / (float)(gs - 1);
    float f = p * (float)size;
    f = fmaxf(0.0f, fminf(f, (float)size - 1.0f));       // (a NaN coordinate lands on size - 1: always a cell of the map)
    const float fl = floorf(f);
    const float t = f - fl;                               // exact in fp32
    *i0 = (int)fl;
    *i1 = min(*i0 + 1, size - 1);                         // far border: i0 = size - 1, t = 0
    *w0 = 1.0f - t;
    *w1 = t;
}

// One workgroup per RoI. out = ((w00 * v00 + w01 * v01) + w10 * v10) + w11 * v11, w_qr = wy_q * wx_r: every product and every
// sum rounded to fp32, in this association.
template <bool VEC>
__global__ __launch_bounds__(256) void sparse_bilinear_fwd_kernel(const float* __restrict__ fmap, const float* __restrict__ bbox,
                                                                  float* __restrict__ out, int* __restrict__ taps4,
                                                                  float* __restrict__ wts4, int H, int W, int CP, int coff, int F,
                                                                  int rois_per_image, int gs, int KP) {
    __shared__ int s_cell[256 * 4];
    __shared__ float s_w[256 * 4];
    const int m = blockIdx.x;
    const int b = m / rois_per_image;
    const int ntap = gs * gs;
    const float x0 = bbox[m * 4 + 0], y0 = bbox[m * 4 + 1], x1 = bbox[m * 4 + 2], y1 = bbox[m * 4 + 3];
    const float bw = x1 - x0, bh = y1 - y0;
    if ((int)threadIdx.x < ntap) {
        const int yi = threadIdx.x / gs, xi = threadIdx.x - yi * gs;
        int ya, yb, xa, xb;
        float wya, wyb, wxa, wxb;
        tap_axis(y0, bh, yi, gs, H, &ya, &yb, &wya, &wyb);
        tap_axis(x0, bw, xi, gs, W, &xa, &xb, &wxa, &wxb);
        const int c[4] = {ya * W + xa, ya * W + xb, yb * W + xa, yb * W + xb};
        const float w[4] = {wya * wxa, wya * wxb, wyb * wxa, wyb * wxb};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s_cell[threadIdx.x * 4 + q] = c[q];
            s_w[threadIdx.x * 4 + q] = w[q];
        }
        if (taps4) {
            const long at = ((long)m * ntap + threadIdx.x) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                taps4[at + q] = c[q];
                wts4[at + q] = w[q];
            }
        }
    }
    __syncthreads();
    float* o = out + (long)m * KP;
    const float* fb = fmap + (long)b * H * W * CP + coff;
    if (VEC) {
        const int F4 = F / 4;
        for (int idx = threadIdx.x; idx < ntap * F4; idx += 256) {
            const int tap = idx / F4, f4 = idx - tap * F4;
            const int* c = s_cell + tap * 4;
            const float* w = s_w + tap * 4;
            const f32x4 v0 = *(const f32x4*)(fb + (long)c[0] * CP + f4 * 4);
            const f32x4 v1 = *(const f32x4*)(fb + (long)c[1] * CP + f4 * 4);
            const f32x4 v2 = *(const f32x4*)(fb + (long)c[2] * CP + f4 * 4);
            const f32x4 v3 = *(const f32x4*)(fb + (long)c[3] * CP + f4 * 4);
            *(f32x4*)(o + (long)idx * 4) = ((w[0] * v0 + w[1] * v1) + w[2] * v2) + w[3] * v3;
        }
    } else {
        for (int idx = threadIdx.x; idx < ntap * F; idx += 256) {
            const int tap = idx / F, f = idx - tap * F;
            const int* c = s_cell + tap * 4;
            const float* w = s_w + tap * 4;
            const float v0 = fb[(long)c[0] * CP + f], v1 = fb[(long)c[1] * CP + f];
            const float v2 = fb[(long)c[2] * CP + f], v3 = fb[(long)c[3] * CP + f];
            o[idx] = ((w[0] * v0 + w[1] * v1) + w[2] * v2) + w[3] * v3;
        }
    }
    // as sparse_fwd_kernel: channel gs*gs*F = box height, +1 = box width; the rest is K padding
    for (int k = ntap * F + threadIdx.x; k < KP; k += 256)
        o[k] = (k == ntap * F) ? bh : (k == ntap * F + 1) ? bw : 0.f;
}

// One wave per feature-map cell: sparse_bwd_kernel's cell sum (dss.h sparse_cell_sum) with a weight per slot. Entry j of the cell's
// list belongs to lane group j % epi, epi = 64 / (F / 4); a group adds weight * row (the product rounded, then the sum) left to
// right from +0; the groups are added in order.
__global__ __launch_bounds__(256) void sparse_bilinear_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ order,
                                                                  const int* __restrict__ cell_start,
                                                                  const float* __restrict__ wts4, float* __restrict__ dfmap,
                                                                  int HW, int CP, int coff, int F, int rois_per_image, int ntap,
                                                                  int KP, int zero_from, long ncell_total) {
    sparse_cell_sum<true>(dy, order, cell_start, wts4, dfmap, HW, CP, coff, F, rois_per_image, ntap, KP, zero_from, ncell_total);
}

// the expanded list (four slots per tap) in the terms of denet_sparse_sort: rois_per_image * 4 "RoIs" of gs * gs keys
int expanded_rois(const char* who, int B, int H, int W, int rois_per_image, int gs, int* rois4) {
    DENET_CHECK_ARG(B > 0 && H > 0 && W > 0 && rois_per_image > 0 && gs >= 2 && gs * gs <= 256,
                    "%s: bad arguments (B = %d, map %d x %d, %d RoIs per image, grid size %d)", who, B, H, W, rois_per_image, gs);
    DENET_CHECK_ARG((long)H * W <= 32768, "%s: feature map of %d x %d cells exceeds the 32768 cells of the grouping", who, H, W);
    DENET_CHECK_ARG((long)rois_per_image * 4 * gs * gs <= INT_MAX / 4, "%s: %d RoIs per image are too many slots", who, rois_per_image);
    *rois4 = rois_per_image * 4;
    return DENET_OK;
}

}  // namespace

extern "C" int denet_sparse_bilinear_fwd(const float* fmap, const float* bbox, float* out, int* taps4, float* wts4, int B, int H,
                                         int W, int CP, int coff, int F, int rois_per_image, int gs, int KP, hipStream_t stream) {
    DENET_CHECK_ARG(gs >= 2 && gs * gs <= 256, "sparse_bilinear_fwd: grid size %d unsupported", gs);
    DENET_CHECK_ARG(B > 0 && H > 0 && W > 0 && rois_per_image > 0 && F > 0 && coff >= 0, "sparse_bilinear_fwd: bad arguments");
    DENET_CHECK_ARG(coff + F <= CP && KP >= gs * gs * F + 2, "sparse_bilinear_fwd: channel layout inconsistent");
    DENET_CHECK_ARG((long)H * W <= INT_MAX / 2, "sparse_bilinear_fwd: feature map of %d x %d cells is too large", H, W);
    DENET_CHECK_ARG(fmap && bbox && out, "sparse_bilinear_fwd: null pointer");
    DENET_CHECK_ARG((taps4 == nullptr) == (wts4 == nullptr), "sparse_bilinear_fwd: taps4 and wts4 are given together or not at all");
    const int M = B * rois_per_image;
    const bool vec = (coff & 3) == 0 && (F % 4 == 0) && (CP % 4 == 0) && (KP % 4 == 0);
    // ops.kernel_symbol: kind 60 = the gather, 61 = its gradient
    const int prof = denet_prof_begin(60, 0, 0, 0, stream);
    if (vec)
        hipLaunchKernelGGL(sparse_bilinear_fwd_kernel<true>, dim3(M), dim3(256), 0, stream, fmap, bbox, out, taps4, wts4, H, W, CP,
                           coff, F, rois_per_image, gs, KP);
    else
        hipLaunchKernelGGL(sparse_bilinear_fwd_kernel<false>, dim3(M), dim3(256), 0, stream, fmap, bbox, out, taps4, wts4, H, W, CP,
                           coff, F, rois_per_image, gs, KP);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("sparse_bilinear_fwd");
    return DENET_OK;
}

extern "C" size_t denet_sparse_bilinear_workspace_bytes(int B, int H, int W, int rois_per_image, int gs) {
    int rois4;
    if (expanded_rois("sparse_bilinear_workspace_bytes", B, H, W, rois_per_image, gs, &rois4)) return 0;
    return denet_sparse_sort_workspace_bytes(B, H, W, rois4, gs);
}

extern "C" int denet_sparse_bilinear_sort(const int* taps4, void* sort_ws, size_t sort_ws_bytes, int B, int H, int W,
                                          int rois_per_image, int gs, hipStream_t stream) {
    int rois4;
    const int rc = expanded_rois("sparse_bilinear_sort", B, H, W, rois_per_image, gs, &rois4);
    if (rc) return rc;
    DENET_CHECK_ARG(taps4 && sort_ws, "sparse_bilinear_sort: null pointer");
    return denet_sparse_sort(taps4, sort_ws, sort_ws_bytes, B, H, W, rois4, gs, stream);
}

// taps4 == NULL: `sort_ws` already holds the lists written by denet_sparse_bilinear_sort for the same cells
extern "C" int denet_sparse_bilinear_bwd(const float* dy, const int* taps4, const float* wts4, void* sort_ws, size_t sort_ws_bytes,
                                         float* dfmap, int B, int H, int W, int CP, int coff, int F, int rois_per_image, int gs,
                                         int KP, int zero_from, hipStream_t stream) {
    DENET_CHECK_ARG(F > 0 && F % 4 == 0, "sparse_bilinear_bwd: F (%d) must be a positive multiple of 4", F);
    DENET_CHECK_ARG(F / 4 <= 64, "sparse_bilinear_bwd: F (%d) exceeds 256, the channels one wave sums", F);
    DENET_CHECK_ARG(CP % 4 == 0 && KP % 4 == 0, "sparse_bilinear_bwd: CP (%d) and KP (%d) must be multiples of 4", CP, KP);
    int rois4;
    int rc = expanded_rois("sparse_bilinear_bwd", B, H, W, rois_per_image, gs, &rois4);
    if (rc) return rc;
    DENET_CHECK_ARG(coff >= 0 && KP >= gs * gs * F + 2, "sparse_bilinear_bwd: channel layout inconsistent");
    DENET_CHECK_ARG(zero_from >= coff + F && zero_from <= CP, "sparse_bilinear_bwd: zero_from out of range");
    DENET_CHECK_ARG(dy && wts4 && sort_ws && dfmap, "sparse_bilinear_bwd: null pointer");
    SortLayout L;
    rc = sort_layout(B, H, W, rois4, gs, &L);      // (cannot fail behind expanded_rois)
    if (rc) return rc;
    const size_t need = L.total * sizeof(int);
    DENET_CHECK_ARG(sort_ws_bytes >= need, "sparse_bilinear_bwd: workspace too small (%zu < %zu)", sort_ws_bytes, need);
    if (taps4) {
        rc = denet_sparse_sort(taps4, sort_ws, sort_ws_bytes, B, H, W, rois4, gs, stream);
        if (rc) return rc;
    }
    const int* order = (const int*)sort_ws;
    const long ncell = (long)B * H * W;
    const int prof = denet_prof_begin(61, 0, 0, 0, stream);
    hipLaunchKernelGGL(sparse_bilinear_bwd_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, stream, dy, order,
                       order + L.off_start, wts4, dfmap, H * W, CP, coff, F, rois_per_image, gs * gs, KP, zero_from, ncell);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("sparse_bilinear_bwd");
    return DENET_OK;
}
