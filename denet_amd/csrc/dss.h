// What the directed-sparse-sampling kernels of dss.hip share with their opt-in modes (focal.hip, sparse_bilinear.hip): the modes
// call the default path's device code, they do not repeat it. The bit equality that DESIGN.md sections 16 and 17 promise between
// a mode and the default path holds because both compile this one text, under -ffp-contract=off (build.py NO_CONTRACT).
//   block_sum_256, finish_sum_kernel, corner_loss_grid   the partial sums of a cost and the pass that finishes them
//   detect_box_term, detect_fit_term, detect_store_sums  the detection cost behind its class part
//   sparse_cell_sum<WEIGHTED>                            the gather gradient of one feature-map cell
//   SortLayout, sort_layout                              the workspace of denet_sparse_sort
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr double LN2 = 0.6931471805599453;

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// grid of the corner cost kernels: at most 1024 partial sums, far inside denet_loss_workspace_bytes()
int corner_loss_grid(long total) {
    const int g = grid_for(total);
    return g > 1024 ? 1024 : g;
}

// sum of v over the 256 threads of a workgroup, in a fixed order; every thread calls it, thread 0 uses the result
__device__ __forceinline__ double block_sum_256(double v) {
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// out[slot] = factor * sum(partial[0..n))
__global__ void finish_sum_kernel(const double* __restrict__ partial, int n, double factor, float* __restrict__ out) {
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    const double sum = block_sum_256(acc);
    if (threadIdx.x == 0) *out = (float)(factor * sum);
}

// ---------------------------------------------------------------------------------------------
// detection cost behind the class part: one wave per RoI m, z / dz its row of logits / gradients (dz may be null)
// ---------------------------------------------------------------------------------------------
// box regression over the four logits behind the classes; lanes 0..3 work, every lane returns the RoI's bbox_err
__device__ __forceinline__ double detect_box_term(const float* __restrict__ z, float* __restrict__ dz, int m, int lane, int ncls,
                                                  const float* __restrict__ bbox_valid, const float* __restrict__ bbox_t,
                                                  const float* __restrict__ roi_bbox, int bounded_iou, float bbox_factor,
                                                  float bbox_scale) {
    float sl = 0.f;
    if (lane < 4) {
        const float valid = bbox_valid[m];
        const float* bt = bbox_t + (long)m * 8;
        const float reg = z[ncls + lane];
        float d = 0.f, dd_dreg = -1.f;   // d = residual fed to smooth L1 ; dd_dreg = d(d)/d(reg)
        if (!bounded_iou) {
            // Fast R-CNN targets: (tcx-scx)/sw, (tcy-scy)/sh, ln(tw/sw), ln(th/sh)
            float tk;
            if (lane < 2) tk = (bt[lane] - bt[4 + lane]) / bt[6 + lane];
            else tk = logf(bt[lane] / bt[4 + lane]);
            d = tk - reg;
            dd_dreg = -1.f;
        } else {
            // bounded IoU (denet_detect.py:266-286); prediction decoded from the RoI box
            const float* rb = roi_bbox + (long)m * 4;
            const float scx = 0.5f * (rb[0] + rb[2]), scy = 0.5f * (rb[1] + rb[3]);
            const float sw = rb[2] - rb[0], sh = rb[3] - rb[1];
            const float eps = 0.001f;
            if (lane < 2) {
                const float sc = lane == 0 ? scx : scy, se_ = lane == 0 ? sw : sh;
                // predict_x = 0.5*((cx - w/2) + (cx + w/2)) -> cx = reg*extent + centre
                const float pc = reg * se_ + sc;
                const float dxy = bt[lane] - pc;
                const float tw = bt[2 + lane];
                if (dxy >= 0.f) {
                    const float den = tw + dxy + eps;
                    d = 2.f * dxy / den;
                    // d/d(dxy) = 2*(tw+eps)/den^2 ; d(dxy)/dreg = -extent
                    dd_dreg = 2.f * (tw + eps) / (den * den) * (-se_);
                } else {
                    const float den = tw - dxy + eps;
                    d = -2.f * dxy / den;
                    dd_dreg = -2.f * (tw + eps) / (den * den) * (-se_);
                }
            } else {
                const float se_ = lane == 2 ? sw : sh;
                const float pw = expf(reg) * se_;
                const float tw = bt[lane];
                const float a = tw / (pw + eps), c2 = pw / (tw + eps);
                if (a <= c2) {
                    d = 1.f - a;
                    dd_dreg = tw / ((pw + eps) * (pw + eps)) * pw;   // d(1-a)/dpw * dpw/dreg
                } else {
                    d = 1.f - c2;
                    dd_dreg = -pw / (tw + eps);
                }
            }
        }
        const float ad = fabsf(d);
        sl = (ad < 1.f) ? 0.5f * d * d : ad - 0.5f;
        const float dsl = (ad < 1.f) ? d : (d > 0.f ? 1.f : -1.f);
        if (dz) dz[ncls + lane] = bbox_scale * valid * dsl * dd_dreg;
        sl *= valid;
    }
    for (int o = 2; o > 0; o >>= 1) sl += __shfl_xor(sl, o, 64);
    return (double)bbox_factor * (double)bbox_factor * (double)sl;     // factor of get_errors :295 and of cost :310
}

// independent fitness distribution (denet_detect.py:103-108, 298-301): a second soft-target cross entropy
// over the nfit logits behind the box regressors (plain in the focal mode too); returns its share of bbox_err
__device__ __forceinline__ double detect_fit_term(const float* __restrict__ z, float* __restrict__ dz, int m, int lane, int ncls,
                                                  int nreg, const float* __restrict__ fit_t, int nfit, float fit_factor,
                                                  float fit_scale) {
    const float* zf = z + ncls + nreg;
    const float* tf = fit_t + (long)m * nfit;
    const float zv = lane < nfit ? zf[lane] : -INFINITY;
    float fm = zv;
    for (int o = 32; o > 0; o >>= 1) fm = fmaxf(fm, __shfl_xor(fm, o, 64));
    float fe = lane < nfit ? expf(zv - fm) : 0.f, ft = lane < nfit ? tf[lane] : 0.f;
    float fse = fe, fts = ft;
    for (int o = 32; o > 0; o >>= 1) {
        fse += __shfl_xor(fse, o, 64);
        fts += __shfl_xor(fts, o, 64);
    }
    const float flse = logf(fse);
    const float finv = (float)(1.0 / log((double)nfit));
    const float flp = lane < nfit ? (zv - fm) - flse : 0.f;
    float fsum = ft * flp;
    if (dz && lane < nfit) dz[ncls + nreg + lane] = fit_scale * finv * (fts * expf(flp) - ft);
    for (int o = 32; o > 0; o >>= 1) fsum += __shfl_xor(fsum, o, 64);
    return (double)fit_factor * (-(double)fsum * (double)finv);
}

// the four waves' (det_err, bbox_err) -> partial[block], partial[gridDim.x + block]; every thread of the workgroup calls it
__device__ __forceinline__ void detect_store_sums(double derr, double berr, double* __restrict__ partial) {
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = derr;
        red[1][threadIdx.x >> 6] = berr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        partial[gridDim.x + blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// ---------------------------------------------------------------------------------------------
// gather gradient, step 2: one wave per feature-map cell sums the dy rows of every (roi, tap) that sampled this cell, in
// ascending slot order (deterministic replacement for the reference's atomicAdd scatter).
// WEIGHTED (bilinear sampling): four slots per tap, slot s' = (roi * ntap + tap) * 4 + q names its dy row by s' >> 2 and its
// weight by wts4[s']; a group adds weight * row, the product rounded, then the sum. Nothing else differs.
// ---------------------------------------------------------------------------------------------
template <bool WEIGHTED>
__device__ __forceinline__ void sparse_cell_sum(const float* __restrict__ dy, const int* __restrict__ order,
                                                const int* __restrict__ cell_start, const float* __restrict__ wts4,
                                                float* __restrict__ dfmap, int HW, int CP, int coff, int F, int rois_per_image,
                                                int ntap, int KP, int zero_from, long ncell_total) {
    const int lane = threadIdx.x & 63;
    const long cellg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cellg >= ncell_total) return;
    const int b = (int)(cellg / HW);
    const int cell = (int)(cellg - (long)b * HW);
    const int n = rois_per_image * ntap * (WEIGHTED ? 4 : 1);
    const int F4 = F / 4;
    const int epi = 64 / F4;  // entries per iteration
    const int e = lane / F4, f4 = lane - e * F4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int* cs = cell_start + (long)b * (HW + 1);
    const int start = cs[cell], end = cs[cell + 1];
    const int* ord = order + (long)b * n;
    // entry j of the cell belongs to lane group j % epi: a fixed left-to-right chain per group. The slots of up to CH entries come
    // in with ONE coalesced load and are handed out by shuffles, and a group has the rows of four entries in flight before it
    // adds them (in order): slot -> address -> row was two dependent loads per entry, 3-4 times in a row per wave - the kernel
    // ran at the latency of that chain (281 us alone, 0.84 ms beside the first head layer's filter gradient).
    // The lane that loads a slot loads its weight too: that dependent load is per chunk, not per entry
    const int CH = (64 / epi) * epi;
    const bool grp = e < epi;
    const float* dyb = dy + (long)b * rois_per_image * KP + f4 * 4;
    for (int base = start; base < end; base += CH) {
        const int cnt = min(CH, end - base);
        const int mine = (lane < cnt) ? ord[base + lane] : 0;
        float wmine = 0.f;
        if (WEIGHTED && lane < cnt) wmine = wts4[(long)b * n + mine];
        for (int j0 = 0; j0 < cnt; j0 += 4 * epi) {
            f32x4 v[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * epi + e;
                int slot = __shfl(mine, j & 63, 64);
                if (WEIGHTED) {
                    slot >>= 2;
                    w[u] = __shfl(wmine, j & 63, 64);
                }
                const int roi = slot / ntap, tap = slot - roi * ntap;
                v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (grp && j < cnt) v[u] = *(const f32x4*)(dyb + (long)roi * KP + (long)tap * F);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (grp && j0 + u * epi + e < cnt) {
                    if (WEIGHTED) acc += w[u] * v[u];
                    else acc += v[u];
                }
        }
    }
    f32x4 tot = acc;
    for (int k = 1; k < epi; ++k) {
#pragma unroll
        for (int c = 0; c < 4; ++c) tot[c] += __shfl(acc[c], f4 + k * F4, 64);
    }
    float* o = dfmap + cellg * CP;
    if (lane < F4) {
        if ((coff & 3) == 0) {
            *(f32x4*)(o + coff + lane * 4) = tot;
        } else {      // DNC.C: five corner channels in front of the features, the slice is not 16-byte aligned
            float* q = o + coff + lane * 4;
            q[0] = tot[0]; q[1] = tot[1]; q[2] = tot[2]; q[3] = tot[3];
        }
    }
    // zero the physical padding channels of this cell
    for (int c = zero_from + lane; c < CP; c += 64) o[c] = 0.f;
}

// Workspace of denet_sparse_sort / denet_sparse_bwd: order [B][n] | cell_start [B][HW+1] | counts [B][nchunk][HW] |
// positions [B][nchunk][HW] (int32); n = rois_per_image * gs * gs keys per image (the bilinear rule passes four "RoIs" per RoI)
constexpr int SORT_CHUNK = 2048;
struct SortLayout {
    int n, HW, nchunk, key_bits;
    size_t off_start, off_table, total;   // in ints
};
int sort_layout(int B, int H, int W, int rois_per_image, int gs, SortLayout* L) {
    DENET_CHECK_ARG(B > 0 && H > 0 && W > 0 && rois_per_image > 0 && gs > 0, "sparse_sort: bad arguments");
    DENET_CHECK_ARG((long)H * W <= 32768, "sparse_sort: feature map of %d x %d cells exceeds the 32768-cell LDS cursor", H, W);
    L->n = rois_per_image * gs * gs;
    L->HW = H * W;
    L->nchunk = (L->n + SORT_CHUNK - 1) / SORT_CHUNK;
    L->key_bits = 1;
    while ((1 << L->key_bits) < L->HW) L->key_bits++;
    L->off_start = (size_t)B * L->n;
    L->off_table = L->off_start + (size_t)B * (L->HW + 1);
    L->total = L->off_table + (size_t)2 * B * L->nchunk * L->HW;      // counts | positions
    return DENET_OK;
}

}  // namespace
