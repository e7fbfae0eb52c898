// Opt-in focal cost of the corner map and of the detection head's class part (NHWC fp32, gfx950). `gamma` is the layers'
// focal_gamma; the definition is DESIGN.md section 17. The reference has no such mode: it extends the plain costs of
//   corner NLL cost/gradient      reference denet/layer/denet_corner.py:126-134   (dss.hip corner_loss_kernel)
//   detection cost/gradient       reference denet/layer/denet_detect.py:238-313   (dss.hip detect_loss_kernel)
// whose kernels and entry points stay as they are; gamma = 0 gives their formulas.
// This file is compiled with -ffp-contract=off like dss.hip: the box regression and independent-fitness terms are the plain
// kernel's statements and must give its bits.
#include "common.h"
#include "../../include/denet_hip.h"
#include <math.h>

namespace {

constexpr double LN2 = 0.6931471805599453;

// gamma is 0 (the plain cost) or finite and >= 1: q^(gamma - 1) is singular in between
bool gamma_ok(float gamma) { return gamma == 0.f || (isfinite(gamma) && gamma >= 1.f); }

// ---------------------------------------------------------------------------------------------
// corner map, softmax over [x, -x]: p1 = 1 - p0 exactly, so the modulating factors are p_k^gamma = exp(gamma * l_k)
//   cost  = -scale * sum( t0 * p1^g * l0 + t1 * p0^g * l1 )
//   dconv =  scale * ( t0 * p1^g * (2g p0 l0 - 2 p1) + t1 * p0^g * (2 p0 - 2g p1 l1) )        (dp0/dx = 2 p0 p1)
// Only the Cn corner channels of dconv are written: the others belong to the RoI gather's gradient.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void corner_focal_loss_kernel(const float* __restrict__ pr, const float* __restrict__ tgt,
                                                                float* __restrict__ dconv, double* __restrict__ partial,
                                                                int B, int H, int W, int CP, int Cn, float scale, float gamma) {
    __shared__ double red[256];
    const long total = (long)B * H * W;
    const long plane = (long)H * W;
    double acc = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / plane, yx = i - b * plane;
        for (int ci = 0; ci < Cn; ++ci) {
            const long o0 = ((b * 2 + 0) * Cn + ci) * plane + yx;
            const long o1 = ((b * 2 + 1) * Cn + ci) * plane + yx;
            const float l0 = pr[o0], l1 = pr[o1];
            const float t0 = tgt[o0], t1 = tgt[o1];
            const float w0 = expf(gamma * l1), w1 = expf(gamma * l0);      // p1^gamma weighs the k = 0 term, p0^gamma the k = 1 term
            acc += (double)t0 * (double)w0 * (double)l0 + (double)t1 * (double)w1 * (double)l1;
            if (dconv) {
                const float p0 = expf(l0), p1 = expf(l1);
                const float g0 = t0 * w0 * (2.f * gamma * p0 * l0 - 2.f * p1);
                const float g1 = t1 * w1 * (2.f * p0 - 2.f * gamma * p1 * l1);
                dconv[i * CP + ci] = scale * (g0 + g1);
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out[0] = factor * sum(partial[0..n)) in a fixed order (the finishing pass of the plain costs, dss.hip)
__global__ __launch_bounds__(256) void focal_finish_sum_kernel(const double* __restrict__ partial, int n, double factor,
                                                               float* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (float)(factor * red[0]);
}

// w = q^gamma and q^(gamma - 1) from one powf. gamma = 0: w = 1 for every q, q = 0 included, and the second factor only ever
// appears multiplied by gamma: 0 stands for it (powf(0, -1) is inf)
__device__ __forceinline__ void focal_factors(float q, float gamma, float& w, float& qg1) {
    if (gamma == 0.f) {
        w = 1.f;
        qg1 = 0.f;
    } else {
        qg1 = powf(q, gamma - 1.f);
        w = qg1 * q;
    }
}

// ---------------------------------------------------------------------------------------------
// detection cost, one wave per RoI. Class part (lp = log-softmax, p = exp(lp), q = 1 - p = -expm1(lp)):
//   det_err = -sum_c t_c q_c^g lp_c / ln(ncls)
//   a_c     = t_c * (q_c^g - g q_c^(g-1) p_c lp_c),  A = sum_c a_c,   dz_j = det_scale / ln(ncls) * (p_j * A - a_j)
// The box regression, the independent-fitness cross entropy, costs[1] and the zeroed padding columns are
// detect_loss_kernel's, statement for statement.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void detect_focal_loss_kernel(const float* __restrict__ logits, const float* __restrict__ det_t,
                                                                const float* __restrict__ bbox_valid,
                                                                const float* __restrict__ bbox_t, float* __restrict__ dlogits,
                                                                double* __restrict__ partial, int M, int CP, int ncls,
                                                                int nreg, float det_scale, float bbox_factor,
                                                                float bbox_scale, int bounded_iou,
                                                                const float* __restrict__ roi_bbox,
                                                                const float* __restrict__ fit_t, int nfit, float fit_factor,
                                                                float fit_scale, float gamma) {
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wv;
    double derr = 0, berr = 0;
    if (m < M) {
        const float* z = logits + (long)m * CP;
        float* dz = dlogits ? dlogits + (long)m * CP : nullptr;
        const float* t = det_t + (long)m * ncls;
        float mx = -INFINITY;
        for (int c = lane; c < ncls; c += 64) mx = fmaxf(mx, z[c]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float se = 0.f;
        for (int c = lane; c < ncls; c += 64) se += expf(z[c] - mx);
        for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
        const float lse = logf(se);
        const float inv_logn = (float)(1.0 / log((double)ncls));
        // first pass over the classes: the cost and A, which dz needs whole; the second pass forms a_c again (expf, expm1f and one
        // powf per class) instead of keeping a row of unknown length in registers
        float e = 0.f, A = 0.f;
        for (int c = lane; c < ncls; c += 64) {
            const float lp = (z[c] - mx) - lse;
            const float p = expf(lp), q = -expm1f(lp);
            float w, qg1;
            focal_factors(q, gamma, w, qg1);
            e += t[c] * w * lp;
            A += t[c] * (w - gamma * qg1 * p * lp);
        }
        for (int o = 32; o > 0; o >>= 1) {
            e += __shfl_xor(e, o, 64);
            A += __shfl_xor(A, o, 64);
        }
        derr = -(double)e * (double)inv_logn;
        if (dz) {
            for (int c = lane; c < ncls; c += 64) {
                const float lp = (z[c] - mx) - lse;
                const float p = expf(lp), q = -expm1f(lp);
                float w, qg1;
                focal_factors(q, gamma, w, qg1);
                const float a = t[c] * (w - gamma * qg1 * p * lp);
                dz[c] = det_scale * inv_logn * (p * A - a);
            }
        }
        if (nreg > 0) {
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
                        const float pc = reg * se_ + sc;
                        const float dxy = bt[lane] - pc;
                        const float tw = bt[2 + lane];
                        if (dxy >= 0.f) {
                            const float den = tw + dxy + eps;
                            d = 2.f * dxy / den;
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
                            dd_dreg = tw / ((pw + eps) * (pw + eps)) * pw;
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
            berr = (double)bbox_factor * (double)bbox_factor * (double)sl;     // factor of get_errors :295 and of cost :310
        }
        if (nfit > 0) {
            // independent fitness distribution (denet_detect.py:103-108, 298-301): plain cross entropy, no focal factor
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
            berr += (double)fit_factor * (-(double)fsum * (double)finv);
        }
        if (dz) {
            for (int c = ncls + nreg + nfit + lane; c < CP; c += 64) dz[c] = 0.f;
        }
    }
    if (lane == 0) {
        red[0][wv] = derr;
        red[1][wv] = berr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        partial[gridDim.x + blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

}  // namespace

extern "C" int denet_corner_loss_focal(const float* corner_pr, const float* target, float* dconv, float* cost,
                                       void* workspace, int B, int H, int W, int CP, int Cn, float cost_factor, float gamma,
                                       hipStream_t stream) {
    DENET_CHECK_ARG(gamma_ok(gamma), "corner_loss_focal: gamma must be 0 or finite and >= 1, got %g", (double)gamma);
    DENET_CHECK_ARG(corner_pr && target && cost && workspace, "corner_loss_focal: null pointer");
    // (CP is the channel stride of dconv: it means nothing without one, the test-mode cost)
    DENET_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cn > 0 && (!dconv || Cn <= CP),
                    "corner_loss_focal: bad shape (B = %d, map %d x %d, Cn = %d, CP = %d)", B, H, W, Cn, CP);
    // the grid of denet_corner_loss: at most 1024 partial sums, far inside denet_loss_workspace_bytes()
    long g = ((long)B * H * W + 255) / 256;
    if (g > 1024) g = 1024;
    const float scale = (float)((double)cost_factor / ((double)B * LN2));
    // ops.kernel_symbol: kind 70 = the corner cost, 71 = the detection cost
    const int prof = denet_prof_begin(70, 0, 0, 0, stream);
    hipLaunchKernelGGL(corner_focal_loss_kernel, dim3((unsigned)g), dim3(256), 0, stream, corner_pr, target, dconv,
                       (double*)workspace, B, H, W, CP, Cn, scale, gamma);
    denet_prof_end(prof, stream);
    hipLaunchKernelGGL(focal_finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace, (int)g,
                       -(double)cost_factor / ((double)B * LN2), cost);
    DENET_CHECK_LAUNCH("corner_loss_focal");
    return DENET_OK;
}

extern "C" int denet_detect_loss_focal(const float* logits, const float* det_target, const float* bbox_valid,
                                       const float* bbox_target, const float* roi_bbox, const float* fit_target,
                                       float* dlogits, float* costs, void* workspace, int M, int batch, int CP, int ncls,
                                       int nreg, int nfit, float cost_factor, float bbox_factor, float fit_factor,
                                       int bounded_iou, float gamma, hipStream_t stream) {
    DENET_CHECK_ARG(gamma_ok(gamma), "detect_loss_focal: gamma must be 0 or finite and >= 1, got %g", (double)gamma);
    DENET_CHECK_ARG(logits && det_target && costs && workspace, "detect_loss_focal: null pointer");
    DENET_CHECK_ARG(M > 0 && batch > 0 && ncls > 1, "detect_loss_focal: bad shape (M = %d, batch = %d, ncls = %d)", M, batch, ncls);
    DENET_CHECK_ARG(nreg == 0 || nreg == 4, "detect_loss_focal: nreg must be 0 or 4");
    DENET_CHECK_ARG(nreg == 0 || (bbox_valid && bbox_target), "detect_loss_focal: bbox targets missing");
    DENET_CHECK_ARG(!bounded_iou || roi_bbox, "detect_loss_focal: bounded IoU needs the RoI boxes");
    DENET_CHECK_ARG(nfit >= 0 && nfit <= 64 && (nfit == 0 || fit_target),
                    "detect_loss_focal: fitness targets missing / nfit > 64");
    DENET_CHECK_ARG(ncls + nreg + nfit <= CP, "detect_loss_focal: CP too small");
    const int g = (M + 3) / 4;
    DENET_CHECK_ARG(g <= 65536, "detect_loss_focal: too many RoIs (%d)", M);
    const float det_scale = cost_factor / (float)batch;
    // bbox_factor is applied twice in the reference: get_errors :295 and cost :310
    const float bbox_scale = bbox_factor * bbox_factor / (float)batch;
    const int prof = denet_prof_begin(71, 0, 0, 0, stream);
    hipLaunchKernelGGL(detect_focal_loss_kernel, dim3(g), dim3(256), 0, stream, logits, det_target, bbox_valid, bbox_target,
                       dlogits, (double*)workspace, M, CP, ncls, nreg, det_scale, bbox_factor, bbox_scale, bounded_iou,
                       roi_bbox, fit_target, nfit, fit_factor, fit_factor / (float)batch, gamma);
    denet_prof_end(prof, stream);
    hipLaunchKernelGGL(focal_finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace, g,
                       (double)cost_factor / (double)batch, costs);
    // costs[1] = box cost + independent-fitness cost (both already carry their factors)
    hipLaunchKernelGGL(focal_finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace + g, g,
                       1.0 / (double)batch, costs + 1);
    DENET_CHECK_LAUNCH("detect_loss_focal");
    return DENET_OK;
}
