// Opt-in focal cost of the corner map and of the detection head's class part (NHWC fp32, gfx950). `gamma` is the layers'
// focal_gamma; the definition is DESIGN.md section 17. The reference has no such mode: it extends the plain costs of
//   corner NLL cost/gradient      reference denet/layer/denet_corner.py:126-134   (dss.hip corner_loss_kernel)
//   detection cost/gradient       reference denet/layer/denet_detect.py:238-313   (dss.hip detect_loss_kernel)
// whose kernels and entry points stay as they are; gamma = 0 gives their formulas.
// This file is compiled with -ffp-contract=off like dss.hip: the box regression and independent-fitness terms, the finishing
// sum and the corner grid are the plain kernels' own code (dss.h) and give their bits.
#include "dss.h"
#include "../../include/denet_hip.h"

namespace {

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
    const double sum = block_sum_256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
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
// The box regression, the independent-fitness cross entropy (no focal factor) and costs[1] are detect_loss_kernel's: both
// kernels call dss.h for them.
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
        if (nreg > 0) berr = detect_box_term(z, dz, m, lane, ncls, bbox_valid, bbox_t, roi_bbox, bounded_iou, bbox_factor, bbox_scale);
        if (nfit > 0) berr += detect_fit_term(z, dz, m, lane, ncls, nreg, fit_t, nfit, fit_factor, fit_scale);
        if (dz) {
            for (int c = ncls + nreg + nfit + lane; c < CP; c += 64) dz[c] = 0.f;
        }
    }
    detect_store_sums(derr, berr, partial);
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
    const int g = corner_loss_grid((long)B * H * W);
    const float scale = (float)((double)cost_factor / ((double)B * LN2));
    // ops.kernel_symbol: kind 70 = the corner cost, 71 = the detection cost
    const int prof = denet_prof_begin(70, 0, 0, 0, stream);
    hipLaunchKernelGGL(corner_focal_loss_kernel, dim3(g), dim3(256), 0, stream, corner_pr, target, dconv,
                       (double*)workspace, B, H, W, CP, Cn, scale, gamma);
    denet_prof_end(prof, stream);
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace, g,
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
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace, g,
                       (double)cost_factor / (double)batch, costs);
    // costs[1] = box cost + independent-fitness cost (both already carry their factors)
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace + g, g,
                       1.0 / (double)batch, costs + 1);
    DENET_CHECK_LAUNCH("detect_loss_focal");
    return DENET_OK;
}
