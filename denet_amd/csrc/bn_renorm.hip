// Batch RENORMALISATION (Ioffe 2017) for the batch norms whose model parameters ask for it (renormMaxR > 1 or renormMaxD > 0:
// `BN[m, eps, r, d, it]`, the JSON keys renormMaxR / renormMaxD / renormMaxIt, model-modify --modify-bn-renorm). Opt-in; every
// other layer never reaches this file.
// Reference: the commented-out block denet/layer/batch_norm.py:65-73 (nothing in the reference runs it, so the definition below
// is the contract). Per channel, with mu_b / inv_b the batch statistics of denet_bn_fwd_train (biased
// variance, eps inside the root) and mean / stdinv the layer's running statistics AS THEY STAND BEFORE THIS STEP'S UPDATE:
//     r = clip((1 / inv_b) * stdinv, 1 / r_max, r_max)            d = clip((mu_b - mean) * stdinv, -d_max, d_max)
//     y = (x - mu_b) * (gamma * inv_b * r) + (beta + gamma * d)   [+ res] [relu]
//     mean <- m * mean + (1 - m) * mu_b      stdinv <- m * stdinv + (1 - m) * inv_b          (batch_norm.py:75-76, unchanged)
// r and d carry no gradient (zero_grad, :71-72). With g = dy masked by y > 0, xh = (x - mu_b) * inv_b, s1 = sum g, s2 = sum g xh:
//     dbeta = s1      dgamma = r * s2 + d * s1      dx = gamma * inv_b * r * (g - s1 / M - xh * s2 / M)      dres = g
// r_max / d_max are this step's limits, computed by the host from the epoch (BatchNormLayer.renorm_limits).
//
// The forward equation is plain batch norm with gamma_eff = gamma * r and beta_eff = beta + gamma * d, the dx equation the plain
// one with gamma_eff: the M x C passes are bn.hip's own kernels fed the effective vectors (denet_bn_apply, denet_bn_bwd_sums,
// denet_bn_bwd_apply - the same kernel and the same vectors in both directions, so the ReLU mask the backward pass recomputes
// from x is the forward's). What is new is the per-channel work between them:
//   bn_renorm_stats_finish_kernel  partial [rows][2][C] (a convolution epilogue's, or denet_bn_stats_partial's) -> save_mean,
//                                  save_invstd (bn_stats_final_kernel's reduction order and expressions: bit-identical, no
//                                  atomics), r, d, gamma_eff, beta_eff, and THEN the running statistics, by the same lane in the
//                                  same launch: the values r and d were clipped against are read before they are overwritten
//                                  and cannot be lost to the ordering of two launches. A long row list (a stem convolution
//                                  leaves 16 384 rows) is reduced here in ONE stage on purpose, as denet_bn_fwd_train_pre does:
//                                  the two-stage fold (bn_stats_fold_kernel) exists only on the pool-fused route, which a
//                                  renorm-active layer does not take; measured ~9 us per launch on DeNet-34 (EXPERIMENTS.md)
//   bn_renorm_grad_fold_kernel     s1, s2 (denet_bn_bwd_sums, written to scratch) -> dgamma = r * s2 + d * s1, dbeta = s1 in the
//                                  gradient slab; the slab never holds s2
// state [4][C] floats: r | d | gamma_eff | beta_eff, written by the forward call, read by the backward call of the same step.
#include "bn_reduce.h"
#include "../../include/denet_hip.h"
#include <math.h>

namespace {

// one wave per BNF_FC channels, 64 / BNF_FC row lanes: bn_stats_final_kernel's shape (bn.hip), no LDS
__global__ __launch_bounds__(64) void bn_renorm_stats_finish_kernel(const double* __restrict__ partial, int rows, long M, int C,
                                                                    float eps, float momentum, float r_max, float d_max,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float* __restrict__ run_mean, float* __restrict__ run_stdinv,
                                                                    float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                    float* __restrict__ state) {
    const int cl = threadIdx.x % BNF_FC, jl = threadIdx.x / BNF_FC;
    const int c = blockIdx.x * BNF_FC + cl;
    double s, ss;
    bnf_reduce_partials<false>(partial, rows, C, c, jl, s, ss);
    bnf_reduce_row_lanes(s, ss);
    if (jl != 0 || c >= C) return;
    // the running statistics of BEFORE this step: read here, overwritten below by this very lane (bnf_finish_stats)
    const float old_mean = run_mean[c], old_stdinv = run_stdinv[c];
    bnf_finish_stats(s, ss, M, eps, momentum, c, save_mean, save_invstd, run_mean, run_stdinv);
    const float fmean = save_mean[c], finv = save_invstd[c];
    const float r = fminf(fmaxf((1.0f / finv) * old_stdinv, 1.0f / r_max), r_max);
    const float d = fminf(fmaxf((fmean - old_mean) * old_stdinv, -d_max), d_max);
    const float g = gamma[c];
    state[c] = r;
    state[C + c] = d;
    state[2 * C + c] = g * r;
    state[3 * C + c] = beta[c] + g * d;
}

// sums [2][C]: s1 = sum g | s2 = sum g * xhat (bn_bwd_final_kernel's dbeta | dgamma of the plain layer)
__global__ __launch_bounds__(256) void bn_renorm_grad_fold_kernel(const float* __restrict__ sums, const float* __restrict__ state, int C,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float s1 = sums[c], s2 = sums[C + c];
    dgamma[c] = state[c] * s2 + state[C + c] * s1;
    dbeta[c] = s1;
}

}  // namespace

// denet_bn_workspace_bytes + the [2][C] scratch of the two plain sums
extern "C" size_t denet_bn_renorm_workspace_bytes(long M, int C) {
    const size_t base = denet_bn_workspace_bytes(M, C);
    return base ? base + (size_t)2 * C * sizeof(float) : 0;
}

// training forward (batch_norm.py:65-73). partial / rows: the sums a producing convolution left (denet_conv_fwd_stats ...), or
// partial = NULL: measured here over x (needs workspace). ops.kernel_symbol: kinds 40 / 41 = the two new launches
extern "C" int denet_bn_renorm_fwd_train(const float* x, const float* res, float* y, const float* gamma, const float* beta,
                                         float* run_mean, float* run_stdinv, float* save_mean, float* save_invstd, float* state,
                                         const double* partial, int rows, void* workspace, long M, int C, float momentum, float eps,
                                         float r_max, float d_max, int relu, hipStream_t stream) {
    DENET_CHECK_ARG(x && y && gamma && beta && run_mean && run_stdinv && save_mean && save_invstd && state && (partial || workspace),
                    "bn_renorm_fwd_train: null pointer");
    DENET_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "bn_renorm_fwd_train: bad shape M=%ld C=%d", M, C);
    DENET_CHECK_ARG(!partial || rows > 0, "bn_renorm_fwd_train: %d rows of partial sums", rows);
    DENET_CHECK_ARG(r_max >= 1.0f && d_max >= 0.0f && isfinite(r_max) && isfinite(d_max),
                    "bn_renorm_fwd_train: limits r_max = %g (>= 1), d_max = %g (>= 0) must be finite", (double)r_max, (double)d_max);
    if (!partial) {
        int rc = denet_bn_stats_partial(x, workspace, &rows, M, C, stream);
        if (rc != DENET_OK) return rc;
        partial = (const double*)workspace;
    }
    const int prof = denet_prof_begin(40, 0, 0, 0, stream);
    hipLaunchKernelGGL(bn_renorm_stats_finish_kernel, dim3((C + BNF_FC - 1) / BNF_FC), dim3(64), 0, stream, partial, rows, M, C, eps,
                       momentum, r_max, d_max, gamma, beta, run_mean, run_stdinv, save_mean, save_invstd, state);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("bn_renorm_fwd_train");
    return denet_bn_apply(x, res, y, state + 2 * (size_t)C, state + 3 * (size_t)C, save_mean, save_invstd, M, C, relu, stream);
}

// its gradient: state / save_mean / save_invstd from the forward call of this step. y: the forward output where the ReLU mask
// needs it (a residual was added), else NULL (recomputed from x with the effective vectors). dres: NULL or the masked gradient
// (want_dres). workspace: denet_bn_renorm_workspace_bytes(M, C)
extern "C" int denet_bn_renorm_bwd(const float* x, const float* y, const float* dy, const float* save_mean, const float* save_invstd,
                                   const float* state, float* dx, float* dres, float* dgamma, float* dbeta, void* workspace, long M,
                                   int C, int relu, hipStream_t stream) {
    DENET_CHECK_ARG(x && dy && save_mean && save_invstd && state && dx && dgamma && dbeta && workspace, "bn_renorm_bwd: null pointer");
    DENET_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "bn_renorm_bwd: bad shape M=%ld C=%d", M, C);
    const size_t base = denet_bn_workspace_bytes(M, C);
    float* coef = (float*)((char*)workspace + base) - 2 * (size_t)C;      // (the tail of the plain workspace, as in denet_bn_bwd)
    float* sums = (float*)((char*)workspace + base);
    const float* gamma_eff = state + 2 * (size_t)C;
    const float* beta_eff = state + 3 * (size_t)C;
    int rc = denet_bn_bwd_sums(x, y, dy, gamma_eff, beta_eff, save_mean, save_invstd, sums + C, sums, coef, workspace, M, C, relu, stream);
    if (rc != DENET_OK) return rc;
    const int prof = denet_prof_begin(41, 0, 0, 0, stream);
    hipLaunchKernelGGL(bn_renorm_grad_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, sums, state, C, dgamma, dbeta);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("bn_renorm_bwd");
    return denet_bn_bwd_apply(x, y, dy, gamma_eff, beta_eff, save_mean, save_invstd, coef, dx, dres, M, C, relu, stream);
}
