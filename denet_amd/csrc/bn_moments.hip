// Batch-norm statistics re-estimation (model-update-bn). Reference: denet/model/update_bn.py:52-70 - for one batch-norm
// layer, the per-channel mean and biased variance of its raw input are taken batch by batch in a test-mode forward pass,
// averaged over the full batches in float64, and turned into the running `mean` / `stdinv` in float32.
//
// accumulate: x [M][C] fp32 NHWC -> acc[0][c] += mean_c, acc[1][c] += var_c (biased) of this batch. Two launches:
//   1. partial: every thread sums the SHIFTED values d = x - x[row 0] and d*d of its rows in fp64; the workgroup combines them
//      through LDS and writes one row of the slab partial[gy][2][C]. The shift (the "shifted data" form of the textbook
//      variance algorithms) keeps sum(d*d)/M - (sum(d)/M)^2 free of cancellation when |mean| >> std, which E[x^2] - mean^2 is not:
//      the relative error is eps * (1 + (mean - x0)^2 / var), x0 being one sample of the channel.
//   2. fold: one wave per two channels reduces the slab rows in a fixed order (bn_reduce.h: the order of every two-stage
//      batch-norm reduction) and adds the batch's moments into acc.
//   No atomics: the result is bitwise the same from run to run. No allocation and no host synchronisation.
// finish: acc, n -> run_mean = f32(acc0 / n), run_stdinv = 1 / sqrt(f32(acc1 / n) + 1e-5) in float32 with correctly rounded
// add, square root and division (update_bn.py:63-66 evaluated by numpy in float32).
#include "bn_reduce.h"
#include "../../include/denet_hip.h"

namespace {

constexpr int MOM_WGS = 2048;   // bn_map's target: a memory-bound pass, about 8 workgroups per CU, grid-stride over the rest

// partial[gy][2][C] : sum(x - x0), sum((x - x0)^2), x0 = x[row 0]
__global__ __launch_bounds__(256) void bn_moments_partial_kernel(const float* __restrict__ x, long M, int C, int LC,
                                                                 double* __restrict__ partial) {
    __shared__ double red[256 * 8];
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
    const int c = (blockIdx.x * LC + cl) * 4;
    const f32x4 k0 = *(const f32x4*)(x + c);
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    const long step = (long)gridDim.y * RS;
    long r = (long)blockIdx.y * RS + rsub;
    // four independent row loads in flight per lane
    for (; r + 3 * step < M; r += 4 * step) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(x + (r + u * step) * C + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)v[u][k] - (double)k0[k];
                s[k] += d;
                ss[k] += d * d;
            }
        }
    }
    for (; r < M; r += step) {
        const f32x4 v = *(const f32x4*)(x + r * C + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)v[k] - (double)k0[k];
            s[k] += d;
            ss[k] += d * d;
        }
    }
    bn_reduce_workgroup_tail(s, ss, red, LC, C, c, partial);
}

// one wave per BNF_FC channels: BNF_FJ lanes stride over the slab rows (four loads in flight each), a shuffle tree adds them
constexpr int MOM_NT = 64;

__global__ __launch_bounds__(MOM_NT) void bn_moments_fold_kernel(const float* __restrict__ x, const double* __restrict__ partial,
                                                                 int gy, long M, int C, double* __restrict__ acc) {
    const int cl = threadIdx.x % BNF_FC, jl = threadIdx.x / BNF_FC;
    const int c = blockIdx.x * BNF_FC + cl;
    double s, ss;
    bnf_reduce_partials<false>(partial, gy, C, c, jl, s, ss);
    bnf_reduce_row_lanes(s, ss);
    if (jl != 0 || c >= C) return;
    const double md = s / (double)M;
    double var = ss / (double)M - md * md;   // biased variance of the shifted values = of x
    if (var < 0) var = 0;
    acc[c] += (double)x[c] + md;
    acc[C + c] += var;
}

__global__ __launch_bounds__(256) void bn_moments_finish_kernel(const double* __restrict__ acc, long n, float eps, int C,
                                                                float* __restrict__ run_mean, float* __restrict__ run_stdinv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double dn = (double)n;
    const float mean = (float)(acc[c] / dn);
    const float var = (float)(acc[C + c] / dn);
    run_mean[c] = mean;
    // plain float operations: HIP compiles / and sqrtf correctly rounded (the default -fhip-fp32-correctly-rounded-divide-sqrt,
    // no fast-math); __fsqrt_rn is NOT - it maps to the native approximation unless OCML_BASIC_ROUNDED_OPERATIONS is defined
    const float ve = var + eps;
    run_stdinv[c] = 1.0f / sqrtf(ve);
}

}  // namespace

extern "C" size_t denet_bn_moments_workspace_bytes(long M, int C) {
    if (M <= 0 || C <= 0 || C % 4) return 0;
    const BnReduceMap m = bn_map(M, C, MOM_WGS);
    return (size_t)m.gy * 2 * C * sizeof(double);
}

extern "C" int denet_bn_moments_accumulate(const float* x, double* acc, void* workspace, size_t workspace_bytes, long M, int C,
                                           hipStream_t stream) {
    DENET_CHECK_ARG(x && acc && workspace, "bn_moments_accumulate: null pointer");
    DENET_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "bn_moments_accumulate: bad shape M=%ld C=%d", M, C);
    DENET_CHECK_ARG(workspace_bytes >= denet_bn_moments_workspace_bytes(M, C), "bn_moments_accumulate: workspace of %zu bytes < %zu",
                    workspace_bytes, denet_bn_moments_workspace_bytes(M, C));
    const BnReduceMap m = bn_map(M, C, MOM_WGS);
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(bn_moments_partial_kernel, dim3(m.gx, m.gy), dim3(256), 0, stream, x, M, C, m.LC, partial);
    hipLaunchKernelGGL(bn_moments_fold_kernel, dim3((C + BNF_FC - 1) / BNF_FC), dim3(MOM_NT), 0, stream, x, (const double*)partial, m.gy, M,
                       C, acc);
    DENET_CHECK_LAUNCH("bn_moments_accumulate");
    return DENET_OK;
}

extern "C" int denet_bn_moments_finish(const double* acc, long n, float eps, float* run_mean, float* run_stdinv, int C,
                                       hipStream_t stream) {
    DENET_CHECK_ARG(acc && run_mean && run_stdinv, "bn_moments_finish: null pointer");
    DENET_CHECK_ARG(n > 0 && C > 0, "bn_moments_finish: bad arguments n=%ld C=%d", n, C);
    hipLaunchKernelGGL(bn_moments_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, acc, n, eps, C, run_mean, run_stdinv);
    DENET_CHECK_LAUNCH("bn_moments_finish");
    return DENET_OK;
}
