// Batch-norm statistics re-estimation (model-update-bn). Reference: denet/model/update_bn.py:52-70 - for one batch-norm
// layer, the per-channel mean and biased variance of its raw input are taken batch by batch in a test-mode forward pass,
// averaged over the full batches in float64, and turned into the running `mean` / `stdinv` in float32.
//
// accumulate: x [M][C] fp32 NHWC -> acc[0][c] += mean_c, acc[1][c] += var_c (biased) of this batch. Two launches:
//   1. partial: every thread sums the SHIFTED values d = x - x[row 0] and d*d of its rows in fp64; the workgroup combines them
//      through LDS and writes one row of the slab partial[gy][2][C]. The shift (the "shifted data" form of the textbook
//      variance algorithms) keeps sum(d*d)/M - (sum(d)/M)^2 free of cancellation when |mean| >> std, which E[x^2] - mean^2 is not:
//      the relative error is eps * (1 + (mean - x0)^2 / var), x0 being one sample of the channel.
//   2. fold: one wave per two channels reduces the slab rows in a fixed order and adds the batch's moments into acc.
//   No atomics: the result is bitwise the same from run to run. No allocation and no host synchronisation.
// finish: acc, n -> run_mean = f32(acc0 / n), run_stdinv = 1 / sqrt(f32(acc1 / n) + 1e-5) in float32 with correctly rounded
// add, square root and division (update_bn.py:63-66 evaluated by numpy in float32).
#include "common.h"
#include "../../include/denet_hip.h"

namespace {

struct MomMap {
    int LC;      // lanes along channels (float4 units)
    int RS;      // rows handled concurrently by one workgroup
    int gx, gy;  // grid
};

MomMap mom_map(long M, int C) {
    MomMap m;
    const int c4 = C / 4;
    int lc = 1;
    while (lc < 256 && (c4 % (lc * 2)) == 0) lc *= 2;
    m.LC = lc;
    m.RS = 256 / lc;
    m.gx = c4 / lc;
    const long rows_blocks = (M + m.RS - 1) / m.RS;
    // a memory-bound pass: about 2048 workgroups (8 per CU), grid-stride over the rest
    int gy = 2048 / m.gx;
    if (gy < 1) gy = 1;
    if (gy > rows_blocks) gy = (int)rows_blocks;
    m.gy = gy;
    return m;
}

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
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        red[tid * 8 + k] = s[k];
        red[tid * 8 + 4 + k] = ss[k];
    }
    __syncthreads();
    if (rsub == 0) {
        for (int j = 1; j < RS; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] += red[(j * LC + cl) * 8 + k];
                ss[k] += red[(j * LC + cl) * 8 + 4 + k];
            }
        }
        double* p = partial + (long)blockIdx.y * 2 * C;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[c + k] = s[k];
            p[C + c + k] = ss[k];
        }
    }
}

// one wave per MC channels: MJ = 64 / MC lanes stride over the slab rows (four loads in flight each), a shuffle tree adds them
constexpr int MC = 2, MJ = 64 / MC, MOM_NT = 64;

__global__ __launch_bounds__(MOM_NT) void bn_moments_fold_kernel(const float* __restrict__ x, const double* __restrict__ partial,
                                                                 int gy, long M, int C, double* __restrict__ acc) {
    const int cl = threadIdx.x % MC, jl = threadIdx.x / MC;
    const int c = blockIdx.x * MC + cl;
    double s = 0, ss = 0;
    if (c < C) {
        int j = jl;
        for (; j + 3 * MJ < gy; j += 4 * MJ) {
            const double a0 = partial[(long)j * 2 * C + c], b0 = partial[(long)j * 2 * C + C + c];
            const double a1 = partial[(long)(j + MJ) * 2 * C + c], b1 = partial[(long)(j + MJ) * 2 * C + C + c];
            const double a2 = partial[(long)(j + 2 * MJ) * 2 * C + c], b2 = partial[(long)(j + 2 * MJ) * 2 * C + C + c];
            const double a3 = partial[(long)(j + 3 * MJ) * 2 * C + c], b3 = partial[(long)(j + 3 * MJ) * 2 * C + C + c];
            s += (a0 + a1) + (a2 + a3);
            ss += (b0 + b1) + (b2 + b3);
        }
        for (; j < gy; j += MJ) {
            s += partial[(long)j * 2 * C + c];
            ss += partial[(long)j * 2 * C + C + c];
        }
    }
#pragma unroll
    for (int off = MC; off < 64; off <<= 1) {
        s += __shfl_xor(s, off, 64);
        ss += __shfl_xor(ss, off, 64);
    }
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
    const MomMap m = mom_map(M, C);
    return (size_t)m.gy * 2 * C * sizeof(double);
}

extern "C" int denet_bn_moments_accumulate(const float* x, double* acc, void* workspace, size_t workspace_bytes, long M, int C,
                                           hipStream_t stream) {
    DENET_CHECK_ARG(x && acc && workspace, "bn_moments_accumulate: null pointer");
    DENET_CHECK_ARG(M > 0 && C > 0 && C % 4 == 0, "bn_moments_accumulate: bad shape M=%ld C=%d", M, C);
    DENET_CHECK_ARG(workspace_bytes >= denet_bn_moments_workspace_bytes(M, C), "bn_moments_accumulate: workspace of %zu bytes < %zu",
                    workspace_bytes, denet_bn_moments_workspace_bytes(M, C));
    const MomMap m = mom_map(M, C);
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(bn_moments_partial_kernel, dim3(m.gx, m.gy), dim3(256), 0, stream, x, M, C, m.LC, partial);
    hipLaunchKernelGGL(bn_moments_fold_kernel, dim3((C + MC - 1) / MC), dim3(MOM_NT), 0, stream, x, (const double*)partial, m.gy, M,
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
