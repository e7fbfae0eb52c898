// GROUP NORMALISATION (Wu & He 2018) for the batch-norm layers whose model parameters ask for it (normGroups > 0: `BN.G[g, eps]`,
// `BNA.G[g, eps]`, the JSON key normGroups, model-modify --modify-bn-groups). Opt-in; every other layer never reaches this file.
// The reference has no such layer, so the definition below is the contract. x is NHWC [N][HW][C], G groups
// of Cg = C / G consecutive channels, m = HW * Cg; per sample n and group j, the same in training and inference:
//     mu = sum x / m      var = sum (x - mu)^2 / m (biased)      inv = 1 / sqrt(var + eps)
//     y = (x - mu) * (inv * gamma[c]) + beta[c]   [+ res]  [relu]
// With g = dy masked by the ReLU, xh = (x - mu) * inv, A[n,c] = sum_p g, B[n,c] = sum_p g * xh:
//     dbeta[c] = sum_n A      dgamma[c] = sum_n B      S1[n,j] = sum_{c in j} gamma[c] A[n,c]      S2[n,j] = sum_{c in j} gamma[c] B[n,c]
//     dx = inv * (gamma[c] * g - S1 / m - xh * S2 / m)      dres = g
// Three launches per direction, none of them with an atomic; every sum is accumulated in double in a fixed order:
//   gn_stats_partial_kernel / gn_bwd_partial_kernel   first stage: PER-SAMPLE column sums, partial [N][rows][2][C] doubles. A sample's
//                                  rows are split over gy workgroups (grid gx x gy x N), so N = 2 still fills the chip. The thread
//                                  mapping and the workgroup's tail are bn_reduce.h's (bn_map, bn_reduce_workgroup_tail).
//   gn_stats_finish_kernel         one wave per (n, j): folds the rows and the Cg channels of the group -> mu, inv (bnf_finish_stats)
//   gn_bwd_finish_kernel           the same wave per (n, j) -> S1 / m, S2 / m; further C / BNF_FC waves of the same launch reduce each
//                                  channel's rows sample by sample (bnf_reduce_partials + bnf_reduce_row_lanes) and add the samples
//                                  in ascending order -> dgamma, dbeta
//   gn_apply_kernel / gn_bwd_apply_kernel             the pointwise passes, float4 along C
// BATCH INDEPENDENCE: rows = gn_rows(HW, C) and every order above depend on (HW, C, G) only, never on N or on n; y[n], dx[n] and the
// saved statistics of a sample are the same bits whether it runs alone or inside any batch. Only the grids of the pointwise
// passes look at N.
// The pointwise expressions are NOT bn_pointwise.h's bn_affine (x * sc + (beta - mu * sc)): a group with m = 1 has x == mu and
// must give y == beta exactly, which only the centred form (x - mu) * sc + beta does; the gradient is evaluated without FMA
// contraction so that gamma * g - S1 / m cancels exactly there (dx == 0). bn_mask_y and the reduction pieces are shared.
#include "bn_reduce.h"
#include "bn_pointwise.h"
#include "../../include/denet_hip.h"
#include <math.h>

namespace {

constexpr int GN_WGS = 256;     // bn_map's target PER SAMPLE: a 128 x 128 x 64 sample is 256 workgroups of 4 rows per thread

// the rows a sample's first stage leaves: a function of (HW, C) alone
static inline BnReduceMap gn_map(long HW, int C) { return bn_map(HW, C, GN_WGS); }

// the pointwise passes write no sums: their grid may look at N (about 2048 workgroups in all)
static inline BnReduceMap gn_apply_map(int N, long HW, int C) {
    int t = 2048 / N;
    return bn_map(HW, C, t < 1 ? 1 : t);
}

struct GnQuad {
    float mu[4], is[4];     // the statistics of the group each of the four channels belongs to
    float ga[4], be[4];     // gamma, beta
    float sc[4];            // is * gamma
    float c1[4], c2[4];     // backward: S1 / m, S2 / m of the group
};

// stats: save_mean / save_invstd + n * G; channels c .. c + 3 may straddle groups when Cg % 4 != 0
__device__ __forceinline__ void gn_quad_load(GnQuad& q, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             const float* __restrict__ mean, const float* __restrict__ invstd, int c, int Cg) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = (c + k) / Cg;
        q.mu[k] = mean[j];
        q.is[k] = invstd[j];
        q.ga[k] = gamma[c + k];
        q.be[k] = beta ? beta[c + k] : 0.f;
        q.sc[k] = q.is[k] * q.ga[k];
    }
}
// coef [G][2] of the sample: S1 / m | S2 / m
__device__ __forceinline__ void gn_quad_load_coef(GnQuad& q, const float* __restrict__ coef, int c, int Cg) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = (c + k) / Cg;
        q.c1[k] = coef[2 * j];
        q.c2[k] = coef[2 * j + 1];
    }
}

__device__ __forceinline__ f32x4 gn_affine(const GnQuad& q, f32x4 x) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaf(x[k] - q.mu[k], q.sc[k], q.be[k]);
    return v;
}
__device__ __forceinline__ f32x4 gn_forward(const GnQuad& q, f32x4 x, bool has_res, f32x4 res, int relu) {
    f32x4 v = gn_affine(q, x);
    if (has_res) v += res;
    if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    return v;
}
__device__ __forceinline__ f32x4 gn_xhat(const GnQuad& q, f32x4 x) {
    f32x4 h;
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (x[k] - q.mu[k]) * q.is[k];
    return h;
}
// g where the ReLU passed: from the forward output, or recomputed from x with the forward's own expression
__device__ __forceinline__ f32x4 gn_mask(const GnQuad& q, f32x4 g, f32x4 x, const float* __restrict__ y, long o) {
    return y ? bn_mask_y(g, *(const f32x4*)(y + o)) : bn_mask_y(g, gn_affine(q, x));
}
// dx = inv * (gamma * g - S1 / m - xhat * S2 / m), every operation rounded on its own
__device__ __forceinline__ f32x4 gn_backward(const GnQuad& q, f32x4 g, f32x4 x) {
#pragma clang fp contract(off)
    const f32x4 xh = gn_xhat(q, x);
    f32x4 d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gg = q.ga[k] * g[k];
        const float t = xh[k] * q.c2[k];
        d[k] = q.is[k] * ((gg - q.c1[k]) - t);
    }
    return d;
}

// partial[n][gy][2][C] : sum(x), sum(x*x) of sample n = blockIdx.z over its HW rows
__global__ __launch_bounds__(256) void gn_stats_partial_kernel(const float* __restrict__ x, long HW, int C, int LC,
                                                               double* __restrict__ partial) {
    __shared__ double red[256 * 8];
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
    const int c = (blockIdx.x * LC + cl) * 4;
    const int n = blockIdx.z;
    const float* xs = x + (long)n * HW * C;
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    for (long r = (long)blockIdx.y * RS + rsub; r < HW; r += (long)gridDim.y * RS) {
        const f32x4 v = *(const f32x4*)(xs + r * C + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)v[k];
            s[k] += d;
            ss[k] += d * d;
        }
    }
    bn_reduce_workgroup_tail(s, ss, red, LC, C, c, partial + (long)n * gridDim.y * 2 * C);
}

// the sums of group j of one sample: lane l adds the elements l, l + 64, ... of the flattened (row, channel of the group) list,
// four independent loads in flight, then a shuffle tree over the wave. WEIGHTED: each element times gamma of its channel
template <bool WEIGHTED>
__device__ __forceinline__ void gn_reduce_group(const double* __restrict__ p, int rows, int C, int Cg,
                                                const float* __restrict__ gamma, double& s, double& ss) {
    const int total = rows * Cg;
    const int lane = threadIdx.x;
    s = 0;
    ss = 0;
    auto load = [&](int e, double& a, double& b) {
        const int r = e / Cg, ci = e - r * Cg;
        const double w = WEIGHTED ? (double)gamma[ci] : 1.0;
        a = p[(long)r * 2 * C + ci];
        b = p[(long)r * 2 * C + C + ci];
        if (WEIGHTED) {
            a *= w;
            b *= w;
        }
    };
    int e = lane;
    for (; e + 192 < total; e += 256) {
        double a0, b0, a1, b1, a2, b2, a3, b3;
        load(e, a0, b0);
        load(e + 64, a1, b1);
        load(e + 128, a2, b2);
        load(e + 192, a3, b3);
        s += (a0 + a1) + (a2 + a3);
        ss += (b0 + b1) + (b2 + b3);
    }
    for (; e < total; e += 64) {
        double a, b;
        load(e, a, b);
        s += a;
        ss += b;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        s += __shfl_xor(s, off, 64);
        ss += __shfl_xor(ss, off, 64);
    }
}

// one wave per (n, j): save_mean / save_invstd [N * G]
__global__ __launch_bounds__(64) void gn_stats_finish_kernel(const double* __restrict__ partial, int rows, int C, int G, long HW,
                                                             float eps, float* __restrict__ save_mean,
                                                             float* __restrict__ save_invstd) {
    const int n = blockIdx.x / G, j = blockIdx.x - n * G;
    const int Cg = C / G;
    double s, ss;
    gn_reduce_group<false>(partial + (long)n * rows * 2 * C + j * Cg, rows, C, Cg, nullptr, s, ss);
    if (threadIdx.x != 0) return;
    bnf_finish_stats(s, ss, HW * Cg, eps, 0.f, blockIdx.x, save_mean, save_invstd, nullptr, nullptr);
}

// y = relu?( (x - mu) * inv * gamma + beta (+ res) ), sample n = blockIdx.z
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                       float* __restrict__ y, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, long HW, int C, int G, int LC, int relu) {
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
    const int c = (blockIdx.x * LC + cl) * 4;
    const int n = blockIdx.z;
    GnQuad q;
    gn_quad_load(q, gamma, beta, mean + (long)n * G, invstd + (long)n * G, c, C / G);
    const long base = (long)n * HW * C;
    for (long r = (long)blockIdx.y * RS + rsub; r < HW; r += (long)gridDim.y * RS) {
        const long o = base + r * C + c;
        f32x4 rv = {0.f, 0.f, 0.f, 0.f};
        if (res) rv = *(const f32x4*)(res + o);
        *(f32x4*)(y + o) = gn_forward(q, *(const f32x4*)(x + o), res != nullptr, rv, relu);
    }
}

// partial[n][gy][2][C] : A = sum(g), B = sum(g * xhat) of sample n over its HW rows
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, long HW, int C, int G, int LC,
                                                             int relu, double* __restrict__ partial) {
    __shared__ double red[256 * 8];
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
    const int c = (blockIdx.x * LC + cl) * 4;
    const int n = blockIdx.z;
    GnQuad q;
    gn_quad_load(q, gamma, beta, mean + (long)n * G, invstd + (long)n * G, c, C / G);
    const long base = (long)n * HW * C;
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    for (long r = (long)blockIdx.y * RS + rsub; r < HW; r += (long)gridDim.y * RS) {
        const long o = base + r * C + c;
        const f32x4 xv = *(const f32x4*)(x + o);
        f32x4 g = *(const f32x4*)(dy + o);
        if (relu) g = gn_mask(q, g, xv, y, o);
        const f32x4 xh = gn_xhat(q, xv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] += (double)g[k];
            ss[k] += (double)g[k] * (double)xh[k];
        }
    }
    bn_reduce_workgroup_tail(s, ss, red, LC, C, c, partial + (long)n * gridDim.y * 2 * C);
}

// workgroups [0, N * G): (n, j) -> coef[n][j][2] = S1 / m | S2 / m. Workgroups behind them: BNF_FC channels each, the rows of a
// sample in bn_bwd_final_kernel's order, the samples added in ascending order -> dgamma, dbeta (written, not accumulated)
__global__ __launch_bounds__(64) void gn_bwd_finish_kernel(const double* __restrict__ partial, int rows, int N, int C, int G, long HW,
                                                           const float* __restrict__ gamma, float* __restrict__ coef,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int NG = N * G;
    if ((int)blockIdx.x < NG) {
        const int n = blockIdx.x / G, j = blockIdx.x - n * G;
        const int Cg = C / G;
        double s, ss;
        gn_reduce_group<true>(partial + (long)n * rows * 2 * C + j * Cg, rows, C, Cg, gamma + j * Cg, s, ss);
        if (threadIdx.x != 0) return;
        const double m = (double)(HW * Cg);
        coef[2 * (long)blockIdx.x] = (float)(s / m);
        coef[2 * (long)blockIdx.x + 1] = (float)(ss / m);
        return;
    }
    const int cl = threadIdx.x % BNF_FC, jl = threadIdx.x / BNF_FC;
    const int c = ((int)blockIdx.x - NG) * BNF_FC + cl;
    double ts = 0, tss = 0;
    for (int n = 0; n < N; ++n) {
        double s, ss;
        bnf_reduce_partials<false>(partial + (long)n * rows * 2 * C, rows, C, c, jl, s, ss);
        bnf_reduce_row_lanes(s, ss);
        ts += s;
        tss += ss;
    }
    if (jl != 0 || c >= C) return;
    dbeta[c] = (float)ts;
    dgamma[c] = (float)tss;
}

// dx = inv * (gamma * g - S1 / m - xhat * S2 / m) ; optional dres = g ; sample n = blockIdx.z
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ dy, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ coef,
                                                           float* __restrict__ dx, float* __restrict__ dres, long HW, int C, int G,
                                                           int LC, int relu) {
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
    const int c = (blockIdx.x * LC + cl) * 4;
    const int n = blockIdx.z;
    GnQuad q;
    gn_quad_load(q, gamma, beta, mean + (long)n * G, invstd + (long)n * G, c, C / G);
    gn_quad_load_coef(q, coef + 2 * (long)n * G, c, C / G);
    const long base = (long)n * HW * C;
    for (long r = (long)blockIdx.y * RS + rsub; r < HW; r += (long)gridDim.y * RS) {
        const long o = base + r * C + c;
        const f32x4 xv = *(const f32x4*)(x + o);
        f32x4 g = *(const f32x4*)(dy + o);
        if (relu) g = gn_mask(q, g, xv, y, o);
        *(f32x4*)(dx + o) = gn_backward(q, g, xv);
        if (dres) *(f32x4*)(dres + o) = g;
    }
}

// workspace: partial [N][rows][2][C] doubles | coef [N][G][2] floats (room for G = C) | fallback save_mean, save_invstd [N][C]
static inline size_t gn_partial_doubles(int N, long HW, int C) { return (size_t)N * gn_map(HW, C).gy * 2 * C; }

static bool gn_shape_ok(int N, long HW, int C, int G) {
    return N > 0 && N <= 65535 && HW > 0 && HW < (1L << 31) && C > 0 && C % 4 == 0 && G > 0 && C % G == 0 &&
           (long)N * G < (1L << 31) - C && (long)gn_map(HW, C).gy * C < (1L << 30);
}

}  // namespace

extern "C" size_t denet_gn_workspace_bytes(int N, long HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0 || C % 4) return 0;
    return gn_partial_doubles(N, HW, C) * sizeof(double) + (size_t)4 * N * C * sizeof(float);
}

// forward, training and inference alike. save_mean / save_invstd [N * G]: NULL (both) keeps them in the workspace.
// ops.kernel_symbol: kinds 42 / 43 / 44 = the three launches
extern "C" int denet_gn_fwd(const float* x, const float* res, float* y, const float* gamma, const float* beta, float* save_mean,
                            float* save_invstd, void* workspace, int N, long HW, int C, int G, float eps, int relu,
                            hipStream_t stream) {
    DENET_CHECK_ARG(x && y && gamma && beta && workspace, "gn_fwd: null pointer");
    DENET_CHECK_ARG(!save_mean == !save_invstd, "gn_fwd: save_mean and save_invstd are given together or not at all");
    DENET_CHECK_ARG(gn_shape_ok(N, HW, C, G), "gn_fwd: bad shape N=%d HW=%ld C=%d G=%d (C a multiple of 4 and of G)", N, HW, C, G);
    DENET_CHECK_ARG(eps > 0.0f && isfinite(eps), "gn_fwd: eps = %g must be positive and finite", (double)eps);
    const BnReduceMap m = gn_map(HW, C);
    double* partial = (double*)workspace;
    float* tail = (float*)(partial + gn_partial_doubles(N, HW, C));
    if (!save_mean) {
        save_mean = tail + 2 * (size_t)N * C;
        save_invstd = tail + 3 * (size_t)N * C;
    }
    int prof = denet_prof_begin(42, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_stats_partial_kernel, dim3(m.gx, m.gy, N), dim3(256), 0, stream, x, HW, C, m.LC, partial);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(43, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_stats_finish_kernel, dim3(N * G), dim3(64), 0, stream, partial, m.gy, C, G, HW, eps, save_mean, save_invstd);
    denet_prof_end(prof, stream);
    const BnReduceMap a = gn_apply_map(N, HW, C);
    prof = denet_prof_begin(44, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(a.gx, a.gy, N), dim3(256), 0, stream, x, res, y, gamma, beta, save_mean, save_invstd, HW, C,
                       G, a.LC, relu);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("gn_fwd");
    return DENET_OK;
}

// its gradient. y: the forward output where the ReLU mask needs it (a residual was added), else NULL (recomputed from x, needs
// beta). dres: NULL or the masked gradient. dgamma / dbeta are WRITTEN. ops.kernel_symbol: kinds 45 / 46 / 47
extern "C" int denet_gn_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta,
                            void* workspace, int N, long HW, int C, int G, int relu, hipStream_t stream) {
    DENET_CHECK_ARG(x && dy && gamma && save_mean && save_invstd && dx && dgamma && dbeta && workspace, "gn_bwd: null pointer");
    DENET_CHECK_ARG(!relu || y || beta, "gn_bwd: the relu mask needs the forward output y, or beta to recompute it");
    DENET_CHECK_ARG(gn_shape_ok(N, HW, C, G), "gn_bwd: bad shape N=%d HW=%ld C=%d G=%d (C a multiple of 4 and of G)", N, HW, C, G);
    const BnReduceMap m = gn_map(HW, C);
    double* partial = (double*)workspace;
    float* coef = (float*)(partial + gn_partial_doubles(N, HW, C));
    int prof = denet_prof_begin(45, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(m.gx, m.gy, N), dim3(256), 0, stream, x, y, dy, gamma, beta, save_mean, save_invstd,
                       HW, C, G, m.LC, relu, partial);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(46, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3(N * G + (C + BNF_FC - 1) / BNF_FC), dim3(64), 0, stream, partial, m.gy, N, C, G, HW,
                       gamma, coef, dgamma, dbeta);
    denet_prof_end(prof, stream);
    const BnReduceMap a = gn_apply_map(N, HW, C);
    prof = denet_prof_begin(47, 0, 0, 0, stream);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(a.gx, a.gy, N), dim3(256), 0, stream, x, y, dy, gamma, beta, save_mean, save_invstd,
                       coef, dx, dres, HW, C, G, a.LC, relu);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("gn_bwd");
    return DENET_OK;
}
