// The ORDER of a two-stage per-channel reduction over partial [rows][2][C] doubles: everything that decides which additions
// happen in which sequence, in one text. The bit identities the project promises - a batch norm's second stage inside the
// producing launch (bn_final.h) against the separate kernels (bn.hip), batch renormalisation (bn_renorm.hip) against the plain
// layer, the moments of model-update-bn (bn_moments.hip) from run to run - hold because every side compiles this file.
//   BnReduceMap, bn_map                                first stage: thread / grid mapping of an M x C pass, rows of the partial list
//   bn_reduce_workgroup_tail                           first stage: the workgroup's sums -> its row partial[blockIdx.y][2][C]
//   BNF_FC, BNF_FJ, bnf_load                           second stage: channels per wave, row lanes, one partial sum
//   bnf_reduce_partials(_multi), bnf_reduce_row_lanes  second stage: a lane's rows, then the lanes of a channel
//   bnf_finish_stats, bnf_finish_sums                  what the lane that holds a channel's sums writes
// (colsum_partial_kernel / colsum_final_kernel of elementwise.hip are NOT here: one sum in [gy][C], an LDS final, another order.)
#pragma once
#include "common.h"

struct BnReduceMap {
    int LC;      // lanes along channels (float4 units)
    int RS;      // rows handled concurrently by one workgroup
    int gx, gy;  // grid
};

// target: about how many workgroups the pass runs (bn.hip: 1024, ~4 per CU, keeps the second-stage reduction short;
// bn_moments.hip: 2048, 8 per CU for a memory-bound pass that grid-strides over the rest)
static inline BnReduceMap bn_map(long M, int C, int target) {
    BnReduceMap m;
    int c4 = C / 4;
    int lc = 1;
    while (lc < 256 && (c4 % (lc * 2)) == 0) lc *= 2;
    m.LC = lc;
    m.RS = 256 / lc;
    m.gx = c4 / lc;
    long rows_blocks = (M + m.RS - 1) / m.RS;
    int gy = target / m.gx;
    if (gy < 1) gy = 1;
    if (gy > rows_blocks) gy = (int)rows_blocks;
    m.gy = gy;
    return m;
}

// The end of a first-stage kernel of 256 threads mapped by bn_map (thread = channel lane cl = tid % LC, row slot rsub = tid / LC,
// owning the float4 of channels at c): s / ss are the thread's sums over its rows; the row slots of a channel lane are added in
// slot order through LDS (red: the kernel's __shared__ double [256 * 8]) and the workgroup's row partial[blockIdx.y][2][C] is
// written. Called by every thread.
__device__ __forceinline__ void bn_reduce_workgroup_tail(double (&s)[4], double (&ss)[4], double* red, int LC, int C, int c,
                                                         double* __restrict__ partial) {
    const int tid = threadIdx.x;
    const int cl = tid % LC, rsub = tid / LC, RS = 256 / LC;
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

// second stage: a one-wave workgroup reduces BNF_FC channels, BNF_FJ = 64/BNF_FC lanes stride over the partial rows and a shuffle tree
// adds them. The stage is latency bound (a few hundred KB, a chain of dependent row loads per lane): 32 row lanes keep the
// chain at gy/128 rounds of 4 loads in flight, C/2 workgroups spread it over the chip. NO LDS on purpose: these kernels run
// beside the persistent 64-channel Winograd kernels, whose workgroups hold a CU's whole LDS - a kernel that asks for any
// waits for one of them to retire (measured: 165 us instead of 7 for the six layer-1 finals of a step).
constexpr int BNF_FC = 2, BNF_FJ = 64 / BNF_FC;      // channels per wave, row lanes

typedef __attribute__((address_space(1))) unsigned long long bnf_gu64;

// a partial sum: plain, or (SC1, for the in-launch second stage of bn_final.h) a load past L1 and the XCD's L2
template <bool SC1>
__device__ __forceinline__ double bnf_load(const double* p) {
    if (SC1) return __longlong_as_double((long long)__hip_atomic_load((const bnf_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return *p;
}

__device__ __forceinline__ void bnf_reduce_row_lanes(double& s, double& ss) {
#pragma unroll
    for (int off = BNF_FC; off < 64; off <<= 1) {
        s += __shfl_xor(s, off, 64);
        ss += __shfl_xor(ss, off, 64);
    }
}

// lane (c, jl) of a wave: the sums over rows jl, jl + BNF_FJ, ... of column c (4 independent row loads in flight)
template <bool SC1>
__device__ __forceinline__ void bnf_reduce_partials(const double* __restrict__ partial, int gy, int C, int c, int jl, double& s,
                                                    double& ss) {
    s = 0;
    ss = 0;
    if (c < C) {
        int j = jl;
        for (; j + 3 * BNF_FJ < gy; j += 4 * BNF_FJ) {
            const double a0 = bnf_load<SC1>(partial + (long)j * 2 * C + c), b0 = bnf_load<SC1>(partial + (long)j * 2 * C + C + c);
            const double a1 = bnf_load<SC1>(partial + (long)(j + BNF_FJ) * 2 * C + c),
                         b1 = bnf_load<SC1>(partial + (long)(j + BNF_FJ) * 2 * C + C + c);
            const double a2 = bnf_load<SC1>(partial + (long)(j + 2 * BNF_FJ) * 2 * C + c),
                         b2 = bnf_load<SC1>(partial + (long)(j + 2 * BNF_FJ) * 2 * C + C + c);
            const double a3 = bnf_load<SC1>(partial + (long)(j + 3 * BNF_FJ) * 2 * C + c),
                         b3 = bnf_load<SC1>(partial + (long)(j + 3 * BNF_FJ) * 2 * C + C + c);
            s += (a0 + a1) + (a2 + a3);
            ss += (b0 + b1) + (b2 + b3);
        }
        for (; j < gy; j += BNF_FJ) {
            s += bnf_load<SC1>(partial + (long)j * 2 * C + c);
            ss += bnf_load<SC1>(partial + (long)j * 2 * C + C + c);
        }
    }
}

// the same sums for U columns c[0..U-1] of one lane at once: the loads of all U columns of a round are issued together (a wave
// that walks its column pairs one after the other is latency-bound: two dependent round trips per pair), the additions of every
// column are those of bnf_reduce_partials in the same order
template <bool SC1, int U>
__device__ __forceinline__ void bnf_reduce_partials_multi(const double* __restrict__ partial, int gy, int C, const int (&c)[U], int jl,
                                                          double (&s)[U], double (&ss)[U]) {
    int cs[U];          // (a column outside the tensor: a valid address is loaded - no exec-masked load, which would end the
                        // scheduling region and drain the loads in flight - and the caller drops the result)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        s[u] = ss[u] = 0;
        cs[u] = c[u] < C ? c[u] : 0;
    }
    int j = jl;
    // two groups of four rows per lane at a time (the loads of 2 x 4 x 2 x U values leave together: 256 rows - what a fused
    // kernel's launch leaves - are ONE round trip for the last workgroup, on whose latency the end of the launch waits)
    for (; j + 7 * BNF_FJ < gy; j += 8 * BNF_FJ) {
        double a[U][8], b[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const double* row = partial + (long)(j + r * BNF_FJ) * 2 * C;
                a[u][r] = bnf_load<SC1>(row + cs[u]);
                b[u][r] = bnf_load<SC1>(row + C + cs[u]);
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] += (a[u][0] + a[u][1]) + (a[u][2] + a[u][3]);
            ss[u] += (b[u][0] + b[u][1]) + (b[u][2] + b[u][3]);
            s[u] += (a[u][4] + a[u][5]) + (a[u][6] + a[u][7]);
            ss[u] += (b[u][4] + b[u][5]) + (b[u][6] + b[u][7]);
        }
    }
    for (; j + 3 * BNF_FJ < gy; j += 4 * BNF_FJ) {
        double a[U][4], b[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double* row = partial + (long)(j + r * BNF_FJ) * 2 * C;
                a[u][r] = bnf_load<SC1>(row + cs[u]);
                b[u][r] = bnf_load<SC1>(row + C + cs[u]);
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] += (a[u][0] + a[u][1]) + (a[u][2] + a[u][3]);
            ss[u] += (b[u][0] + b[u][1]) + (b[u][2] + b[u][3]);
        }
    }
    for (; j < gy; j += BNF_FJ) {
        double a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double* row = partial + (long)j * 2 * C;
            a[u] = bnf_load<SC1>(row + cs[u]);
            b[u] = bnf_load<SC1>(row + C + cs[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] += a[u];
            ss[u] += b[u];
        }
    }
}

// what the lane with jl == 0 does with the sums of channel c (the bodies of bn_stats_final_kernel / bn_bwd_final_kernel)
__device__ __forceinline__ void bnf_finish_stats(double s, double ss, long M, float eps, float momentum, int c,
                                                 float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                 float* __restrict__ run_mean, float* __restrict__ run_stdinv) {
    const double mean = s / (double)M;
    double var = ss / (double)M - mean * mean;  // biased variance (cuDNN)
    if (var < 0) var = 0;
    const float fmean = (float)mean;
    const float finv = (float)(1.0 / sqrt(var + (double)eps));
    save_mean[c] = fmean;
    save_invstd[c] = finv;
    if (run_mean) {
        // batch_norm.py:75-76: mean <- m*mean + (1-m)*batch_mean ; stdinv <- m*stdinv + (1-m)*batch_invstd
        const float om = (float)(1.0 - (double)momentum);
        run_mean[c] = momentum * run_mean[c] + om * fmean;
        run_stdinv[c] = momentum * run_stdinv[c] + om * finv;
    }
}
// dbeta = sum g ; dgamma = sum g*xhat ; coef[0][c] = dbeta/M ; coef[1][c] = dgamma/M
__device__ __forceinline__ void bnf_finish_sums(double s, double ss, long M, int C, int c, float* __restrict__ dgamma,
                                                float* __restrict__ dbeta, float* __restrict__ coef) {
    dbeta[c] = (float)s;
    dgamma[c] = (float)ss;
    coef[c] = (float)(s / (double)M);
    coef[C + c] = (float)(ss / (double)M);
}
