// The pointwise expressions of a batch-norm layer (+ ReLU / residual add), forward and backward, each in one text, for a
// float4 of channels. The kernels that evaluate a batch norm inside another pass - the linked Winograd transforms and the
// backward sums of the output transform (winograd.hip), the pooled forms of bn.hip - promise the bits of bn_apply_kernel /
// bn_bwd_partial_kernel / bn_bwd_apply_kernel: they do because every one of them calls the functions below. Both files compile
// with FMA contraction on, so two typed-out copies of g - mg - xh * mgx agree only while the compiler contracts them alike.
//   BnQuad, bn_quad_load(_coef)    per-channel coefficients of channels c .. c + 3
//   bn_affine, bn_forward          x * sc + sh;  relu?(x * sc + sh (+ res))
//   bn_mask_y, bn_mask_x           g where the layer's ReLU passed: from the forward output, or recomputed from x
//   bn_xhat                        (x - mean) * invstd
//   bn_backward                    sc * (g - mean(g) - xhat * mean(g * xhat))
// Reference: denet/layer/batch_norm.py:50-79, batch_norm_relu.py:34-54 (gradient masked by xn > 0, then cuDNN's BN gradient).
// (The MFMA kernels' epilogues - igemm.hip, wino2f.hip, wino4f.hip, wino4t.hip, dgrad_s2.hip - and elementwise.hip keep their own.)
#pragma once
#include "common.h"

struct BnQuad {
    float mu[4], is[4];     // mean, 1 / std
    float sc[4], sh[4];     // y = x * sc + sh: sc = gamma * invstd, sh = beta - mean * sc
    float mg[4], mgx[4];    // backward (bn_quad_load_coef): mean(g), mean(g * xhat)
};

// GAMMA_OPT / BETA_OPT: the pointer may be NULL and then stands for 1 / 0 (a backward pass whose mask comes from the forward
// output needs no beta, and backward sums - wino_output_kernel - with such a mask no gamma either). A kernel whose launchers
// check the pointer leaves the flag off and compiles no NULL case in.
template <bool GAMMA_OPT = false, bool BETA_OPT = false>
__device__ __forceinline__ void bn_quad_load(BnQuad& q, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             const float* __restrict__ mean, const float* __restrict__ invstd, int c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q.mu[k] = mean[c + k];
        q.is[k] = invstd[c + k];
        q.sc[k] = (!GAMMA_OPT || gamma ? gamma[c + k] : 1.f) * q.is[k];
        q.sh[k] = (!BETA_OPT || beta ? beta[c + k] : 0.f) - q.mu[k] * q.sc[k];
    }
}
// coef [2][C]: the two means of the backward pass (bn_bwd_final_kernel)
__device__ __forceinline__ void bn_quad_load_coef(BnQuad& q, const float* __restrict__ coef, int C, int c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q.mg[k] = coef[c + k];
        q.mgx[k] = coef[C + c + k];
    }
}

__device__ __forceinline__ f32x4 bn_affine(const BnQuad& q, f32x4 x) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaf(x[k], q.sc[k], q.sh[k]);
    return v;
}

// y = relu?( gamma * (x - mean) * invstd + beta (+ res) ); res is read only where has_res
__device__ __forceinline__ f32x4 bn_forward(const BnQuad& q, f32x4 x, bool has_res, f32x4 res, int relu) {
    f32x4 v = bn_affine(q, x);
    if (has_res) v += res;
    if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    return v;
}

// the gradient where the ReLU behind the layer passed: y > 0 with the forward output, else recomputed from x with the
// forward's own expression (bit-identical, saves reading y)
__device__ __forceinline__ f32x4 bn_mask_y(f32x4 g, f32x4 y) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = y[k] > 0.f ? g[k] : 0.f;
    return g;
}
__device__ __forceinline__ f32x4 bn_mask_x(const BnQuad& q, f32x4 g, f32x4 x) {
    return bn_mask_y(g, bn_affine(q, x));
}

__device__ __forceinline__ f32x4 bn_xhat(const BnQuad& q, f32x4 x) {
    f32x4 h;
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (x[k] - q.mu[k]) * q.is[k];
    return h;
}

// dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))
__device__ __forceinline__ f32x4 bn_backward(const BnQuad& q, f32x4 g, f32x4 x) {
    const f32x4 xh = bn_xhat(q, x);
    f32x4 d;
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = q.sc[k] * (g[k] - q.mg[k] - xh[k] * q.mgx[k]);
    return d;
}
