// The smooth `A` activations of the reference (denet/layer/activation.py:25-44) on channel-padded NHWC fp32 tensors:
//   sigmoid (:28-29), elu with alpha = 1 (:35-36), tanh (:37-38), softplus (:41-42); relu / relu-safe stay in elementwise.hip.
// A tensor is [M][CP] with C logical channels (M = batch x pixels, CP = C rounded up). The consumers of a tensor rely on
// zeros in channels C..CP-1, and f(0) != 0 for sigmoid and softplus (f'(0) != 0 for all four), so every kernel here writes
// +0.0f to those lanes whatever they hold on input.
// The derivatives are written from the forward OUTPUT y, like relu_bwd: the layer keeps one tensor alive, the pass reads two.
#include "common.h"
#include <math.h>

#include "../../include/denet_hip.h"

namespace {

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// no overflow for any finite x: the exponentials only ever see -|x|
template <int KIND>
__device__ __forceinline__ float act_f(float x) {
    if (KIND == DENET_ACT_SIGMOID) {
        const float t = expf(-fabsf(x));            // in [0, 1]
        const float r = 1.0f / (1.0f + t);
        return x >= 0.f ? r : t * r;
    } else if (KIND == DENET_ACT_TANH) {
        return tanhf(x);
    } else if (KIND == DENET_ACT_ELU) {
        return x > 0.f ? x : expm1f(x);
    } else {
        // softplus: max(x, 0) + log1p(t), t = exp(-|x|) in [0, 1]. log1p(t) = log(u) * t / (u - 1) with u = fl(1 + t) (u - 1 is
        // exact, and the quotient undoes the rounding of u to first order); u == 1: log1p(t) = t to fp32. The library's log1pf made
        // this pass 2.5 times as long as the ReLU pass (EXPERIMENTS.md).
        const float t = expf(-fabsf(x));
        const float u = 1.0f + t;
        const float d = u - 1.0f;
        const float l = d == 0.f ? t : logf(u) * (t / d);
        return fmaxf(x, 0.f) + l;
    }
}

// d act / dx as a function of y = act(x)
template <int KIND>
__device__ __forceinline__ float act_df(float y) {
    if (KIND == DENET_ACT_SIGMOID) {
        return y * (1.0f - y);
    } else if (KIND == DENET_ACT_TANH) {
        return 1.0f - y * y;
    } else if (KIND == DENET_ACT_ELU) {
        return y > 0.f ? 1.0f : y + 1.0f;
    } else {                                          // 1 - exp(-y) = sigmoid(x)
        return -expm1f(-y);
    }
}

// first channel of the four that vector i of a [M][CP] tensor holds (i < 2^31, checked by the callers)
__device__ __forceinline__ int chan_of(uint32_t i, const FastDiv& cp4) {
    return (int)(i - cp4.div(i) * cp4.d) * 4;
}

// y = act(x); ADD: y = act(a + b).  MASK: C < CP, lanes >= C are written as +0
template <int KIND, bool ADD, bool MASK>
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      float* __restrict__ y, long n4, int C, FastDiv cp4) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 v = ((const f32x4*)a)[i];
        if (ADD) v += ((const f32x4*)b)[i];
        const int c = MASK ? chan_of((uint32_t)i, cp4) : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float r = act_f<KIND>(v[k]);
            v[k] = (!MASK || c + k < C) ? r : 0.f;
        }
        ((f32x4*)y)[i] = v;
    }
}

// dx = dy * act'(y)
template <int KIND, bool MASK>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                      float* __restrict__ dx, long n4, int C, FastDiv cp4) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 yv = ((const f32x4*)y)[i];
        f32x4 g = ((const f32x4*)dy)[i];
        const int c = MASK ? chan_of((uint32_t)i, cp4) : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float r = g[k] * act_df<KIND>(yv[k]);
            g[k] = (!MASK || c + k < C) ? r : 0.f;
        }
        ((f32x4*)dx)[i] = g;
    }
}

bool shape_ok(long M, int C, int CP) {
    return M >= 0 && C >= 1 && CP >= C && CP % 4 == 0 && M * (CP / 4) < (1L << 31);
}

bool kind_ok(int kind) { return kind >= DENET_ACT_SIGMOID && kind <= DENET_ACT_SOFTPLUS; }

template <int KIND, bool ADD>
void launch_fwd(const float* a, const float* b, float* y, long n4, int C, int CP, hipStream_t stream) {
    FastDiv cp4;
    cp4.init((uint32_t)(CP / 4));
    if (C < CP)
        hipLaunchKernelGGL((act_fwd_kernel<KIND, ADD, true>), dim3(grid_for(n4)), dim3(256), 0, stream, a, b, y, n4, C, cp4);
    else
        hipLaunchKernelGGL((act_fwd_kernel<KIND, ADD, false>), dim3(grid_for(n4)), dim3(256), 0, stream, a, b, y, n4, C, cp4);
}

template <bool ADD>
void dispatch_fwd(const float* a, const float* b, float* y, long n4, int C, int CP, int kind, hipStream_t stream) {
    switch (kind) {
        case DENET_ACT_SIGMOID: launch_fwd<DENET_ACT_SIGMOID, ADD>(a, b, y, n4, C, CP, stream); break;
        case DENET_ACT_TANH: launch_fwd<DENET_ACT_TANH, ADD>(a, b, y, n4, C, CP, stream); break;
        case DENET_ACT_ELU: launch_fwd<DENET_ACT_ELU, ADD>(a, b, y, n4, C, CP, stream); break;
        default: launch_fwd<DENET_ACT_SOFTPLUS, ADD>(a, b, y, n4, C, CP, stream); break;
    }
}

template <int KIND>
void launch_bwd(const float* y, const float* dy, float* dx, long n4, int C, int CP, hipStream_t stream) {
    FastDiv cp4;
    cp4.init((uint32_t)(CP / 4));
    if (C < CP)
        hipLaunchKernelGGL((act_bwd_kernel<KIND, true>), dim3(grid_for(n4)), dim3(256), 0, stream, y, dy, dx, n4, C, cp4);
    else
        hipLaunchKernelGGL((act_bwd_kernel<KIND, false>), dim3(grid_for(n4)), dim3(256), 0, stream, y, dy, dx, n4, C, cp4);
}

}  // namespace

extern "C" int denet_act_fwd(const float* x, float* y, long M, int C, int CP, int kind, hipStream_t stream) {
    DENET_CHECK_ARG(x && y && shape_ok(M, C, CP), "act_fwd: bad args (M=%ld C=%d CP=%d)", M, C, CP);
    DENET_CHECK_ARG(kind_ok(kind), "act_fwd: unknown activation kind %d", kind);
    if (M == 0) return DENET_OK;
    dispatch_fwd<false>(x, nullptr, y, M * (CP / 4), C, CP, kind, stream);
    DENET_CHECK_LAUNCH("act_fwd");
    return DENET_OK;
}

extern "C" int denet_add_act_fwd(const float* a, const float* b, float* y, long M, int C, int CP, int kind,
                                 hipStream_t stream) {
    DENET_CHECK_ARG(a && b && y && shape_ok(M, C, CP), "add_act_fwd: bad args (M=%ld C=%d CP=%d)", M, C, CP);
    DENET_CHECK_ARG(kind_ok(kind), "add_act_fwd: unknown activation kind %d", kind);
    if (M == 0) return DENET_OK;
    dispatch_fwd<true>(a, b, y, M * (CP / 4), C, CP, kind, stream);
    DENET_CHECK_LAUNCH("add_act_fwd");
    return DENET_OK;
}

extern "C" int denet_act_bwd(const float* y, const float* dy, float* dx, long M, int C, int CP, int kind,
                             hipStream_t stream) {
    DENET_CHECK_ARG(y && dy && dx && shape_ok(M, C, CP), "act_bwd: bad args (M=%ld C=%d CP=%d)", M, C, CP);
    DENET_CHECK_ARG(kind_ok(kind), "act_bwd: unknown activation kind %d", kind);
    if (M == 0) return DENET_OK;
    const long n4 = M * (CP / 4);
    switch (kind) {
        case DENET_ACT_SIGMOID: launch_bwd<DENET_ACT_SIGMOID>(y, dy, dx, n4, C, CP, stream); break;
        case DENET_ACT_TANH: launch_bwd<DENET_ACT_TANH>(y, dy, dx, n4, C, CP, stream); break;
        case DENET_ACT_ELU: launch_bwd<DENET_ACT_ELU>(y, dy, dx, n4, C, CP, stream); break;
        default: launch_bwd<DENET_ACT_SOFTPLUS>(y, dy, dx, n4, C, CP, stream); break;
    }
    DENET_CHECK_LAUNCH("act_bwd");
    return DENET_OK;
}
