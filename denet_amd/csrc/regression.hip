// Soft-max classification over chosen pixels of a spatial logit map (the `R` layer's view path). Reference:
// denet/layer/regression.py - the logits of the V pixels in `valid` are gathered into (B, C, V) (:31-35), log_softmax over the
// classes (:40, :64-66), output = the softmax averaged over the views (:45-47), cost = -mean of the log-probability of the
// sample's class (:97-98).
//
// Logits are NHWC [B][HW][CP] fp32 (C real classes in CP physical channels); `offsets` holds the V pixel indices (y * W + x)
// of the views, fixed when the layer is built and distinct; `cls` the class of every sample.
//
// loss:  1. zero: the gradient map [B][HW][CP] is cleared with vector stores (padding channels and non-view pixels stay 0).
//        2. rows: one wave64 per (b, view) row: max and log-sum-exp over the C classes (lanes stride over C, any C), the row's
//           NLL into a slab of doubles, and the gradient (softmax - onehot) / (B * V) at that pixel.
//        3. finish: one workgroup sums the slab in a fixed order: costs[0] = mean NLL, costs[1] = 0.
//        No atomics: the cost and the gradient are bitwise the same from run to run.
// probs: one wave per sample: for v = 0 .. V-1 in order, softmax of the view added into pr[b][c]; then pr /= V.
#include "common.h"
#include "../../include/denet_hip.h"

namespace {

constexpr int RG_NT = 256, RG_WAVES = RG_NT / 64;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(RG_NT) void regression_zero_kernel(float* __restrict__ out, long n4) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * RG_NT + threadIdx.x; i < n4; i += (long)gridDim.x * RG_NT) ((f32x4*)out)[i] = z;
}

__global__ __launch_bounds__(RG_NT) void regression_loss_kernel(const float* __restrict__ logits, const int* __restrict__ offsets,
                                                                const int* __restrict__ cls, float* __restrict__ dlogits,
                                                                double* __restrict__ nll, int rows, int V, int HW, int CP, int C,
                                                                float scale) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = r / V, v = r - b * V;
    const long base = ((long)b * HW + offsets[v]) * CP;
    const float* z = logits + base;
    const int t = cls[b];
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(z[c] - mx);
    se = wave_sum(se);
    const float lse = logf(se);
    const bool ok = t >= 0 && t < C;                 // a class outside [0, C) makes the cost NaN instead of reading past the row
    if (lane == 0) nll[r] = ok ? -(double)((z[t] - mx) - lse) : (double)NAN;
    if (dlogits) {
        float* dz = dlogits + base;
        for (int c = lane; c < C; c += 64) {
            const float p = expf((z[c] - mx) - lse);
            dz[c] = scale * (p - (c == t ? 1.f : 0.f));
        }
    }
}

// costs[0] = sum(nll[0..n)) / n, summed in a fixed order; costs[1] = 0
__global__ __launch_bounds__(RG_NT) void regression_finish_kernel(const double* __restrict__ nll, int n, float* __restrict__ costs) {
    __shared__ double red[RG_NT];
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += RG_NT) acc += nll[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = RG_NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 2) costs[threadIdx.x] = threadIdx.x == 0 ? (float)(red[0] / (double)n) : 0.f;
}

__global__ __launch_bounds__(RG_NT) void regression_probs_kernel(const float* __restrict__ logits, const int* __restrict__ offsets,
                                                                 float* __restrict__ pr, int B, int V, int HW, int CP, int C) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * RG_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;
    float* out = pr + (long)b * C;
    for (int v = 0; v < V; ++v) {
        const float* z = logits + ((long)b * HW + offsets[v]) * CP;
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
        mx = wave_max(mx);
        float se = 0.f;
        for (int c = lane; c < C; c += 64) se += expf(z[c] - mx);
        se = wave_sum(se);
        const float lse = logf(se);
        // every lane owns the same classes in every view: its own read-modify-write, no race
        for (int c = lane; c < C; c += 64) {
            const float p = expf((z[c] - mx) - lse);
            out[c] = v == 0 ? p : out[c] + p;
        }
    }
    for (int c = lane; c < C; c += 64) out[c] = out[c] / (float)V;
}

}  // namespace

extern "C" size_t denet_regression_workspace_bytes(int B, int V) {
    if (B <= 0 || V <= 0) return 0;
    return (size_t)B * V * sizeof(double);
}

extern "C" int denet_regression_loss(const float* logits, const int* offsets, const int* cls, float* dlogits, float* costs,
                                     void* workspace, size_t workspace_bytes, int B, int HW, int CP, int C, int V,
                                     hipStream_t stream) {
    DENET_CHECK_ARG(logits && offsets && cls && costs && workspace, "regression_loss: null pointer");
    DENET_CHECK_ARG(B > 0 && HW > 0 && V > 0 && V <= HW && C > 0 && C <= CP && CP % 4 == 0,
                    "regression_loss: bad shape B=%d HW=%d CP=%d C=%d V=%d", B, HW, CP, C, V);
    DENET_CHECK_ARG((long)B * V <= 0x7fffffffL && (long)B * HW * CP <= 0x7fffffffffL, "regression_loss: too large");
    DENET_CHECK_ARG(workspace_bytes >= denet_regression_workspace_bytes(B, V), "regression_loss: workspace of %zu bytes < %zu",
                    workspace_bytes, denet_regression_workspace_bytes(B, V));
    const int rows = B * V;
    if (dlogits) {
        const long n4 = (long)B * HW * CP / 4;
        const long g = (n4 + RG_NT - 1) / RG_NT;
        hipLaunchKernelGGL(regression_zero_kernel, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(RG_NT), 0, stream, dlogits, n4);
    }
    hipLaunchKernelGGL(regression_loss_kernel, dim3((rows + RG_WAVES - 1) / RG_WAVES), dim3(RG_NT), 0, stream, logits, offsets, cls,
                       dlogits, (double*)workspace, rows, V, HW, CP, C, (float)(1.0 / (double)rows));
    hipLaunchKernelGGL(regression_finish_kernel, dim3(1), dim3(RG_NT), 0, stream, (const double*)workspace, rows, costs);
    DENET_CHECK_LAUNCH("regression_loss");
    return DENET_OK;
}

extern "C" int denet_regression_probs(const float* logits, const int* offsets, float* pr, int B, int HW, int CP, int C, int V,
                                      hipStream_t stream) {
    DENET_CHECK_ARG(logits && offsets && pr, "regression_probs: null pointer");
    DENET_CHECK_ARG(B > 0 && HW > 0 && V > 0 && V <= HW && C > 0 && C <= CP, "regression_probs: bad shape B=%d HW=%d CP=%d C=%d V=%d",
                    B, HW, CP, C, V);
    hipLaunchKernelGGL(regression_probs_kernel, dim3((B + RG_WAVES - 1) / RG_WAVES), dim3(RG_NT), 0, stream, logits, offsets, pr, B,
                       V, HW, CP, C);
    DENET_CHECK_LAUNCH("regression_probs");
    return DENET_OK;
}
