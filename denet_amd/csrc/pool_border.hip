// Border-keeping pooling (`P.B` / `P.AB`, ignore_border = False), NHWC fp32.
//   reference denet/layer/pool.py:39-40: theano.tensor.signal.pool.pool_2d(..., ignore_border=False), no padding.
//   Window (oy, ox) covers rows oy*sh .. min(oy*sh + kh, H) - 1 and columns ox*sw .. min(ox*sw + kw, W) - 1: it is clipped
//   at the bottom and right edge. max: the maximum over the clipped window; average_inc_pad: the sum over the clipped window
//   divided by the number of taps IN THE CLIPPED WINDOW (there is no padding to include).
//   Gradients (gather form, no atomics, no argmax tensor):
//     max     : every tap EQUAL to its window's maximum receives the window's gradient. ASSUMPTION: this is the rule of Theano's
//               host MaxPoolGrad as read, not executed; the cuDNN path of pool.hip records one argmax tap.
//     average : every tap of a window receives dy / count(window).
// The window is given per axis. All HBM-bound; one thread per float4 of channels per pixel, grid-stride, as pool.hip.
#include "common.h"
#include "../../include/denet_hip.h"

namespace {

template <bool MAX>
__global__ __launch_bounds__(256) void pool_border_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H,
                                                              int W, int C, int OH, int OW, int kh, int kw, int sh, int sw) {
    const int C4 = C / 4;
    const long total = (long)N * OH * OW * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long t = i / C4;
        const int ox = (int)(t % OW);
        t /= OW;
        const int oy = (int)(t % OH);
        const int n = (int)(t / OH);
        // the entry point has checked (OH - 1) * sh < H and (OW - 1) * sw < W: no window is empty
        const int y0 = oy * sh, x0 = ox * sw;
        const int y1 = min(y0 + kh, H), x1 = min(x0 + kw, W);
        f32x4 acc;
        if (MAX)
            acc = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        else
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int iy = y0; iy < y1; ++iy) {
            const float* row = x + (((long)n * H + iy) * W) * C + c4 * 4;
            for (int ix = x0; ix < x1; ++ix) {
                const f32x4 v = *(const f32x4*)(row + (long)ix * C);
                if (MAX) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = v[e] > acc[e] ? v[e] : acc[e];
                } else {
                    acc += v;
                }
            }
        }
        if (!MAX) acc = acc / (float)((y1 - y0) * (x1 - x0));
        *(f32x4*)(y + i * 4) = acc;
    }
}

// one thread per input float4: the sum over the windows that cover it
template <bool MAX>
__global__ __launch_bounds__(256) void pool_border_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                              int H, int W, int C, int OH, int OW, int kh, int kw, int sh,
                                                              int sw) {
    const int C4 = C / 4;
    const long total = (long)N * H * W * C4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4);
        long t = i / C4;
        const int ix = (int)(t % W);
        t /= W;
        const int iy = (int)(t % H);
        const int n = (int)(t / H);
        // windows oy with oy*sh <= iy <= oy*sh + kh - 1
        int oy_lo = iy - kh + 1 + sh - 1;
        oy_lo = oy_lo < 0 ? 0 : oy_lo / sh;
        int oy_hi = iy / sh;
        if (oy_hi > OH - 1) oy_hi = OH - 1;
        int ox_lo = ix - kw + 1 + sw - 1;
        ox_lo = ox_lo < 0 ? 0 : ox_lo / sw;
        int ox_hi = ix / sw;
        if (ox_hi > OW - 1) ox_hi = OW - 1;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (MAX) v = *(const f32x4*)(x + i * 4);
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const int rows = min(oy * sh + kh, H) - oy * sh;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const long o = (((long)n * OH + oy) * OW + ox) * C + c4 * 4;
                const f32x4 g = *(const f32x4*)(dy + o);
                if (MAX) {
                    const f32x4 m = *(const f32x4*)(y + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += (v[e] == m[e]) ? g[e] : 0.f;      // every tie, not the first one
                } else {
                    const int cols = min(ox * sw + kw, W) - ox * sw;
                    acc += g / (float)(rows * cols);
                }
            }
        }
        *(f32x4*)(dx + i * 4) = acc;
    }
}

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// true when the geometry is one the kernels may run: every window starts inside the map, so none is empty and, clipped, no
// read leaves the tensor
bool geometry_ok(int N, int H, int W, int C, int OH, int OW, int kh, int kw, int sh, int sw) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return false;
    if (kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || OH <= 0 || OW <= 0) return false;
    if ((long)(OH - 1) * sh >= H || (long)(OW - 1) * sw >= W) return false;
    return true;
}

}  // namespace

#define POOL_BORDER_GEOMETRY(name)                                                                                             \
    DENET_CHECK_ARG(geometry_ok(N, H, W, C, OH, OW, kh, kw, sh, sw),                                                          \
                    name ": bad geometry (N %d, H %d, W %d, C %d, OH %d, OW %d, window %d x %d, stride %d x %d): C must be a " \
                         "multiple of 4 and every window must start inside the map",                                          \
                    N, H, W, C, OH, OW, kh, kw, sh, sw)

extern "C" int denet_maxpool_border_fwd(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, int kh, int kw,
                                        int sh, int sw, hipStream_t stream) {
    DENET_CHECK_ARG(x && y, "maxpool_border_fwd: null pointer");
    POOL_BORDER_GEOMETRY("maxpool_border_fwd");
    long total = (long)N * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool_border_fwd_kernel<true>, dim3(grid_for(total)), dim3(256), 0, stream, x, y, N, H, W, C, OH, OW, kh,
                       kw, sh, sw);
    DENET_CHECK_LAUNCH("maxpool_border_fwd");
    return DENET_OK;
}

extern "C" int denet_maxpool_border_bwd(const float* x, const float* y, const float* dy, float* dx, int N, int H, int W, int C,
                                        int OH, int OW, int kh, int kw, int sh, int sw, hipStream_t stream) {
    DENET_CHECK_ARG(x && y && dy && dx, "maxpool_border_bwd: null pointer");
    POOL_BORDER_GEOMETRY("maxpool_border_bwd");
    long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(pool_border_bwd_kernel<true>, dim3(grid_for(total)), dim3(256), 0, stream, x, y, dy, dx, N, H, W, C, OH,
                       OW, kh, kw, sh, sw);
    DENET_CHECK_LAUNCH("maxpool_border_bwd");
    return DENET_OK;
}

extern "C" int denet_avgpool_border_fwd(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, int kh, int kw,
                                        int sh, int sw, hipStream_t stream) {
    DENET_CHECK_ARG(x && y, "avgpool_border_fwd: null pointer");
    POOL_BORDER_GEOMETRY("avgpool_border_fwd");
    long total = (long)N * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool_border_fwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, stream, x, y, N, H, W, C, OH, OW, kh,
                       kw, sh, sw);
    DENET_CHECK_LAUNCH("avgpool_border_fwd");
    return DENET_OK;
}

extern "C" int denet_avgpool_border_bwd(const float* dy, float* dx, int N, int H, int W, int C, int OH, int OW, int kh, int kw,
                                        int sh, int sw, hipStream_t stream) {
    DENET_CHECK_ARG(dy && dx, "avgpool_border_bwd: null pointer");
    POOL_BORDER_GEOMETRY("avgpool_border_bwd");
    long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(pool_border_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, stream, (const float*)nullptr,
                       (const float*)nullptr, dy, dx, N, H, W, C, OH, OW, kh, kw, sh, sw);
    DENET_CHECK_LAUNCH("avgpool_border_bwd");
    return DENET_OK;
}
