// Global-norm gradient clipping and on-device gradient / weight norms (ModelCNN.gradient_clip, ModelCNN.track_grad_norm;
// model-train --gradient-clip NORM / --gradient-norms). Opt-in; the default step never reaches this file.
// Reference: denet/model/model_cnn.py:237-239 is theano.gradient.grad_clip(train_cost, -c, c), which clips the gradient ARRIVING AT
// THE COST (the constant 1): every gradient times min(1, c). No driver sets it; there is no behaviour to match, so the definition
// below is the contract. With g the trained part of the flat gradient buffer after the solver's grad_scale
// and before the decay term:
//     norm = sqrt(sum g^2)        coef = norm > c ? c / norm : 1.0f        the solver uses coef * g wherever it used g
// norm = NaN gives coef = 1, norm = inf gives coef = 0 (and 0 * inf = NaN): a non-finite gradient is not rescued.
//
// The reduction is bit-reproducible: its order is fixed by the chunk table alone, never by the grid, the device or the timing.
//   chunk table  int [n_chunks][3] = (offset, length, segment), built once by the host (ops.norm_chunks): the 64-aligned ranges of
//                the trained arrays cut into chunks of at most DENET_GRAD_NORM_CHUNK floats; no chunk straddles two arrays, one
//                segment = one array, the chunks of a segment are consecutive. Offsets and lengths are multiples of 4.
//   grad_norm_partial_kernel  one workgroup of 256 threads per chunk. float4 loads, (double)x * (double)x (exact: 48 bits) added
//                into four double lanes per thread in index order, (s0 + s1) + (s2 + s3), the 64 lanes of a wave by shuffles
//                (offsets 32 .. 1), the four waves through LDS in wave order, one plain store of the chunk's partial. The
//                workgroup of the first / last chunk of a segment also stores that chunk's index for the second launch.
//   grad_norm_finish_kernel   one workgroup. Per segment the sum of its chunks' partials in chunk order, the total = the sum of the
//                segment sums in segment order; seg_norm[s] = sqrt(sum_s) * scale, out = {norm, coef}, and the running record
//                stats[8] (doubles): steps | steps clipped | steps with a non-finite norm | sum of the finite norms | largest
//                finite norm | 3 unused. Nothing is read back by the host per step.
// No atomics and no hand-off between workgroups inside a launch. The padded entries of the device layout are zero in the gradient
// buffer by the kernels' design (igemm.hip and conv_rect.hip mask the unreal taps, padded channels read zeros, alignment gaps are
// never written), so reducing each array's 64-aligned extent adds nothing to the sums.
//
// solver_coef_kernel / adam_coef_kernel: elementwise.hip's solver_kernel / adam_kernel with `g * gscale` formed as there and THEN
// multiplied by *coef in a multiply of its own that the compiler may not contract into the decay FMA: coef = 1 leaves every bit
// of the plain step.
#include "common.h"
#include "../../include/denet_hip.h"
#include <math.h>

#define DENET_GRAD_NORM_CHUNK 8192          // floats per chunk: a compile-time constant, the same on every device and grid
#define DENET_GRAD_NORM_MAX_SEGMENTS 4096   // segment sums live in the LDS of the one finishing workgroup
#define GN_TILE 2048                        // partials staged per round of the finishing workgroup

namespace {

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ x, const int* __restrict__ table,
                                                                int n_chunks, int n_segments, double* __restrict__ partial,
                                                                int* __restrict__ seg_first, int* __restrict__ seg_last) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    const int off = table[3 * c], seg = table[3 * c + 2];
    int len = table[3 * c + 1];
    if (len > DENET_GRAD_NORM_CHUNK) len = DENET_GRAD_NORM_CHUNK;
    if (off < 0) len = 0;
    const int n4 = len >> 2;
    const f32x4* __restrict__ p = (const f32x4*)(x + off);
    // a thread adds its vectors in index order into four sums, one per vector lane. A full chunk (all but the last of an array)
    // issues its loads before the first sum waits for one; a short chunk takes the loop - the same additions in the same order
    constexpr int GN_LOADS = DENET_GRAD_NORM_CHUNK / 4 / 256;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (n4 == GN_LOADS * 256) {
        f32x4 v[GN_LOADS];
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) v[k] = p[k * 256 + (int)threadIdx.x];
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) {
            s0 += (double)v[k][0] * (double)v[k][0];
            s1 += (double)v[k][1] * (double)v[k][1];
            s2 += (double)v[k][2] * (double)v[k][2];
            s3 += (double)v[k][3] * (double)v[k][3];
        }
    } else {
        for (int i = (int)threadIdx.x; i < n4; i += 256) {
            const f32x4 t = p[i];
            s0 += (double)t[0] * (double)t[0];
            s1 += (double)t[1] * (double)t[1];
            s2 += (double)t[2] * (double)t[2];
            s3 += (double)t[3] * (double)t[3];
        }
    }
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
    if (seg < 0 || seg >= n_segments) return;
    if (c == 0 || table[3 * (c - 1) + 2] != seg) seg_first[seg] = c;
    if (c == n_chunks - 1 || table[3 * (c + 1) + 2] != seg) seg_last[seg] = c;
}

// a + v[0] + v[1] + ... strictly left to right; eight LDS reads are in flight while the additions wait for one another
__device__ __forceinline__ double add_in_order(double a, const double* v, int n) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = v[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) a += t[j];
    }
    for (; i < n; ++i) a += v[i];
    return a;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, const int* __restrict__ seg_first,
                                                               const int* __restrict__ seg_last, int n_chunks, int n_segments,
                                                               float scale, float clip, float* __restrict__ seg_norm,
                                                               float* __restrict__ out, double* __restrict__ stats) {
    __shared__ double tile[GN_TILE];
    __shared__ double seg_sum[DENET_GRAD_NORM_MAX_SEGMENTS];
    const int tid = threadIdx.x;
    for (int s = tid; s < n_segments; s += 256) seg_sum[s] = 0.0;
    for (int t0 = 0; t0 < n_chunks; t0 += GN_TILE) {
        const int t1 = min(t0 + GN_TILE, n_chunks);
        __syncthreads();
        for (int c = t0 + tid; c < t1; c += 256) tile[c - t0] = partial[c];
        __syncthreads();
        // a segment is owned by one thread: its partials are added in chunk order, round after round
        for (int s = tid; s < n_segments; s += 256) {
            const int lo = max(max(seg_first[s], 0), t0), hi = min(min(seg_last[s], n_chunks - 1), t1 - 1);
            seg_sum[s] = add_in_order(seg_sum[s], tile + (lo - t0), hi - lo + 1);
        }
    }
    __syncthreads();
    for (int s = tid; s < n_segments; s += 256) seg_norm[s] = (float)(sqrt(seg_sum[s]) * (double)scale);
    if (tid != 0) return;
    const double total = add_in_order(0.0, seg_sum, n_segments);
    const double norm = sqrt(total) * (double)scale;
    const float norm_f = (float)norm;
    const bool clipped = clip > 0.0f && norm > (double)clip;          // (false for NaN)
    const float coef = clipped ? (float)((double)clip / norm) : 1.0f;  // (inf: 0)
    out[0] = norm_f;
    out[1] = coef;
    if (stats) {
        stats[0] += 1.0;
        if (clipped) stats[1] += 1.0;
        if (isfinite(norm_f)) {
            stats[3] += (double)norm_f;
            if ((double)norm_f > stats[4]) stats[4] = (double)norm_f;
        } else {
            stats[2] += 1.0;
        }
    }
}

// a multiply rounded on its own: never half of an FMA
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// elementwise.hip solver_kernel with coef (a device scalar) applied to g * gscale
__global__ __launch_bounds__(256) void solver_coef_kernel(float* __restrict__ p, float* __restrict__ m,
                                                          const float* __restrict__ g, long n, long n_decay, float lr,
                                                          float mu, float rho, float decay, float gscale, int mode,
                                                          const float* __restrict__ coef) {
    const float cf = *coef;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float pv = p[i];
        float gv = mul_rounded(g[i] * gscale, cf);
        if (i < n_decay) gv += decay * pv;
        float mv;
        if (mode == 1) {
            mv = rho * m[i] + gv;
            p[i] = pv - lr * (gv + mu * mv);
        } else {
            mv = rho * m[i] + (1.0f - rho) * gv;
            p[i] = pv - lr * mv;
        }
        m[i] = mv;
    }
}

// elementwise.hip adam_kernel with coef applied to g * gscale
__global__ __launch_bounds__(256) void adam_coef_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, long n, long n_decay, float lr, float b1,
                                                        float b2, float c1, float c2, float decay, float gscale,
                                                        const float* __restrict__ coef) {
    const float cf = *coef;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float pv = p[i];
        float gv = mul_rounded(g[i] * gscale, cf);
        if (i < n_decay) gv += decay * pv;
        const float mv = b1 * m[i] + (1.0f - b1) * gv;
        const float vv = b2 * v[i] + (1.0f - b2) * (gv * gv);
        p[i] = pv - lr * (mv * c1) / (sqrtf(vv * c2) + 1e-8f);
        m[i] = mv;
        v[i] = vv;
    }
}

size_t partial_bytes(int n_chunks) { return (((size_t)n_chunks * sizeof(double)) + 63) / 64 * 64; }

}  // namespace

extern "C" int denet_grad_norm_chunk_len(void) { return DENET_GRAD_NORM_CHUNK; }

// host only: the table ops.norm_chunks built, against the rules the kernels rely on, and against the n floats of the buffer
extern "C" int denet_grad_norm_check_table(const int* table, int n_chunks, int n_segments, long n) {
    DENET_CHECK_ARG(table, "grad_norm_check_table: null pointer");
    DENET_CHECK_ARG(n_chunks > 0, "grad_norm_check_table: n_chunks = %d", n_chunks);
    DENET_CHECK_ARG(n_segments > 0 && n_segments <= DENET_GRAD_NORM_MAX_SEGMENTS && n_segments <= n_chunks,
                    "grad_norm_check_table: %d segments (1 .. %d, at most one per chunk)", n_segments, DENET_GRAD_NORM_MAX_SEGMENTS);
    long end = 0;
    int seg = -1;
    for (int c = 0; c < n_chunks; ++c) {
        const long off = table[3 * c], len = table[3 * c + 1];
        const int s = table[3 * c + 2];
        DENET_CHECK_ARG(len > 0 && len <= DENET_GRAD_NORM_CHUNK, "grad_norm_check_table: chunk %d is %ld floats long (1 .. %d)", c, len,
                        DENET_GRAD_NORM_CHUNK);
        DENET_CHECK_ARG(off % 4 == 0 && len % 4 == 0, "grad_norm_check_table: chunk %d is misaligned (offset %ld, length %ld: multiples of 4)",
                        c, off, len);
        DENET_CHECK_ARG(off >= end && off + len <= n, "grad_norm_check_table: chunk %d [%ld, %ld) overlaps its predecessor or leaves the %ld floats",
                        c, off, off + len, n);
        DENET_CHECK_ARG(s == seg || s == seg + 1, "grad_norm_check_table: chunk %d has segment %d behind segment %d", c, s, seg);
        end = off + len;
        seg = s;
    }
    DENET_CHECK_ARG(seg == n_segments - 1, "grad_norm_check_table: the chunks name %d segments, not %d", seg + 1, n_segments);
    return DENET_OK;
}

extern "C" size_t denet_grad_norm_workspace_bytes(int n_chunks, int n_segments) {
    if (n_chunks <= 0 || n_segments <= 0) return 0;
    return partial_bytes(n_chunks) + (size_t)2 * n_segments * sizeof(int);
}

// ops.kernel_symbol: kinds 50 / 51 = the two launches of the norm pass, 52 / 53 = the solvers that read coef
extern "C" int denet_grad_norm(const float* x, const int* table, int n_chunks, int n_segments, float scale, float clip, void* workspace,
                               float* seg_norm, float* out, double* stats, hipStream_t stream) {
    DENET_CHECK_ARG(x && table && workspace && seg_norm && out, "grad_norm: null pointer");
    DENET_CHECK_ARG(n_chunks > 0, "grad_norm: n_chunks = %d", n_chunks);
    DENET_CHECK_ARG(n_segments > 0 && n_segments <= DENET_GRAD_NORM_MAX_SEGMENTS && n_segments <= n_chunks,
                    "grad_norm: %d segments (1 .. %d, at most one per chunk)", n_segments, DENET_GRAD_NORM_MAX_SEGMENTS);
    DENET_CHECK_ARG(((uintptr_t)x & 15) == 0, "grad_norm: x is not 16-byte aligned");
    DENET_CHECK_ARG(scale >= 0.0f && isfinite(scale), "grad_norm: scale = %g", (double)scale);
    double* partial = (double*)workspace;
    int* seg_first = (int*)((char*)workspace + partial_bytes(n_chunks));
    int* seg_last = seg_first + n_segments;
    int prof = denet_prof_begin(50, 0, 0, 0, stream);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(n_chunks), dim3(256), 0, stream, x, table, n_chunks, n_segments, partial, seg_first,
                       seg_last);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(51, 0, 0, 0, stream);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, (const int*)seg_first,
                       (const int*)seg_last, n_chunks, n_segments, scale, clip, seg_norm, out, stats);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("grad_norm");
    return DENET_OK;
}

extern "C" int denet_solver_step_coef(float* params, float* moments, const float* grads, long n, long n_decay, float lr, float momentum,
                                      int iteration, float decay, float grad_scale, int mode, const float* coef, hipStream_t stream) {
    DENET_CHECK_ARG(params && moments && grads && coef && n > 0 && n_decay >= 0 && n_decay <= n, "solver_step_coef: bad args");
    DENET_CHECK_ARG(mode == 0 || mode == 1, "solver_step_coef: mode must be 0 (sgd) or 1 (nesterov/torch)");
    const float rho = iteration > 0 ? momentum : 0.0f;
    const int prof = denet_prof_begin(52, 0, 0, 0, stream);
    hipLaunchKernelGGL(solver_coef_kernel, dim3(grid_for(n)), dim3(256), 0, stream, params, moments, grads, n, n_decay, lr, momentum, rho,
                       decay, grad_scale, mode, coef);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("solver_step_coef");
    return DENET_OK;
}

extern "C" int denet_solver_adam_coef(float* params, float* m, float* v, const float* grads, long n, long n_decay, float lr, float beta1,
                                      float beta2, int iteration, float decay, float grad_scale, const float* coef, hipStream_t stream) {
    DENET_CHECK_ARG(params && m && v && grads && coef && n > 0 && n_decay >= 0 && n_decay <= n, "solver_adam_coef: bad args");
    DENET_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && iteration >= 0, "solver_adam_coef: bad betas");
    const float c1 = (float)(1.0 / (1.0 - pow((double)beta1, (double)iteration + 1.0)));
    const float c2 = (float)(1.0 / (1.0 - pow((double)beta2, (double)iteration + 1.0)));
    const int prof = denet_prof_begin(53, 0, 0, 0, stream);
    hipLaunchKernelGGL(adam_coef_kernel, dim3(grid_for(n)), dim3(256), 0, stream, params, m, v, grads, n, n_decay, lr, beta1, beta2, c1, c2,
                       decay, grad_scale, coef);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("solver_adam_coef");
    return DENET_OK;
}
