// An exponential moving average of the weights, kept on the device (ModelCNN.ema_decay; model-train --ema DECAY). Opt-in; the
// default step never reaches this file. The reference has no such mode: the definition below is the contract (DESIGN.md
// section 18). Once per parameter update, right behind the solver, for every float of the flat parameter buffer P into its shadow
// E, and for every float of the batch-norm statistics S into ES:
//     e <- fmaf(om, p - e, e)        om = float32(1 - d_t), formed by the host in double and passed by value
// The subtraction is rounded on its own, the multiply and the addition in one fused rounding. The difference form is deliberate:
// where p == e the entry keeps its value, so frozen arrays, padded channels and alignment gaps never drift.
//   ema_update_kernel  grid-stride, 256 threads, at most EMA_MAX_BLOCKS workgroups. The body is read and written as 16-byte
//                      vectors from the first 16-byte boundary of e on; up to 3 floats in front of it and up to 3 behind it are
//                      scalars, so any n >= 1 and any (4-byte) alignment work. When e and p sit differently inside their 16 bytes no
//                      vector can be aligned on both: the whole range is then scalar.
//   swap_kernel        a[i] <-> b[i] with the same split; exact (bits are moved, nothing is computed).
// No atomics; plain vector stores. One pass moves 3 x 4 x n bytes (update: two reads, one write) or 4 x 4 x n (swap).
#include "common.h"
#include "../../include/denet_hip.h"

#define EMA_MAX_BLOCKS 2048   // 256 CUs x 8 workgroups of 256 threads: one resident set, the rest by the grid stride

namespace {

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > EMA_MAX_BLOCKS) b = EMA_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// a subtraction rounded on its own: never half of an FMA
__device__ __forceinline__ float sub_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ float ema_one(float e, float p, float om) { return fmaf(om, sub_rounded(p, e), e); }

// the floats [0, n) as head [0, head) | body [head, head + 4 * n4) | tail [head + 4 * n4, n): index of the i-th scalar one
__device__ __forceinline__ long scalar_index(long i, long head, long n4) { return i < head ? i : i + 4 * n4; }

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, long head, long n4,
                                                         long n, float om) {
    const long first = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    f32x4* __restrict__ e4 = (f32x4*)(e + head);
    const f32x4* __restrict__ p4 = (const f32x4*)(p + head);
    for (long i = first; i < n4; i += stride) {
        f32x4 ev = e4[i];
        const f32x4 pv = p4[i];
        ev[0] = ema_one(ev[0], pv[0], om);
        ev[1] = ema_one(ev[1], pv[1], om);
        ev[2] = ema_one(ev[2], pv[2], om);
        ev[3] = ema_one(ev[3], pv[3], om);
        e4[i] = ev;
    }
    const long rest = n - 4 * n4;
    for (long i = first; i < rest; i += stride) {
        const long k = scalar_index(i, head, n4);
        e[k] = ema_one(e[k], p[k], om);
    }
}

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long head, long n4, long n) {
    const long first = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    f32x4* __restrict__ a4 = (f32x4*)(a + head);
    f32x4* __restrict__ b4 = (f32x4*)(b + head);
    for (long i = first; i < n4; i += stride) {
        const f32x4 av = a4[i], bv = b4[i];
        a4[i] = bv;
        b4[i] = av;
    }
    const long rest = n - 4 * n4;
    for (long i = first; i < rest; i += stride) {
        const long k = scalar_index(i, head, n4);
        const float av = a[k], bv = b[k];
        a[k] = bv;
        b[k] = av;
    }
}

// head: floats in front of a's first 16-byte boundary (0 .. 3, at most n); n4: whole vectors behind it. Both 0 when b sits
// differently inside its 16 bytes (the range is then scalar)
void split(const float* a, const float* b, long n, long* head, long* n4) {
    *head = 0;
    *n4 = 0;
    if (((uintptr_t)a & 15) != ((uintptr_t)b & 15)) return;
    long h = (long)(((16 - ((uintptr_t)a & 15)) & 15) / 4);
    if (h > n) h = n;
    *head = h;
    *n4 = (n - h) / 4;
}

bool disjoint(const float* a, const float* b, long n) { return a + n <= b || b + n <= a; }

}  // namespace

// ops.kernel_symbol: kind 54 = the average's update, 55 = the exchange of two buffers
extern "C" int denet_ema_update(float* e, const float* p, long n, float om, hipStream_t stream) {
    DENET_CHECK_ARG(e && p, "ema_update: null pointer");
    DENET_CHECK_ARG(n >= 1, "ema_update: n = %ld", n);
    DENET_CHECK_ARG((((uintptr_t)e | (uintptr_t)p) & 3) == 0, "ema_update: a pointer is not 4-byte aligned");
    DENET_CHECK_ARG(disjoint(e, p, n), "ema_update: e and p overlap");
    DENET_CHECK_ARG(om >= 0.0f && om <= 1.0f, "ema_update: om = %g (1 - decay, inside [0, 1])", (double)om);
    long head, n4;
    split(e, p, n, &head, &n4);
    const long rest = n - 4 * n4;
    const int prof = denet_prof_begin(54, 0, 0, 0, stream);
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n4 > rest ? n4 : rest)), dim3(256), 0, stream, e, p, head, n4, n, om);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("ema_update");
    return DENET_OK;
}

extern "C" int denet_swap(float* a, float* b, long n, hipStream_t stream) {
    DENET_CHECK_ARG(a && b, "swap: null pointer");
    DENET_CHECK_ARG(n >= 1, "swap: n = %ld", n);
    DENET_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "swap: a pointer is not 4-byte aligned");
    DENET_CHECK_ARG(disjoint(a, b, n), "swap: a and b overlap");
    long head, n4;
    split(a, b, n, &head, &n4);
    const long rest = n - 4 * n4;
    const int prof = denet_prof_begin(55, 0, 0, 0, stream);
    hipLaunchKernelGGL(swap_kernel, dim3(grid_for(n4 > rest ? n4 : rest)), dim3(256), 0, stream, a, b, head, n4, n);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("swap");
    return DENET_OK;
}
