// The Winograd F(m x m, 3x3) transforms (m = 2 or 4), each in one text, and the internal functions the Winograd files call
// across translation units. The kernels that evaluate a batch norm on the fly (wino_prep_lds_kernel) must produce the bits of
// wino_input_kernel / wino_dout_kernel: they do because every kernel of winograd.hip calls the functions below.
//   Wino<MO>, wino_fma, WINO_DOT, ld4      the tables and one multiply-add of a transform
//   wino_input_col, wino_input_store       V = B^T d B        (column by column, then the rows, stored as V[xi][t][c])
//   wino_dout_col, wino_dout_store         dM = A d A^T       (adjoint of the output transform, stored as dM[xi][t][k])
//   wino_output_col, wino_output_at        Y = A^T m A        (column by column, then one value of the result)
//   wino_filter_transform                  U = G g G^T
//   wino_dfilter_col, wino_dfilter_rows    dw = G^T dU G      (adjoint of the filter transform)
// A transform takes the column its caller has loaded and the intermediate BY ARRAY REFERENCE and the caller keeps its own load
// loop: a single function with a callback for the patch value costs wino_input_kernel<4> a wave per SIMD and
// wino_prep_lds_kernel<4, false> two (EXPERIMENTS.md).
// (w2g_dfilter_kernel of wino2f.hip is NOT here: plain expressions instead of wino_fma, another rounding on purpose; the fused
// kernels wino4f.hip / wino4t.hip take Wino<4>::AT only, they accumulate component by component.)
#pragma once
#include "common.h"

// ---- internal functions called across files (the files that define them include this header) ----------------------------------
// igemm.hip: batched products out[b] = a[b] w[b]^T and the split-K filter-gradient products, with their tuning runs
int denet_gemm_batched_nt(const float* a, const float* w, float* out, int batch, int M, int Nc, int Kc, long stride_a,
                          long stride_w, long stride_out, hipStream_t stream);
int denet_gemm_batched_tune(const float* a, const float* w, float* out, int batch, int M, int Nc, int Kc, long stride_a,
                            long stride_w, long stride_out, hipStream_t stream);
int denet_wgrad_batched(const float* x, const float* dy, float* dw, float* workspace, size_t workspace_bytes, int batch,
                        int T, int Cc, int Kr, hipStream_t stream);
int denet_wgrad_batched_tune(const float* x, const float* dy, float* dw, float* workspace, size_t workspace_bytes, int batch,
                             int T, int Cc, int Kr, hipStream_t stream);
// wino4f.hip: F(4x4) products + output transform in one kernel
int denet_wino4f_block(int tile, long T, int C, int K);
int denet_wino4f_stats_rows(int tb, long T);
int denet_wino4f_run(int tb, const float* V, const float* U, const float* bias, const float* add, float* y, double* stats,
                     const float* bs_x, const float* bs_y, const float* bs_gamma, const float* bs_beta, const float* bs_mean,
                     const float* bs_invstd, int bs_relu, int N, int H, int W, int C, int K, int relu, hipStream_t stream);
// wino4g.hip: F(4x4) filter-gradient component products
int denet_wino4g_splits(int tile, long T, int C, int K);
size_t denet_wino4g_workspace_bytes(int splits, int C, int K);
int denet_wino4g_run(int splits, const float* dM, const float* V, float* dU, float* part, size_t part_bytes, long T, int C, int K,
                     hipStream_t stream);

__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }

// ---- transform matrices (Lavin & Gray, "Fast algorithms for convolutional neural networks") -----------------
// F(m x m, 3x3): TS = m + 2 points. Y = A^T [ (G g G^T) .* (B^T d B) ] A for the CORRELATION taps g.
template <int MO>
struct Wino;
template <>
struct Wino<2> {
    static constexpr int TS = 4;
    static constexpr float BT[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
    static constexpr float G[4][3] = {{1, 0, 0}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0, 0, 1}};
    static constexpr float AT[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
};
template <>
struct Wino<4> {
    static constexpr int TS = 6;
    static constexpr float BT[6][6] = {{4, 0, -5, 0, 1, 0},  {0, -4, -4, 1, 1, 0}, {0, 4, -4, -1, 1, 0},
                                       {0, -2, -1, 2, 1, 0}, {0, 2, -1, -2, 1, 0}, {0, 4, 0, -5, 0, 1}};
    static constexpr float G[6][3] = {{0.25f, 0, 0},
                                      {-1.f / 6, -1.f / 6, -1.f / 6},
                                      {-1.f / 6, 1.f / 6, -1.f / 6},
                                      {1.f / 24, 1.f / 12, 1.f / 6},
                                      {1.f / 24, -1.f / 12, 1.f / 6},
                                      {0, 0, 1}};
    static constexpr float AT[4][6] = {{1, 1, 1, 1, 1, 0}, {0, 1, -1, 2, -2, 0}, {0, 1, 1, 4, 4, 0}, {0, 1, -1, 8, -8, 1}};
};

// one multiply-add of a transform, written as an explicit fused operation: left to the compiler, an expression like
// 4*d0 - 5*d2 + d4 is contracted as fma(-5, d2, 4*d0) in one kernel and as fma(4, d0, -5*d2) in another (both legal, different
// roundings)
__device__ __forceinline__ float wino_fma(float c, float v, float acc) { return __builtin_fmaf(c, v, acc); }
__device__ __forceinline__ f32x4 wino_fma(float c, f32x4 v, f32x4 acc) {
    f32x4 r;
    r[0] = __builtin_fmaf(c, v[0], acc[0]);
    r[1] = __builtin_fmaf(c, v[1], acc[1]);
    r[2] = __builtin_fmaf(c, v[2], acc[2]);
    r[3] = __builtin_fmaf(c, v[3], acc[3]);
    return r;
}

// acc = sum_l coef[l] * v[l] with the compile-time coefficients folded (0 dropped): first product rounded, then one fused
// multiply-add per further term, in index order
#define WINO_DOT(acc, NL, COEF, VAL)                       \
    {                                                      \
        bool first_ = true;                                \
        _Pragma("unroll") for (int l_ = 0; l_ < (NL); ++l_) { \
            const float c_ = (COEF);                       \
            if (c_ != 0.f) {                               \
                if (first_) acc = c_ * (VAL);              \
                else acc = wino_fma(c_, (VAL), acc);       \
                first_ = false;                            \
            }                                              \
        }                                                  \
    }

// ---- input transform V = B^T d B ---------------------------------------------------------------------------------------------
// column j of B^T d from column j of the TS x TS patch: tt[i][j] = sum_l BT[i][l] d[l]
template <int MO>
__device__ __forceinline__ void wino_input_col(const f32x4 (&d)[Wino<MO>::TS], f32x4 (&tt)[Wino<MO>::TS][Wino<MO>::TS], int j) {
    using WT = Wino<MO>;
#pragma unroll
    for (int i = 0; i < WT::TS; ++i) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        WINO_DOT(acc, WT::TS, WT::BT[i][l_], d[l_]);
        tt[i][j] = acc;
    }
}
// V[xi][t][c .. c + 3] = ((B^T d) B)[xi], xi = TS * i + j; V: [TS * TS][T][C]
template <int MO>
__device__ __forceinline__ void wino_input_store(const f32x4 (&tt)[Wino<MO>::TS][Wino<MO>::TS], float* V, long T, long t,
                                                 int C, int c) {
    using WT = Wino<MO>;
    constexpr int TS = WT::TS;
#pragma unroll
    for (int i = 0; i < TS; ++i)
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            WINO_DOT(acc, TS, WT::BT[j][l_], tt[i][l_]);
            *(f32x4*)(V + ((long)(TS * i + j) * T + t) * C + c) = acc;
        }
}

// ---- adjoint of the output transform dM = A d A^T over a tile's own MO x MO pixels --------------------------------------------
// column j of A d: a[i][j] = sum_l AT[l][i] d[l]
template <int MO>
__device__ __forceinline__ void wino_dout_col(const f32x4 (&d)[MO], f32x4 (&a)[Wino<MO>::TS][MO], int j) {
    using WT = Wino<MO>;
#pragma unroll
    for (int i = 0; i < WT::TS; ++i) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        WINO_DOT(acc, MO, WT::AT[l_][i], d[l_]);
        a[i][j] = acc;
    }
}
// dM[xi][t][k .. k + 3] = ((A d) A^T)[xi]; dM: [TS * TS][T][K]
template <int MO>
__device__ __forceinline__ void wino_dout_store(const f32x4 (&a)[Wino<MO>::TS][MO], float* dM, long T, long t, int K,
                                                int k) {
    using WT = Wino<MO>;
    constexpr int TS = WT::TS;
#pragma unroll
    for (int i = 0; i < TS; ++i)
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            WINO_DOT(acc, MO, WT::AT[l_][j], a[i][l_]);
            *(f32x4*)(dM + ((long)(TS * i + j) * T + t) * K + k) = acc;
        }
}

// ---- output transform Y = A^T m A ---------------------------------------------------------------------------------------------
// column j of A^T m: s[i][j] = sum_l AT[i][l] m[l]
template <int MO>
__device__ __forceinline__ void wino_output_col(const f32x4 (&m)[Wino<MO>::TS], f32x4 (&s)[MO][Wino<MO>::TS], int j) {
    using WT = Wino<MO>;
#pragma unroll
    for (int i = 0; i < MO; ++i) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        WINO_DOT(acc, WT::TS, WT::AT[i][l_], m[l_]);
        s[i][j] = acc;
    }
}
// Y[i][j] from row i of A^T m (the caller's epilogue takes the values one at a time)
template <int MO>
__device__ __forceinline__ f32x4 wino_output_at(const f32x4 (&si)[Wino<MO>::TS], int j) {
    using WT = Wino<MO>;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    WINO_DOT(acc, WT::TS, WT::AT[j][l_], si[l_]);
    return acc;
}

// ---- filter transform U = G g G^T ---------------------------------------------------------------------------------------------
template <int MO>
__device__ __forceinline__ void wino_filter_transform(const float (&g)[3][3], float (&u)[Wino<MO>::TS][Wino<MO>::TS]) {
    using WT = Wino<MO>;
    constexpr int TS = WT::TS;
    float a[TS][3];
#pragma unroll
    for (int i = 0; i < TS; ++i)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            float acc = 0.f;
            WINO_DOT(acc, 3, WT::G[i][l_], g[l_][s]);
            a[i][s] = acc;
        }
#pragma unroll
    for (int i = 0; i < TS; ++i)
#pragma unroll
        for (int j = 0; j < TS; ++j) {
            float acc = 0.f;
            WINO_DOT(acc, 3, WT::G[j][l_], a[i][l_]);
            u[i][j] = acc;
        }
}

// ---- adjoint of the filter transform dw = G^T dU G ----------------------------------------------------------------------------
// column j of G^T u: r[i][j] = sum_l G[l][i] u[l]
template <int MO>
__device__ __forceinline__ void wino_dfilter_col(const float (&u)[Wino<MO>::TS], float (&r)[3][Wino<MO>::TS], int j) {
    using WT = Wino<MO>;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = 0.f;
        WINO_DOT(acc, WT::TS, WT::G[l_][i], u[l_]);
        r[i][j] = acc;
    }
}
template <int MO>
__device__ __forceinline__ void wino_dfilter_rows(const float (&r)[3][Wino<MO>::TS], float (&dw)[3][3]) {
    using WT = Wino<MO>;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = 0.f;
            WINO_DOT(acc, WT::TS, WT::G[l_][j], r[i][l_]);
            dw[i][j] = acc;
        }
}
