// OPT-IN training variant, never the headline path (ops.TRAIN_PRECISION = "bf16", model-train --precision bf16; the numerics
// contract is in DESIGN.md, "bf16 training"): the backward passes of a square convolution with both operands rounded to bf16
// (nearest-even, where they are staged) and multiplied on the bf16 matrix cores of gfx950, accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16. The forward pass is conv_bf16.hip's kernel on the raw filter.
//
// Data gradient (stride 1):  dx = conv_bf16_kernel(dy, w_t, padding R-1-pad) (+ add), with the rotated, transposed filter copy
//                            w_t[c][R-1-r][S-1-s][k] = bf16(w[k][r][s][c]) made from the fp32 filter by filter_to_bf16_dgrad_kernel
//                            (one rounding of w).
// Filter gradient:           dw[K][R*S*C] = dy^T[K][pix] * im2col(x)[pix][R*S*C], stride 1 or 2, any padding the forward takes.
//   Tiling:    256 threads (4 wave64) per BM x 128 tile of dw, BM = 128 / 64 / 32 filter rows by K alone (conv_rect.hip's table:
//              nothing is measured). The reduction index is the pixel, the STRIDED axis of both NHWC operands: a chunk of 32 pixels
//              is transposed while it is converted, on the LDS store - a lane loads 4 channels of two neighbouring pixels and
//              writes 4 dwords (pixel pair) into a [channel][pixel] bf16 image with rows of 80 bytes (32 bf16 + 16 bytes of
//              padding, conv_bf16.hip), from which the MFMA fragments are 16-byte reads. The 16-byte slots of a row are swizzled
//              with the row so that the dword stores of a half wave hit 32 banks. Two LDS buffers, one barrier per chunk.
//   Zeros:     padding taps, pixels beyond N*OH*OW, filter rows beyond K and columns beyond R*S*C are staged as +0.
//   Slices:    the chunks are cut into slices by wgrad_slices (geometry only, at most 128); a slice writes its partial dw to the
//              workspace and conv_bf16_wgrad_reduce_kernel adds them in slice order. No atomics: bit-identical run to run.
#include "bf16_mma.h"
#include "../../include/denet_hip.h"

namespace {

constexpr int BK = 32;                                // pixels per chunk
constexpr int BN = 128;                               // columns of R*S*C per tile

struct WgradParams {
    const float* x;                // [N][H][W][C] fp32
    const float* dy;               // [N][OH][OW][K] fp32
    float* out;                    // dw [K][R][S][C], or the slices
    int N, H, W, C, K, R, S, stride, pad, OH, OW;
    int M;                         // N*OH*OW
    int RSC;
    int ksteps;                    // chunks of 32 pixels
    int steps_per_slice;
    long slice_stride;             // K*R*S*C
    int tiles_n;                   // tiles along R*S*C
    FastDiv div_img, div_row, div_c, div_s;      // OH*OW, OW, C, S
    unsigned x_bytes, dy_bytes;
};

template <int BM, int BNT>
__global__ __launch_bounds__(256) void conv_bf16_wgrad_kernel(const WgradParams p) {
    static_assert(BNT == BN && (BM == 128 || BM == 64 || BM == 32), "tile table");
    constexpr int WK = BM >= 64 ? 2 : 1, WR = 4 / WK;        // waves along the filters / the columns
    constexpr int TK = BM / (32 * WK), TR = BN / (32 * WR);  // 32 x 32 MFMA tiles of a wave
    constexpr int QA = BM / 4;                              // channel quads of a dy pixel in the tile
    constexpr int PD = (16 * QA + 255) / 256;               // dy loader passes: 16 pixel pairs x QA quads
    constexpr int PX = 2;                                   // x loader passes: 16 pixel pairs x 32 quads
    constexpr int SZX = BN * ROWB, SZD = BM * ROWB;

    __shared__ __attribute__((aligned(16))) char smem[2 * (SZX + SZD)];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WK, wk = wave % WK;
    const int li = lane & 31, lh = lane >> 5;

    const uint32_t tile_id = xcd_remap(blockIdx.x, gridDim.x);
    const int k0 = (int)(tile_id / p.tiles_n) * BM, n0 = (int)(tile_id % p.tiles_n) * BN;
    const int z = blockIdx.y;
    const int st0 = z * p.steps_per_slice;
    const int st1 = min(st0 + p.steps_per_slice, p.ksteps);

    // ---------------- loaders ----------------
    // item = tid + 256 * pass -> (pixel pair pp of the chunk's 16, channel quad q of the tile's Q): the low 3 bits of an item are the low
    // bits of q (8 lanes read 128 contiguous bytes of one pixel), the next 2 the low bits of pp, the rest (q >> 3, pp >> 2). With the
    // slot swizzle of store_chunk the 32 dword stores of a half wave then fall into 32 different LDS banks
    auto item_q = [](int it, int Q) { return (it & 7) + 8 * ((it >> 5) % (Q / 8)); };
    auto item_pp = [](int it, int Q) { return ((it >> 3) & 3) + 4 * ((it >> 5) / (Q / 8)); };
    // x: Q = 32 quads of the tile's 128 columns. C % 32 = 0 and n0 % 128 = 0: a quad lies inside one tap, which is the lane's for the
    // whole reduction (the quad of an item does not depend on the pass: 256 % 32 = 0 and 8 % (Q / 8) = 0)
    const int cq = item_q(tid, 32);
    int x_pp[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) x_pp[i] = item_pp(tid + 256 * i, 32);
    const int col = n0 + 4 * cq;
    const bool col_ok = col < p.RSC;
    int x_dr = 0, x_ds = 0, x_c = 0;
    if (col_ok) {
        const uint32_t tap = p.div_c.div((uint32_t)col);
        x_c = col - (int)tap * p.C;
        const uint32_t r = p.div_s.div(tap);
        x_dr = (int)r - p.pad;
        x_ds = (int)(tap - r * p.S) - p.pad;
    }
    // dy: Q = QA quads of the tile's BM filters
    int d_pp[PD], d_kq[PD];
    bool d_ok[PD];
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        const int it = tid + 256 * i;
        d_pp[i] = item_pp(it, QA);
        d_kq[i] = item_q(it, QA);
        d_ok[i] = d_pp[i] < 16 && k0 + 4 * d_kq[i] < p.K;
    }
    const __amdgpu_buffer_rsrc_t r_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_d = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, p.dy_bytes, 0x00020000);

    f32x4 rx[PX][2], rd[PD][2];

    auto load_chunk = [&](int st) {
        const int mb = st * BK;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int m = mb + 2 * x_pp[i] + e;
                int off = OOBV;
                if (col_ok && m < p.M) {
                    const uint32_t n = p.div_img.div((uint32_t)m);
                    const uint32_t rem = (uint32_t)m - n * (uint32_t)(p.OH * p.OW);
                    const uint32_t oy = p.div_row.div(rem);
                    const uint32_t ox = rem - oy * (uint32_t)p.OW;
                    const int iy = (int)oy * p.stride + x_dr, ix = (int)ox * p.stride + x_ds;
                    if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
                        off = (int)((unsigned)((((int)n * p.H + iy) * p.W + ix) * p.C + x_c) * 4u);
                }
                rx[i][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_x, off, 0, 0));
            }
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int m = mb + 2 * d_pp[i] + e;
                const int off = (d_ok[i] && m < p.M) ? (int)(((unsigned)m * (unsigned)p.K + (unsigned)(k0 + 4 * d_kq[i])) * 4u) : OOBV;
                rd[i][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_d, off, 0, 0));
            }
        }
    };

    // the transpose: [channel][pixel] images, a pixel pair is one dword. The four 16-byte slots of a row (8 pixels each) are
    // swizzled with bits 3..4 of the row (read side: fragment addresses below)
    auto store_chunk = [&](int buf) {
        char* dx = smem + buf * (SZX + SZD);
        char* dd = dx + SZX;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int o = (((x_pp[i] >> 2) ^ ((cq >> 1) & 3)) * 4 + (x_pp[i] & 3)) * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) *(unsigned*)(dx + (4 * cq + t) * ROWB + o) = pack2(rx[i][0][t], rx[i][1][t]);
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            if (d_pp[i] < 16) {
                const int o = (((d_pp[i] >> 2) ^ ((d_kq[i] >> 1) & 3)) * 4 + (d_pp[i] & 3)) * 4;
#pragma unroll
                for (int t = 0; t < 4; ++t) *(unsigned*)(dd + (4 * d_kq[i] + t) * ROWB + o) = pack2(rd[i][0][t], rd[i][1][t]);
            }
        }
    };

    f32x16 acc[TR][TK];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int j = 0; j < TK; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment addresses: lane = (row l & 31 of a 32-row tile, group l >> 5 of 8 consecutive pixels)
    const int xrow = wr * (TR * 32) + li;
    const int drow = wk * (TK * 32) + li;
    // (slot 2 * ks + lh of the row, swizzled with bits 3..4 of the row: xrow + 32 * i and drow + 32 * j keep those bits)
    const int fx = xrow * ROWB, sx = (xrow >> 3) & 3;
    const int fd = drow * ROWB, sd = (drow >> 3) & 3;

    load_chunk(st0);
    store_chunk(0);
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
        const bool more = st + 1 < st1;
        if (more) load_chunk(st + 1);
        const char* cx = smem + ((st - st0) & 1) * (SZX + SZD);
        const char* cd = cx + SZX;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 xv[TR], dv[TK];
#pragma unroll
            for (int i = 0; i < TR; ++i) xv[i] = *(const bf16x8*)(cx + fx + i * 32 * ROWB + (((2 * ks + lh) ^ sx) * 16));
#pragma unroll
            for (int j = 0; j < TK; ++j) dv[j] = *(const bf16x8*)(cd + fd + j * 32 * ROWB + (((2 * ks + lh) ^ sd) * 16));
            // the columns of R*S*C as the first operand: a lane's accumulator then holds 4-element runs along C (16-byte stores)
#pragma unroll
            for (int i = 0; i < TR; ++i)
#pragma unroll
                for (int j = 0; j < TK; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xv[i], dv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_chunk((st - st0 + 1) & 1);
        __syncthreads();
    }

    // ---------------- epilogue: the lane owns filter k = .. + li, columns 8g + 4h .. +3 in registers 4g .. 4g+3 ----------------
    float* out = p.out + (long)z * p.slice_stride;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int k = k0 + drow + 32 * j;
        if (k >= p.K) continue;
        const long row = (long)k * p.RSC;
#pragma unroll
        for (int i = 0; i < TR; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = n0 + wr * (TR * 32) + 32 * i + 8 * g + 4 * lh;
                if (c >= p.RSC) continue;
                const f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                *(f32x4*)(out + row + c) = v;
            }
        }
    }
}

// dw = the slices added in slice order (one float4 column per thread)
__global__ __launch_bounds__(256) void conv_bf16_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, long n4,
                                                                     int slices) {
    const long col = (long)blockIdx.x * 256 + threadIdx.x;
    if (col >= n4) return;
    const f32x4* w4 = (const f32x4*)ws;
    f32x4 s = w4[col];
    for (int zz = 1; zz < slices; ++zz) s += w4[col + (long)zz * n4];
    ((f32x4*)out)[col] = s;
}

// wt[c][R-1-r][S-1-s][k] = bf16(w[k][r][s][c]), round to nearest-even: one 32 x 32 (k, c) tile of one tap per workgroup, read
// along c and written along k
__global__ __launch_bounds__(256) void filter_to_bf16_dgrad_kernel(const float* __restrict__ w, unsigned short* __restrict__ wt, int K,
                                                                   int R, int S, int C) {
    __shared__ float tile[32][33];
    const int tiles_c = C / 32;
    const int k0 = (int)(blockIdx.x / tiles_c) * 32, c0 = (int)(blockIdx.x % tiles_c) * 32;
    const int tap = blockIdx.y, RS = R * S;
    const int r = tap / S, s = tap - r * S;
    const int tap_t = (R - 1 - r) * S + (S - 1 - s);
    const int tid = threadIdx.x;
    const int cc = tid & 31, kk0 = tid >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = kk0 + 8 * i;
        tile[kk][cc] = w[((long)(k0 + kk) * RS + tap) * C + c0 + cc];
    }
    __syncthreads();
    const int kq = tid & 15, c2 = tid >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = c2 + 16 * i;
        *(unsigned*)(wt + ((long)(c0 + c) * RS + tap_t) * K + k0 + 2 * kq) = pack2(tile[2 * kq][c], tile[2 * kq + 1][c]);
    }
}

int wgrad_bm(int K) { return K >= 96 ? 128 : (K >= 64 ? 64 : 32); }

// slices of the filter gradient's pixel reduction, from the geometry alone (conv_rect.hip's rule): enough workgroups for two per
// CU, at least 4 chunks each, at most 128; every slice holds at least one chunk
int wgrad_slices(int N, int C, int K, int R, int S, int OH, int OW) {
    const long tiles = (long)ceil_div(K, wgrad_bm(K)) * ceil_div((long)R * S * C, BN);
    const int ksteps = ceil_div((long)N * OH * OW, BK);
    long sp = 512 / tiles;
    if (sp > ksteps / 4) sp = ksteps / 4;
    if (sp > 128) sp = 128;
    if (sp < 1) sp = 1;
    const int per = ceil_div(ksteps, sp);
    return ceil_div(ksteps, per);
}

template <int BM>
int launch_wgrad(WgradParams& p, int slices, hipStream_t stream) {
    p.tiles_n = ceil_div(p.RSC, BN);
    const int tiles_m = ceil_div(p.K, BM);
    const int prof = denet_prof_begin(22, BM, BN, 0, stream);          // ops.kernel_symbol: conv_bf16_wgrad_kernel<BM, BN>
    hipLaunchKernelGGL((conv_bf16_wgrad_kernel<BM, BN>), dim3((unsigned)(tiles_m * p.tiles_n), (unsigned)slices, 1), dim3(256), 0,
                       stream, p);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("conv_wgrad_bf16");
    return DENET_OK;
}

}  // namespace

extern "C" int denet_filter_to_bf16_dgrad(const float* w, void* wt16, int K, int R, int S, int C, hipStream_t stream) {
    DENET_CHECK_ARG(K > 0 && R > 0 && S > 0 && C > 0, "filter_to_bf16_dgrad: non-positive dimension");
    DENET_CHECK_ARG(C % 32 == 0, "filter_to_bf16_dgrad: physical C (%d) must be a multiple of 32", C);
    DENET_CHECK_ARG(K % 32 == 0, "filter_to_bf16_dgrad: physical K (%d) must be a multiple of 32", K);
    DENET_CHECK_ARG((long)K * R * S * C * 4 < 0xF0000000L && (long)R * S < 65536 && (long)(K / 32) * (C / 32) < (1L << 31),
                    "filter_to_bf16_dgrad: filter too large");
    DENET_CHECK_ARG(w && wt16, "filter_to_bf16_dgrad: null pointer");
    const int prof = denet_prof_begin(24, 0, 0, 0, stream);            // ops.kernel_symbol: filter_to_bf16_dgrad_kernel
    hipLaunchKernelGGL(filter_to_bf16_dgrad_kernel, dim3((unsigned)((K / 32) * (C / 32)), (unsigned)(R * S), 1), dim3(256), 0, stream, w,
                       (unsigned short*)wt16, K, R, S, C);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("filter_to_bf16_dgrad");
    return DENET_OK;
}

extern "C" int denet_conv_dgrad_bf16(const float* dy, const void* wt16, const float* add, float* dx, int N, int H, int W, int C, int K,
                                     int R, int S, int S_real, int stride, int pad, int OH, int OW, hipStream_t stream) {
    int rc = check_conv_bf16("conv_dgrad_bf16", N, H, W, C, K, R, S, S_real, stride, pad, OH, OW);
    if (rc) return rc;
    DENET_CHECK_ARG(stride == 1, "conv_dgrad_bf16: stride 1 only (got %d): a strided data gradient runs the fp32 kernels", stride);
    DENET_CHECK_ARG(pad <= R - 1, "conv_dgrad_bf16: pad (%d) must not exceed R - 1 (%d)", pad, R - 1);
    DENET_CHECK_ARG(OH == H + 2 * pad - R + 1 && OW == W + 2 * pad - S + 1, "conv_dgrad_bf16: a cut output (OH %d, OW %d) is not taken",
                    OH, OW);
    DENET_CHECK_ARG(dy && wt16 && dx, "conv_dgrad_bf16: null tensor");
    // the forward kernel on dy over the rotated, transposed filter: C and K change places, the padding becomes R - 1 - pad
    return denet_conv_fwd_bf16(dy, wt16, nullptr, add, dx, 0, N, OH, OW, K, C, R, S, S, 1, R - 1 - pad, H, W, stream);
}

extern "C" int denet_conv_wgrad_bf16_slices(int N, int C, int K, int R, int S, int OH, int OW) {
    if (N <= 0 || C <= 0 || K <= 0 || R <= 0 || S <= 0 || OH <= 0 || OW <= 0) return 0;
    return wgrad_slices(N, C, K, R, S, OH, OW);
}

extern "C" size_t denet_conv_wgrad_bf16_workspace_bytes(int N, int C, int K, int R, int S, int OH, int OW) {
    const int sp = denet_conv_wgrad_bf16_slices(N, C, K, R, S, OH, OW);
    return sp > 1 ? (size_t)sp * K * R * S * C * sizeof(float) : 0;
}

extern "C" int denet_conv_wgrad_bf16(const float* x, const float* dy, float* dw, float* workspace, size_t workspace_bytes, int N,
                                     int H, int W, int C, int K, int R, int S, int S_real, int stride, int pad, int OH, int OW,
                                     hipStream_t stream) {
    int rc = check_conv_bf16("conv_wgrad_bf16", N, H, W, C, K, R, S, S_real, stride, pad, OH, OW);
    if (rc) return rc;
    DENET_CHECK_ARG(x && dy && dw, "conv_wgrad_bf16: null tensor");
    WgradParams p = {};
    p.x = x; p.dy = dy;
    p.N = N; p.H = H; p.W = W; p.C = C; p.K = K; p.R = R; p.S = S; p.stride = stride; p.pad = pad; p.OH = OH; p.OW = OW;
    p.M = N * OH * OW;
    p.RSC = R * S * C;
    p.ksteps = ceil_div(p.M, BK);
    const int slices = wgrad_slices(N, C, K, R, S, OH, OW);
    p.steps_per_slice = ceil_div(p.ksteps, slices);
    p.slice_stride = (long)K * p.RSC;
    if (slices > 1) {
        DENET_CHECK_ARG(workspace && workspace_bytes >= (size_t)slices * p.slice_stride * sizeof(float),
                        "conv_wgrad_bf16: workspace of %zu bytes, %zu needed (denet_conv_wgrad_bf16_workspace_bytes)", workspace_bytes,
                        (size_t)slices * p.slice_stride * sizeof(float));
        p.out = workspace;
    } else {
        p.out = dw;
    }
    p.div_img.init((uint32_t)(OH * OW));
    p.div_row.init((uint32_t)OW);
    p.div_c.init((uint32_t)C);
    p.div_s.init((uint32_t)S);
    p.x_bytes = (unsigned)((long)N * H * W * C * 4);
    p.dy_bytes = (unsigned)((long)N * OH * OW * K * 4);
    const int bm = wgrad_bm(K);
    if (bm == 128) rc = launch_wgrad<128>(p, slices, stream);
    else if (bm == 64) rc = launch_wgrad<64>(p, slices, stream);
    else rc = launch_wgrad<32>(p, slices, stream);
    if (rc) return rc;
    if (slices > 1) {
        const long n4 = p.slice_stride / 4;
        const int prof = denet_prof_begin(23, 0, 0, 0, stream);        // ops.kernel_symbol: conv_bf16_wgrad_reduce_kernel
        hipLaunchKernelGGL(conv_bf16_wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, workspace, dw, n4,
                           slices);
        denet_prof_end(prof, stream);
        DENET_CHECK_LAUNCH("conv_wgrad_bf16_reduce");
    }
    return DENET_OK;
}
