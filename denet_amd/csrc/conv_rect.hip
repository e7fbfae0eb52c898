// Convolution with a per-axis geometry for gfx950 (MI355X): the `C.X[k, kh, kw, sh, sw]` / `DC.X[...]` tokens of the model
// description (reference: denet/layer/convolution.py:55-83,99-112, deconvolution.py:54-65; gradients: tensor.grad,
// model_cnn.py:318). Filter R x S, stride (sh, sw), padding (ph, pw), output OH x OW given by the caller. The square kernels
// of igemm.hip / winograd.hip take ONE stride and ONE pad; this file is the direct kernel of everything else and shares no
// code path with them. The same text with the taps of a filter (dh, dw) apart is the dilated convolution of the `C.D[k, size,
// stride, d]` / `C.DX[k, kh, kw, sh, sw, dh, dw]` tokens and the dilated residual blocks (conv_dil_kernel; this build's own
// contract, DESIGN.md section 19: the reference has no dilation). The same text on a channel window of x, w and y is the grouped
// convolution of the `C.G[k, size, stride, g]` / `C.GX[k, kh, kw, sh, sw, g]` tokens and the grouped residual blocks
// (conv_grp_kernel, grid.z = the window; this build's own contract, DESIGN.md section 20: the reference has no groups).
//
// Layout (HBM):   activations NHWC fp32, filters KRSC fp32 correlation taps (as igemm.hip).
// Arithmetic:     v_mfma_f32_32x32x2_f32, exact fp32 FMA chain, accumulators in registers.
// Tiling:         256 threads (4 wave64) per BM x BN output tile, the reduction walked in chunks of 32 through two LDS
//                 buffers (the next chunk travels global -> VGPR while the current one is multiplied; one barrier per chunk).
//                 LDS layouts as igemm.hip: K-inner [rows][32+4] (ds_read_b128), K-outer [32][cols+4] (ds_read_b32).
//                   fwd:   A = im2col(x) K-inner,           B = w K-inner
//                   dgrad: A = im2col(dy) K-inner,          B = w (per tap) K-outer; grid.y = the sh*sw classes of input pixels
//                   wgrad: A = dy K-outer (rows = k),       B = im2col(x) K-outer; grid.y = slices of the pixel reduction,
//                          added in slice order by a second kernel (deterministic, no atomics)
//                 Inside an 8-wide k block lane-half h consumes k = 4h..4h+3 of both operands (a fixed permutation of the sum).
// One tile table, chosen by the channel counts alone: no measured choice, the same kernel in every process.
#include "common.h"
#include "../../include/denet_hip.h"

namespace {

constexpr int BK = 32;
constexpr int LDK = BK + 4;

enum { PASS_FWD = 0, PASS_DGRAD = 1, PASS_WGRAD = 2 };

struct RectParams {
    const float* a;      // fwd: x   dgrad: dy  wgrad: dy
    const float* b;      // fwd: w   dgrad: w   wgrad: x
    float* out;          // fwd: y   dgrad: dx  wgrad: dw or the slices
    const float* bias;   // fwd, [K] or null
    const float* add;    // fwd / dgrad: tensor of the output's shape added in the epilogue, or null
    int relu;            // fwd: max(., 0) after bias and add
    int N, H, W, C;
    int OH, OW, K;
    int R, S, S_real;
    int sh, sw, shs, sws, ph, pw;   // strides, their log2, padding
    int M, NC;           // GEMM rows / columns
    int ksteps;          // fwd / wgrad: 32-wide reduction chunks
    int steps_per_split;
    long split_stride;   // wgrad: elements between slices
    int tiles_m, tiles_n;
    int npix;            // N*OH*OW
    int Hc, Wc;          // dgrad: ceil(H/sh), ceil(W/sw): rows of one class per image (classes with fewer are masked)
    FastDiv div_img;     // fwd / wgrad: OH*OW   dgrad: Hc*Wc
    FastDiv div_row;     // fwd / wgrad: OW      dgrad: Wc
    unsigned a_bytes, b_bytes;   // extents of a / b: lanes outside read 0 through the buffer descriptor
    // dilation: tap (r, s) reads row r*dh, column s*dw of its window (read by the DIL instantiations only). 16 bits each: the pair
    // fills the 4 bytes the struct ended in unused, so the kernel arguments of conv_rect_kernel lie where they lay without it
    unsigned short dh, dw;
};
static_assert(sizeof(RectParams) == 192, "RectParams: the kernel-argument layout of conv_rect_kernel is part of its device code");

// A grouped pass: the dense problem `r` of ONE channel window (r.C = Cw input and r.K = Kw output channels: the reduction extents
// and the filter's inner dimension) inside tensors whose pixels hold ldc / ldk channels. Window i = blockIdx.z starts i * Cw
// channels into x / dx, i * Kw into y / dy / bias / add and i * Kw * R * S * Cw elements into w / dw and each of its slices. A struct
// of its own: RectParams is the kernel-argument layout of the kernels that came before
struct GrpParams {
    RectParams r;
    int ldc, ldk;        // channels of a whole pixel of x / dx, of y / dy
    int w_win;           // Kw * R * S * Cw: the filter rows of one window
};

// what the one text reads of either struct (the plain passes: the pixel strides are the extents, no window). The body calls these
// at every use: read once into locals, the plain kernels came out with other scalar registers than they had (EXPERIMENTS.md)
__device__ __forceinline__ const RectParams& rect_of(const RectParams& p) { return p; }
__device__ __forceinline__ const RectParams& rect_of(const GrpParams& q) { return q.r; }
__device__ __forceinline__ int ldc_of(const RectParams& p) { return p.C; }
__device__ __forceinline__ int ldc_of(const GrpParams& q) { return q.ldc; }
__device__ __forceinline__ int ldk_of(const RectParams& p) { return p.K; }
__device__ __forceinline__ int ldk_of(const GrpParams& q) { return q.ldk; }
__device__ __forceinline__ int w_win_of(const RectParams&) { return 0; }
__device__ __forceinline__ int w_win_of(const GrpParams& q) { return q.w_win; }

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
constexpr int OOB_OFFSET = (int)0xF0000000u;   // beyond every extent check_rect admits
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, int elem_off, bool ok) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, ok ? elem_off * 4 : OOB_OFFSET, 0, 0);
    return __builtin_bit_cast(f32x4, v);
}

// The one text of all three passes. DIL = false: the taps of a filter are neighbours (conv_rect_kernel); DIL = true: they lie
// (dh, dw) apart (conv_dil_kernel). A dilated axis has stride 1 (check_rect), so the data gradient's classes are those of the
// strides alone and its tap walk steps by the dilation. Every dilated term sits behind DIL. GRP = true (P = GrpParams): the passes
// of channel window blockIdx.z (conv_grp_kernel): p.C / p.K stay the extents of the reductions, the pixel strides become the whole
// tensors' ldc / ldk and every tensor starts at its window. Every grouped term sits behind GRP.
template <bool DIL, bool GRP, int PASS, int BM, int BN, int WM, int WN, class P>
__device__ __forceinline__ void conv_rect_body(const P q) {
    const RectParams& p = rect_of(q);
    // the window's first element of a, b, the output (and `add`), and its first bias
    const long win = GRP ? (long)blockIdx.z : 0;
    const long win_x = win * p.C, win_y = win * p.K, win_w = win * w_win_of(q);
    const long win_a = PASS == PASS_FWD ? win_x : win_y;
    const long win_b = PASS == PASS_FWD || PASS == PASS_DGRAD ? win_w : win_x;
    const long win_o = PASS == PASS_FWD ? win_y : (PASS == PASS_DGRAD ? win_x : win_w);
    const int dh = DIL ? p.dh : 1, dw = DIL ? p.dw : 1;
    constexpr bool A_KIN = (PASS != PASS_WGRAD);
    constexpr bool B_KIN = (PASS == PASS_FWD);
    constexpr int TM = BM / (32 * WM);
    constexpr int TN = BN / (32 * WN);
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(TM >= 1 && TN >= 1, "tile too small");
    constexpr int LDA = BM + 4, LDB = BN + 4;         // K-outer rows
    constexpr int SZA = A_KIN ? BM * LDK : BK * LDA;
    constexpr int SZB = B_KIN ? BN * LDK : BK * LDB;
    constexpr int PA = BM / 32, PB = BN / 32;          // loader passes, one float4 per thread each
    constexpr int LPR_A = BM / 4, RPP_A = 256 / LPR_A;
    constexpr int LPR_B = BN / 4, RPP_B = 256 / LPR_B;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;              // [2][SZA]
    float* sB = smem + 2 * SZA;    // [2][SZB]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    const uint32_t tile_id = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_n = tile_id % p.tiles_n;
    const int tile_m = tile_id / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // dgrad: grid.y = class (py, px) of input pixels iy = ya*sh + py, ix = xa*sw + px. Such a pixel receives the taps
    // r = r0 + sh*r', s = s0 + sw*s' only, from the output pixel (ya + by - r', xa + bx - s'): a dense problem per class
    int dg_py = 0, dg_px = 0, dg_r0 = 0, dg_s0 = 0, dg_rc = 0, dg_sc = 0, dg_by = 0, dg_bx = 0;
    int step_begin = 0, step_end = p.ksteps;
    if (PASS == PASS_DGRAD) {
        dg_py = blockIdx.y >> p.sws;
        dg_px = blockIdx.y & (p.sw - 1);
        dg_r0 = (dg_py + p.ph) & (p.sh - 1);
        dg_s0 = (dg_px + p.pw) & (p.sw - 1);
        dg_by = (dg_py + p.ph) >> p.shs;
        dg_bx = (dg_px + p.pw) >> p.sws;
        dg_rc = (p.R > dg_r0) ? ((p.R - dg_r0 + p.sh - 1) >> p.shs) : 0;
        dg_sc = (p.S_real > dg_s0) ? ((p.S_real - dg_s0 + p.sw - 1) >> p.sws) : 0;
        step_end = dg_rc * dg_sc * (p.K / BK);
    } else if (PASS == PASS_WGRAD) {
        step_begin = blockIdx.y * p.steps_per_split;
        step_end = min(p.ksteps, step_begin + p.steps_per_split);
    }
    const int nsteps = step_end - step_begin;

    // ---------------- per-thread loader state ----------------
    const int q8 = tid & 7, row8 = tid >> 3;             // K-inner: float4 column of the chunk, row of a 32-row pass
    const int qa = tid % LPR_A, kra = tid / LPR_A;       // K-outer A
    const int qb = tid % LPR_B, krb = tid / LPR_B;       // K-outer B
    // fewer than 32 channels (the network input): a chunk spans 32 / C taps of one filter row
    const int qs = (PASS == PASS_FWD && p.C < 32) ? (4 * q8) / p.C : 0;
    const int qc = (PASS == PASS_FWD && p.C < 32) ? (4 * q8) % p.C : 4 * q8;

    int a_off[PA], a_y[PA], a_x[PA];
    int b_off[PB];
    bool b_ok[PB];
    int wg_r = 0, wg_s = 0, wg_c = 0;
    bool wg_colok = false;
    const int rsc = p.R * p.S * p.C;

    if (PASS == PASS_FWD) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int m = m0 + row8 + 32 * i;
            // a row that is none: every tap lies above the image. Dilated, -(R + 1) + r * dh could come back inside it: the row sits
            // at -(ke_h + 1), ke_h = (R - 1) * dh + 1, and its last tap at -2
            a_y[i] = DIL ? -((p.R - 1) * dh + 2) : -(p.R + 1); a_x[i] = 0; a_off[i] = 0;
            if (m < p.M) {
                const uint32_t n = p.div_img.div(m);
                const uint32_t rem = m - n * (p.OH * p.OW);
                const uint32_t oy = p.div_row.div(rem);
                const uint32_t ox = rem - oy * p.OW;
                a_y[i] = (int)oy * p.sh - p.ph;
                a_x[i] = (int)ox * p.sw - p.pw + qs;
                a_off[i] = (((int)n * p.H + a_y[i]) * p.W + a_x[i]) * ldc_of(q) + qc;
            }
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int n = n0 + row8 + 32 * i;
            b_ok[i] = n < p.K;
            b_off[i] = n * rsc + 4 * q8;
        }
    } else if (PASS == PASS_DGRAD) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int m = m0 + row8 + 32 * i;
            a_y[i] = -1; a_x[i] = 0; a_off[i] = 0;              // a row that is none: every tap comes from above the output
            if (m < p.M) {
                const uint32_t n = p.div_img.div(m);
                const uint32_t rem = m - n * (p.Hc * p.Wc);
                const uint32_t ya = p.div_row.div(rem);
                const uint32_t xa = rem - ya * p.Wc;
                if ((int)ya * p.sh + dg_py < p.H && (int)xa * p.sw + dg_px < p.W) {
                    a_y[i] = (int)ya + dg_by;
                    a_x[i] = (int)xa + dg_bx;
                    a_off[i] = (int)n * (p.OH * p.OW * ldk_of(q)) + 4 * q8;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int col = n0 + 4 * qb;
            b_ok[i] = col < p.C;
            b_off[i] = (krb + RPP_B * i) * rsc + col;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            a_off[i] = (kra + RPP_A * i) * ldk_of(q) + m0 + 4 * qa;
            a_y[i] = 0; a_x[i] = 0;
        }
        const int jg = n0 + 4 * qb;
        const int rs = jg / p.C;
        wg_c = jg - rs * p.C;
        wg_r = rs / p.S;
        wg_s = rs - wg_r * p.S;
        wg_colok = (jg < p.NC) && (wg_s < p.S_real);
#pragma unroll
        for (int i = 0; i < PB; ++i) { b_ok[i] = wg_colok; b_off[i] = 0; }
    }
    const bool wg_rowok = (PASS == PASS_WGRAD) ? (m0 + 4 * qa < p.K) : true;

    // (a window's descriptor starts at the window and ends where the tensor ends)
    const __amdgpu_buffer_rsrc_t r_a = __builtin_amdgcn_make_buffer_rsrc((void*)(GRP ? p.a + win_a : p.a), 0,
                                                                         GRP ? p.a_bytes - (unsigned)win_a * 4 : p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_b = __builtin_amdgcn_make_buffer_rsrc((void*)(GRP ? p.b + win_b : p.b), 0,
                                                                         GRP ? p.b_bytes - (unsigned)win_b * 4 : p.b_bytes, 0x00020000);

    // wave-uniform reduction cursor: fwd (r, s, c0) over the filter, dgrad (r', s', k0) over the taps of the class; wgrad: chunk
    int cur_r = 0, cur_s = 0, cur_c = 0, cur_step = step_begin;
    f32x4 ra[PA], rb[PB];

    auto load_chunk = [&]() {
        if (PASS == PASS_FWD) {
            const int tap_y = DIL ? cur_r * dh : cur_r, tap_x = DIL ? cur_s * dw : cur_s;
            const int u_off = (tap_y * p.W + tap_x) * ldc_of(q) + cur_c;
            const bool tap_ok = cur_s + qs < p.S_real;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const bool ok = tap_ok && ((unsigned)(a_y[i] + tap_y) < (unsigned)p.H) && ((unsigned)(a_x[i] + tap_x) < (unsigned)p.W);
                ra[i] = buf_load4(r_a, a_off[i] + u_off, ok);
            }
#pragma unroll
            for (int i = 0; i < PB; ++i) rb[i] = buf_load4(r_b, b_off[i] + cur_step * BK, b_ok[i]);
            if (p.C >= 32) {
                cur_c += BK;
                if (cur_c >= p.C) {
                    cur_c = 0;
                    if (++cur_s >= p.S) { cur_s = 0; ++cur_r; }
                }
            } else {
                cur_s += 32 / p.C;
                if (cur_s >= p.S) { cur_s = 0; ++cur_r; }
            }
        } else if (PASS == PASS_DGRAD) {
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int oy = a_y[i] - (DIL ? cur_r * dh : cur_r), ox = a_x[i] - (DIL ? cur_s * dw : cur_s);
                const bool ok = ((unsigned)oy < (unsigned)p.OH) && ((unsigned)ox < (unsigned)p.OW);
                ra[i] = buf_load4(r_a, a_off[i] + (oy * p.OW + ox) * ldk_of(q) + cur_c, ok);
            }
            const int u_offb = cur_c * rsc + ((dg_r0 + (cur_r << p.shs)) * p.S + dg_s0 + (cur_s << p.sws)) * p.C;
#pragma unroll
            for (int i = 0; i < PB; ++i) rb[i] = buf_load4(r_b, b_off[i] + u_offb, b_ok[i]);
            cur_c += BK;
            if (cur_c >= p.K) {
                cur_c = 0;
                if (++cur_s >= dg_sc) { cur_s = 0; ++cur_r; }
            }
        } else {
            const int pix0 = cur_step * BK;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const bool ok = wg_rowok && (pix0 + kra + RPP_A * i < p.npix);
                ra[i] = buf_load4(r_a, pix0 * ldk_of(q) + a_off[i], ok);
            }
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int pix = pix0 + krb + RPP_B * i;
                const uint32_t n = p.div_img.div(pix);
                const uint32_t rem = pix - n * (p.OH * p.OW);
                const uint32_t oy = p.div_row.div(rem);
                const uint32_t ox = rem - oy * p.OW;
                const int iy = (int)oy * p.sh - p.ph + (DIL ? wg_r * dh : wg_r);
                const int ix = (int)ox * p.sw - p.pw + (DIL ? wg_s * dw : wg_s);
                const bool ok = wg_colok && (pix < p.npix) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
                rb[i] = buf_load4(r_b, (((int)n * p.H + iy) * p.W + ix) * ldc_of(q) + wg_c, ok);
            }
        }
        ++cur_step;
    };

    auto store_chunk = [&](int buf) {
        float* da = sA + buf * SZA;
        float* db = sB + buf * SZB;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            if (A_KIN) *(f32x4*)(da + (row8 + 32 * i) * LDK + 4 * q8) = ra[i];
            else *(f32x4*)(da + (kra + RPP_A * i) * LDA + 4 * qa) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if (B_KIN) *(f32x4*)(db + (row8 + 32 * i) * LDK + 4 * q8) = rb[i];
            else *(f32x4*)(db + (krb + RPP_B * i) * LDB + 4 * qb) = rb[i];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int arow = wm * (TM * 32) + li;     // this lane's row of A / row (column of the product) of B inside the tile
    const int brow = wn * (TN * 32) + li;

    if (nsteps > 0) {
        load_chunk();
        store_chunk(0);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const bool more = st + 1 < nsteps;
        if (more) load_chunk();
        const float* ca = sA + (st & 1) * SZA;
        const float* cb = sB + (st & 1) * SZB;
#pragma unroll
        for (int kb = 0; kb < BK / 8; ++kb) {
            f32x4 av[TM], bv[TN];
            const int k0 = 8 * kb + 4 * lh;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (A_KIN) {
                    av[i] = *(const f32x4*)(ca + (arow + 32 * i) * LDK + k0);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) av[i][t] = ca[(k0 + t) * LDA + arow + 32 * i];
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (B_KIN) {
                    bv[j] = *(const f32x4*)(cb + (brow + 32 * j) * LDK + k0);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) bv[j][t] = cb[(k0 + t) * LDB + brow + 32 * j];
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[j][t], av[i][t], acc[i][j], 0, 0, 0);
        }
        if (more) store_chunk((st + 1) & 1);
        __syncthreads();
    }

    float* const out = GRP ? p.out + win_o : p.out;
    const float* const bias = GRP ? (p.bias ? p.bias + win_y : nullptr) : p.bias;
    const float* const addp = GRP ? (p.add ? p.add + win_o : nullptr) : p.add;
    // ---------------- epilogue: the lane owns row m = ..+li, columns 8g + 4h .. +3 in registers 4g .. 4g+3 ----------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + arow + 32 * i;
        long row = -1;
        if (PASS == PASS_FWD) {
            if (m < p.M) row = (long)m * ldk_of(q);
        } else if (PASS == PASS_DGRAD) {
            if (m < p.M) {
                const uint32_t n = p.div_img.div(m);
                const uint32_t rem = m - n * (p.Hc * p.Wc);
                const uint32_t ya = p.div_row.div(rem);
                const uint32_t xa = rem - ya * p.Wc;
                const int iy = (int)ya * p.sh + dg_py, ix = (int)xa * p.sw + dg_px;
                if (iy < p.H && ix < p.W) row = (((long)n * p.H + iy) * p.W + ix) * ldc_of(q);
            }
        } else {
            if (m < p.K) row = (long)blockIdx.y * p.split_stride + (long)m * p.NC;
        }
        if (row < 0) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * (TN * 32) + 32 * j + 8 * g + 4 * lh;
                if (n >= p.NC) continue;
                f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                if (PASS == PASS_FWD && bias) v += *(const f32x4*)(bias + n);
                if (PASS != PASS_WGRAD && addp) v += *(const f32x4*)(addp + row + n);
                if (PASS == PASS_FWD && p.relu) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
                }
                *(f32x4*)(out + row + n) = v;
            }
        }
    }
}

template <int PASS, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_rect_kernel(const RectParams p) {
    conv_rect_body<false, false, PASS, BM, BN, WM, WN>(p);
}

// the same passes with the taps (dh, dw) apart: the `C.D[...]` / `C.DX[...]` layers and the dilated residual blocks
template <int PASS, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_dil_kernel(const RectParams p) {
    conv_rect_body<true, false, PASS, BM, BN, WM, WN>(p);
}

// the same passes on channel window blockIdx.z of x, w and y: the `C.G[...]` / `C.GX[...]` layers and the grouped residual blocks
template <int PASS, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_grp_kernel(const GrpParams q) {
    conv_rect_body<false, true, PASS, BM, BN, WM, WN>(q);
}

// Groups of fewer than 32 channels (Cg = Kg in {1, 2, 4, 8, 16}) run as windows of 32 channels (slabs) on a filter that is dense
// inside a slab: output channel k of slab k / 32 reads the Cg channels of its own group and zeros for the rest of the slab.
//   wd[k][r][s][j] = w[k][r][s][j % Cg] if j / Cg == (k % 32) / Cg, else 0            (j < 32; one float4 of wd per thread)
__global__ __launch_bounds__(256) void grp_expand_kernel(const float* __restrict__ w, float* __restrict__ wd, long n4, int RS,
                                                         int cgs) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n4) return;
    const int Cg = 1 << cgs;
    const long krs = t >> 3;                     // (k, r, s): 8 float4 to its 32 slab channels
    const int j0 = (int)(t & 7) * 4;
    const int blk = (int)((krs / RS) & 31) >> cgs;   // the block of the slab this output channel reads
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        v[e] = (j >> cgs) == blk ? w[krs * Cg + (j & (Cg - 1))] : 0.f;
    }
    ((f32x4*)wd)[t] = v;
}

// ... and the gradient of the compact filter is the diagonal blocks of the slab filter's:
//   dw[k][r][s][c] = dwd[k][r][s][((k % 32) / Cg) * Cg + c]                             (one element of dw per thread)
__global__ __launch_bounds__(256) void grp_compact_kernel(const float* __restrict__ dwd, float* __restrict__ dw, long n, int RS,
                                                          int cgs) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int Cg = 1 << cgs;
    const long krs = t >> cgs;
    const int c = (int)(t & (Cg - 1));
    const int blk = (int)((krs / RS) & 31) >> cgs;
    dw[t] = dwd[krs * 32 + blk * Cg + c];
}

// dw = the slices added in slice order (one float4 column per thread)
__global__ __launch_bounds__(256) void conv_rect_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, long n4,
                                                               int splits) {
    const long col = (long)blockIdx.x * 256 + threadIdx.x;
    if (col >= n4) return;
    const f32x4* w4 = (const f32x4*)ws;
    f32x4 s = w4[col];
    for (int z = 1; z < splits; ++z) s += w4[col + (long)z * n4];
    ((f32x4*)out)[col] = s;
}

int check_rect(const char* who, int N, int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh,
               int dw, int OH, int OW) {
    DENET_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0, "%s: non-positive dimension", who);
    DENET_CHECK_ARG(S_real > 0 && S_real <= S, "%s: S_real (%d) out of range", who, S_real);
    DENET_CHECK_ARG(ilog2_exact(sh) >= 0, "%s: row stride sh must be a power of two (got %d)", who, sh);
    DENET_CHECK_ARG(ilog2_exact(sw) >= 0, "%s: column stride sw must be a power of two (got %d)", who, sw);
    DENET_CHECK_ARG(ph >= 0 && pw >= 0, "%s: negative padding (ph %d, pw %d)", who, ph, pw);
    DENET_CHECK_ARG(dh >= 1, "%s: row dilation dh must be at least 1 (got %d)", who, dh);
    DENET_CHECK_ARG(dw >= 1, "%s: column dilation dw must be at least 1 (got %d)", who, dw);
    DENET_CHECK_ARG(dh <= 0xFFFF && dw <= 0xFFFF, "%s: dilation (dh %d, dw %d) beyond 65535", who, dh, dw);
    // a dilated axis has stride 1: the data gradient's classes of input pixels are those of the strides alone
    DENET_CHECK_ARG(dh == 1 || sh == 1, "%s: row stride sh must be 1 on a dilated axis (sh %d, dh %d)", who, sh, dh);
    DENET_CHECK_ARG(dw == 1 || sw == 1, "%s: column stride sw must be 1 on a dilated axis (sw %d, dw %d)", who, sw, dw);
    DENET_CHECK_ARG(K % 32 == 0, "%s: physical K (%d) must be a multiple of 32", who, K);
    if (C >= 32) {
        DENET_CHECK_ARG(C % 32 == 0, "%s: physical C (%d) must be a multiple of 32", who, C);
        DENET_CHECK_ARG(S_real == S, "%s: S_real (%d) != S (%d) with 32 channels or more", who, S_real, S);
    } else {
        DENET_CHECK_ARG(C == 4 || C == 8 || C == 16, "%s: small C must be 4, 8 or 16 (got %d)", who, C);
        DENET_CHECK_ARG((S * C) % 32 == 0, "%s: S*C (%d) must be a multiple of 32 for small C", who, S * C);
    }
    // (the small-C path packs several taps of a filter row into one chunk: neighbours only)
    DENET_CHECK_ARG((dh == 1 && dw == 1) || C % 32 == 0, "%s: a dilated filter needs physical C (%d) to be a multiple of 32", who, C);
    const long keh = (long)(R - 1) * dh + 1, kew = (long)(S_real - 1) * dw + 1;      // effective extents
    DENET_CHECK_ARG(H + 2 * ph >= keh && OH > 0 && (H + 2 * ph - keh) / sh + 1 >= OH, "%s: OH=%d inconsistent", who, OH);
    DENET_CHECK_ARG(W + 2 * pw >= kew && OW > 0 && (W + 2 * pw - kew) / sw + 1 >= OW, "%s: OW=%d inconsistent", who, OW);
    // 32-bit buffer descriptors (byte offsets); 0xF0000000 marks a lane that reads nothing. The padded class grid of the
    // data gradient (ceil(H/sh)*sh x ceil(W/sw)*sw) is indexed with 32-bit integers as well
    DENET_CHECK_ARG((long)N * (H + sh) * (W + sw) * C * 4 < 0xF0000000L && (long)N * OH * OW * K * 4 < 0xF0000000L &&
                        (long)K * R * S * C * 4 < 0xF0000000L,
                    "%s: tensor exceeds the 32-bit buffer extent (3.75 GiB)", who);
    return DENET_OK;
}

RectParams make_params(int N, int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw,
                       int OH, int OW) {
    RectParams p = {};
    p.N = N; p.H = H; p.W = W; p.C = C; p.OH = OH; p.OW = OW; p.K = K; p.R = R; p.S = S; p.S_real = S_real;
    p.sh = sh; p.sw = sw; p.shs = ilog2_exact(sh); p.sws = ilog2_exact(sw); p.ph = ph; p.pw = pw;
    p.dh = (unsigned short)dh; p.dw = (unsigned short)dw;
    p.npix = N * OH * OW;
    return p;
}

// the whole tensors around a window problem: channels of a pixel of x / dx and y / dy, the number of windows (plain passes: 1)
struct GrpDims {
    int ldc, ldk, windows;
};

// what a grouped entry point asks beyond check_rect (which sees the whole tensors): windows of whole 128-byte lines, as many on
// the input as on the output side
int check_grp(const char* who, int C, int K, int Cw, int Kw, int S, int S_real) {
    DENET_CHECK_ARG(Cw > 0 && Cw % 32 == 0, "%s: window Cw (%d) must be a positive multiple of 32", who, Cw);
    DENET_CHECK_ARG(Kw > 0 && Kw % 32 == 0, "%s: window Kw (%d) must be a positive multiple of 32", who, Kw);
    DENET_CHECK_ARG(C % Cw == 0, "%s: window Cw (%d) does not divide C (%d)", who, Cw, C);
    DENET_CHECK_ARG(K % Kw == 0, "%s: window Kw (%d) does not divide K (%d)", who, Kw, K);
    DENET_CHECK_ARG(C / Cw == K / Kw, "%s: %d input windows (C %d / Cw %d) against %d output windows (K %d / Kw %d)", who, C / Cw, C, Cw,
                    K / Kw, K, Kw);
    DENET_CHECK_ARG(S_real == S, "%s: S_real (%d) != S (%d): a grouped filter has no padded taps", who, S_real, S);
    return DENET_OK;
}

template <bool DIL, bool GRP, int PASS, int BM, int BN, int WM, int WN>
int launch_rect(RectParams& p, unsigned grid_y, const GrpDims& gd, hipStream_t stream) {
    constexpr bool A_KIN = (PASS != PASS_WGRAD);
    constexpr bool B_KIN = (PASS == PASS_FWD);
    constexpr int SZA = A_KIN ? BM * LDK : BK * (BM + 4);
    constexpr int SZB = B_KIN ? BN * LDK : BK * (BN + 4);
    constexpr size_t lds = 2 * (size_t)(SZA + SZB) * sizeof(float);
    static_assert(!(DIL && GRP), "a grouped layer is not dilated");
    void (*const kernel)(const RectParams) = DIL ? conv_dil_kernel<PASS, BM, BN, WM, WN> : conv_rect_kernel<PASS, BM, BN, WM, WN>;
    void (*const grp_kernel)(const GrpParams) = conv_grp_kernel<PASS, BM, BN, WM, WN>;
    static bool attr_set[DENET_MAX_DEVICES] = {};
    const hipError_t e = denet_allow_dynamic_lds(GRP ? (const void*)grp_kernel : (const void*)kernel, (int)lds, attr_set);
    if (e != hipSuccess) {
        denet_set_error("conv_rect: hipFuncSetAttribute(%zu B LDS): %s", lds, hipGetErrorString(e));
        return -(int)e;
    }
    p.tiles_m = ceil_div(p.M, BM);
    p.tiles_n = ceil_div(p.NC, BN);
    // ops.kernel_symbol: 20 = conv_rect_kernel<PASS, BM, BN>, 25 = conv_dil_kernel<PASS, BM, BN>, 26 = conv_grp_kernel<PASS, BM, BN>
    const int prof = denet_prof_begin(GRP ? 26 : (DIL ? 25 : 20), PASS, BM, BN, stream);
    if (GRP) {
        const GrpParams q = {p, gd.ldc, gd.ldk, p.K * p.R * p.S * p.C};
        hipLaunchKernelGGL(grp_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n), grid_y, (unsigned)gd.windows), dim3(256), lds, stream, q);
    } else {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(p.tiles_m * p.tiles_n), grid_y, 1), dim3(256), lds, stream, p);
    }
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH(GRP ? "conv_grp" : (DIL ? "conv_dil" : "conv_rect"));
    return DENET_OK;
}

// rows of 128 pixels against 128 / 64 / 32 output columns (fwd, dgrad)
template <bool DIL, bool GRP, int PASS>
int launch_by_cols(RectParams& p, unsigned grid_y, const GrpDims& gd, hipStream_t stream) {
    if (p.NC >= 96) return launch_rect<DIL, GRP, PASS, 128, 128, 2, 2>(p, grid_y, gd, stream);
    if (p.NC >= 64) return launch_rect<DIL, GRP, PASS, 128, 64, 2, 2>(p, grid_y, gd, stream);
    return launch_rect<DIL, GRP, PASS, 128, 32, 4, 1>(p, grid_y, gd, stream);
}

// slices of the filter gradient's pixel reduction: enough workgroups for two per CU, at least 4 chunks each, at most 128
int wgrad_splits(int N, int C, int K, int R, int S, int OH, int OW) {
    const int bm = K >= 96 ? 128 : (K >= 64 ? 64 : 32);
    const long tiles = (long)ceil_div(K, bm) * ceil_div((long)R * S * C, 128);
    const int ksteps = ceil_div((long)N * OH * OW, BK);
    long sp = 512 / tiles;
    if (sp > ksteps / 4) sp = ksteps / 4;
    if (sp > 128) sp = 128;
    if (sp < 1) sp = 1;
    const int per = ceil_div(ksteps, sp);
    return ceil_div(ksteps, per);
}

// The host side of the three passes, one text for the three kernels: `who` names the entry point in the messages. C and K are the
// channels of the whole tensors, Cw and Kw those of one window (the plain passes: Cw = C, Kw = K, one window); the filter is
// [K][R][S][Cw]
template <bool DIL, bool GRP = false>
int rect_fwd(const char* who, const float* x, const float* w, const float* bias, const float* add, float* y, int relu, int N, int H,
             int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw, int OH, int OW,
             int Cw, int Kw, hipStream_t stream) {
    int rc = check_rect(who, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    if (rc) return rc;
    if (GRP && (rc = check_grp(who, C, K, Cw, Kw, S, S_real))) return rc;
    DENET_CHECK_ARG(x && w && y, "%s: null tensor", who);
    RectParams p = make_params(N, H, W, Cw, Kw, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    p.a = x; p.b = w; p.out = y; p.bias = bias; p.add = add; p.relu = relu;
    p.M = p.npix; p.NC = Kw;
    p.ksteps = R * S * Cw / BK;
    p.div_img.init((uint32_t)(OH * OW));
    p.div_row.init((uint32_t)OW);
    p.a_bytes = (unsigned)((long)N * H * W * C * 4);
    p.b_bytes = (unsigned)((long)K * R * S * Cw * 4);
    return launch_by_cols<DIL, GRP, PASS_FWD>(p, 1, GrpDims{C, K, C / Cw}, stream);
}

template <bool DIL, bool GRP = false>
int rect_dgrad(const char* who, const float* dy, const float* w, const float* add, float* dx, int N, int H, int W, int C, int K, int R,
               int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw, int OH, int OW, int Cw, int Kw,
               hipStream_t stream) {
    int rc = check_rect(who, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    if (rc) return rc;
    if (GRP && (rc = check_grp(who, C, K, Cw, Kw, S, S_real))) return rc;
    DENET_CHECK_ARG(dy && w && dx, "%s: null tensor", who);
    DENET_CHECK_ARG(C % 32 == 0, "%s: physical C (%d) must be a multiple of 32 (the network input has no gradient)", who, C);
    RectParams p = make_params(N, H, W, Cw, Kw, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    p.a = dy; p.b = w; p.out = dx; p.add = add;
    p.Hc = ceil_div(H, sh); p.Wc = ceil_div(W, sw);
    p.M = N * p.Hc * p.Wc; p.NC = Cw;
    p.div_img.init((uint32_t)(p.Hc * p.Wc));
    p.div_row.init((uint32_t)p.Wc);
    p.a_bytes = (unsigned)((long)N * OH * OW * K * 4);
    p.b_bytes = (unsigned)((long)K * R * S * Cw * 4);
    return launch_by_cols<DIL, GRP, PASS_DGRAD>(p, (unsigned)(sh * sw), GrpDims{C, K, C / Cw}, stream);
}

template <bool DIL, bool GRP = false>
int rect_wgrad(const char* who, const float* x, const float* dy, float* dw_out, float* workspace, size_t workspace_bytes, int N, int H,
               int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw, int OH, int OW,
               int Cw, int Kw, hipStream_t stream) {
    int rc = check_rect(who, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    if (rc) return rc;
    if (GRP && (rc = check_grp(who, C, K, Cw, Kw, S, S_real))) return rc;
    DENET_CHECK_ARG(x && dy && dw_out, "%s: null tensor", who);
    RectParams p = make_params(N, H, W, Cw, Kw, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW);
    p.a = dy; p.b = x;
    p.M = Kw; p.NC = R * S * Cw;
    p.ksteps = ceil_div(p.npix, BK);
    // (the slices are those of one window's problem: its sums run in the order of the plain pass on that window alone)
    const int splits = wgrad_splits(N, Cw, Kw, R, S, OH, OW);
    p.steps_per_split = ceil_div(p.ksteps, splits);
    p.split_stride = (long)K * p.NC;
    if (splits > 1) {
        DENET_CHECK_ARG(workspace && workspace_bytes >= (size_t)splits * p.split_stride * sizeof(float),
                        "%s: workspace of %zu bytes, %zu needed (denet_conv_%s_wgrad_workspace_bytes)", who, workspace_bytes,
                        (size_t)splits * p.split_stride * sizeof(float), GRP ? "grp" : "rect");
        p.out = workspace;
    } else {
        p.out = dw_out;
    }
    p.div_img.init((uint32_t)(OH * OW));
    p.div_row.init((uint32_t)OW);
    p.a_bytes = (unsigned)((long)N * OH * OW * K * 4);
    p.b_bytes = (unsigned)((long)N * H * W * C * 4);
    const GrpDims gd = {C, K, C / Cw};
    if (Kw >= 96) rc = launch_rect<DIL, GRP, PASS_WGRAD, 128, 128, 2, 2>(p, (unsigned)splits, gd, stream);
    else if (Kw >= 64) rc = launch_rect<DIL, GRP, PASS_WGRAD, 64, 128, 2, 2>(p, (unsigned)splits, gd, stream);
    else rc = launch_rect<DIL, GRP, PASS_WGRAD, 32, 128, 1, 4>(p, (unsigned)splits, gd, stream);
    if (rc) return rc;
    if (splits > 1) {
        const long n4 = p.split_stride / 4;
        hipLaunchKernelGGL(conv_rect_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, workspace, dw_out, n4,
                           splits);
        DENET_CHECK_LAUNCH("conv_rect_reduce");
    }
    return DENET_OK;
}

}  // namespace

extern "C" int denet_conv_rect_fwd(const float* x, const float* w, const float* bias, const float* add, float* y, int relu, int N,
                                   int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int OH,
                                   int OW, hipStream_t stream) {
    return rect_fwd<false>("conv_rect_fwd", x, w, bias, add, y, relu, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, 1, 1, OH, OW, C, K, stream);
}

extern "C" int denet_conv_rect_dgrad(const float* dy, const float* w, const float* add, float* dx, int N, int H, int W, int C, int K,
                                     int R, int S, int S_real, int sh, int sw, int ph, int pw, int OH, int OW,
                                     hipStream_t stream) {
    return rect_dgrad<false>("conv_rect_dgrad", dy, w, add, dx, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, 1, 1, OH, OW, C, K, stream);
}

extern "C" size_t denet_conv_rect_wgrad_workspace_bytes(int N, int C, int K, int R, int S, int OH, int OW) {
    if (N <= 0 || C <= 0 || K <= 0 || R <= 0 || S <= 0 || OH <= 0 || OW <= 0) return 0;
    const int sp = wgrad_splits(N, C, K, R, S, OH, OW);
    return sp > 1 ? (size_t)sp * K * R * S * C * sizeof(float) : 0;
}

extern "C" int denet_conv_rect_wgrad(const float* x, const float* dy, float* dw, float* workspace, size_t workspace_bytes, int N,
                                     int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int OH,
                                     int OW, hipStream_t stream) {
    return rect_wgrad<false>("conv_rect_wgrad", x, dy, dw, workspace, workspace_bytes, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, 1, 1,
                             OH, OW, C, K, stream);
}

extern "C" int denet_conv_dil_fwd(const float* x, const float* w, const float* bias, const float* add, float* y, int relu, int N,
                                  int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw,
                                  int OH, int OW, hipStream_t stream) {
    return rect_fwd<true>("conv_dil_fwd", x, w, bias, add, y, relu, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW, C, K, stream);
}

extern "C" int denet_conv_dil_dgrad(const float* dy, const float* w, const float* add, float* dx, int N, int H, int W, int C, int K,
                                    int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh, int dw, int OH, int OW,
                                    hipStream_t stream) {
    return rect_dgrad<true>("conv_dil_dgrad", dy, w, add, dx, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh, dw, OH, OW, C, K, stream);
}

extern "C" int denet_conv_dil_wgrad(const float* x, const float* dy, float* dw_out, float* workspace, size_t workspace_bytes, int N,
                                    int H, int W, int C, int K, int R, int S, int S_real, int sh, int sw, int ph, int pw, int dh,
                                    int dw, int OH, int OW, hipStream_t stream) {
    return rect_wgrad<true>("conv_dil_wgrad", x, dy, dw_out, workspace, workspace_bytes, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, dh,
                            dw, OH, OW, C, K, stream);
}

extern "C" int denet_conv_grp_fwd(const float* x, const float* w, const float* bias, const float* add, float* y, int relu, int N,
                                  int H, int W, int C, int K, int Cw, int Kw, int R, int S, int S_real, int sh, int sw, int ph, int pw,
                                  int OH, int OW, hipStream_t stream) {
    return rect_fwd<false, true>("conv_grp_fwd", x, w, bias, add, y, relu, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, 1, 1, OH, OW, Cw,
                                 Kw, stream);
}

extern "C" int denet_conv_grp_dgrad(const float* dy, const float* w, const float* add, float* dx, int N, int H, int W, int C, int K,
                                    int Cw, int Kw, int R, int S, int S_real, int sh, int sw, int ph, int pw, int OH, int OW,
                                    hipStream_t stream) {
    return rect_dgrad<false, true>("conv_grp_dgrad", dy, w, add, dx, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw, 1, 1, OH, OW, Cw, Kw,
                                   stream);
}

extern "C" size_t denet_conv_grp_wgrad_workspace_bytes(int N, int C, int K, int Cw, int Kw, int R, int S, int OH, int OW) {
    if (N <= 0 || C <= 0 || K <= 0 || Cw <= 0 || Kw <= 0 || R <= 0 || S <= 0 || OH <= 0 || OW <= 0) return 0;
    const int sp = wgrad_splits(N, Cw, Kw, R, S, OH, OW);
    return sp > 1 ? (size_t)sp * K * R * S * Cw * sizeof(float) : 0;
}

extern "C" int denet_conv_grp_wgrad(const float* x, const float* dy, float* dw, float* workspace, size_t workspace_bytes, int N,
                                    int H, int W, int C, int K, int Cw, int Kw, int R, int S, int S_real, int sh, int sw, int ph,
                                    int pw, int OH, int OW, hipStream_t stream) {
    return rect_wgrad<false, true>("conv_grp_wgrad", x, dy, dw, workspace, workspace_bytes, N, H, W, C, K, R, S, S_real, sh, sw, ph, pw,
                                   1, 1, OH, OW, Cw, Kw, stream);
}

namespace {

int check_slab(const char* who, const void* a, const void* b, int K, int R, int S, int Cg) {
    DENET_CHECK_ARG(a && b, "%s: null tensor", who);
    DENET_CHECK_ARG(K > 0 && K % 32 == 0, "%s: K (%d) must be a positive multiple of 32", who, K);
    DENET_CHECK_ARG(R > 0 && S > 0, "%s: non-positive filter extent (%d x %d)", who, R, S);
    DENET_CHECK_ARG(Cg == 1 || Cg == 2 || Cg == 4 || Cg == 8 || Cg == 16, "%s: group size Cg must be 1, 2, 4, 8 or 16 (got %d)", who, Cg);
    DENET_CHECK_ARG((long)K * R * S * 32 * 4 < 0xF0000000L, "%s: slab filter exceeds the 32-bit buffer extent (3.75 GiB)", who);
    return DENET_OK;
}

}  // namespace

extern "C" int denet_conv_grp_expand(const float* w, float* wd, int K, int R, int S, int Cg, hipStream_t stream) {
    const int rc = check_slab("conv_grp_expand", w, wd, K, R, S, Cg);
    if (rc) return rc;
    const long n4 = (long)K * R * S * 8;
    hipLaunchKernelGGL(grp_expand_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, w, wd, n4, R * S, ilog2_exact(Cg));
    DENET_CHECK_LAUNCH("conv_grp_expand");
    return DENET_OK;
}

extern "C" int denet_conv_grp_compact(const float* dwd, float* dw, int K, int R, int S, int Cg, hipStream_t stream) {
    const int rc = check_slab("conv_grp_compact", dwd, dw, K, R, S, Cg);
    if (rc) return rc;
    const long n = (long)K * R * S * Cg;
    hipLaunchKernelGGL(grp_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dwd, dw, n, R * S, ilog2_exact(Cg));
    DENET_CHECK_LAUNCH("conv_grp_compact");
    return DENET_OK;
}

