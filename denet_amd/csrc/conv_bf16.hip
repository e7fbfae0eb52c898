// OPT-IN inference variant, never the headline path: the forward pass of a square convolution with both operands rounded to
// bf16 and multiplied on the bf16 matrix cores of gfx950 (MI355X),
//     y = epilogue( sum over taps and channels of bf16(x) * bf16(w) ),   accumulated in fp32 by v_mfma_f32_32x32x16_bf16
// (ops.INFER_PRECISION = "bf16", model-predict --precision bf16; the numerics contract is in DESIGN.md). This is NOT the exact
// fp32 FMA chain of igemm.hip: an operand keeps 8 mantissa bits, so the result lies outside the 1e-3 parity budget by design.
//
// Layout (HBM):   activations NHWC fp32 (rounded to nearest-even when they are staged), filters [K][R][S][C] as igemm.hip but
//                 bf16 (denet_filter_to_bf16, made once per weights version by the caller), bias / add / y fp32.
// Implicit GEMM:  N*OH*OW pixels x K filters, reduction over R*S*C in chunks of 32 channels of one tap (C % 32 = 0, so a chunk
//                 never spans two taps); padding taps read as zero through the buffer descriptor.
// Tiling:         256 threads (4 wave64) per 128 x BN output tile, BN = 128 / 64 / 32 by K alone (conv_rect.hip's table: nothing
//                 is measured, the same kernel in every process). Two LDS buffers, each a bf16 image of the A tile and of the B
//                 tile with rows of 80 bytes (32 bf16 + 16 bytes of padding: the 16-byte fragment reads of 16 consecutive rows
//                 cover all 64 banks, gemm3b.hip). The next chunk travels global -> VGPR while the current one is multiplied;
//                 it is converted and written to the other buffer behind the products; one barrier per chunk.
// Order:          every output element is one fixed chain chunk by chunk, 2 MFMA k-steps per chunk: bit-identical run to run.
#include "bf16_mma.h"
#include "../../include/denet_hip.h"

namespace {

constexpr int BK = 32;

struct Bf16Params {
    const float* x;                // [N][H][W][C] fp32
    const unsigned short* w16;     // [K][R][S][C] bf16
    const float* bias;             // [K] or null
    const float* add;              // [N][OH][OW][K] or null
    float* y;                      // [N][OH][OW][K]
    int relu;
    int N, H, W, C, K, R, S, stride, pad, OH, OW;
    int M;                         // N*OH*OW
    int ksteps;                    // R*S*C / 32
    int tiles_n;
    FastDiv div_img, div_row;      // OH*OW, OW
    unsigned x_bytes, w_bytes;
};

template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_bf16_kernel(const Bf16Params p) {
    static_assert(BM == 128 && (BN == 128 || BN == 64 || BN == 32), "tile table");
    constexpr int WN = BN >= 64 ? 2 : 1, WM = 4 / WN;       // waves along the filters / the pixels
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);  // 32 x 32 MFMA tiles of a wave
    constexpr int PA = BM / 32;                             // A loader passes: 32 rows of 8 float4 each
    constexpr int PB = BN >= 64 ? BN / 64 : 1;              // B loader passes: 64 rows of 4 x 16 bytes each
    constexpr int SZA = BM * ROWB, SZB = BN * ROWB;

    __shared__ __attribute__((aligned(16))) char smem[2 * (SZA + SZB)];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    const uint32_t tile_id = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (int)(tile_id / p.tiles_n) * BM, n0 = (int)(tile_id % p.tiles_n) * BN;

    // ---------------- loaders ----------------
    // A: lane = (pixel row tid / 8 of a 32-row pass, float4 tid % 8 of the chunk's 32 channels): im2col addressing of igemm.hip
    const int q8 = tid & 7, row8 = tid >> 3;
    int a_off[PA], a_y[PA], a_x[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + row8 + 32 * i;
        a_y[i] = -(p.R + 1); a_x[i] = 0; a_off[i] = 0;      // a row that is none: every tap lies above the image
        if (m < p.M) {
            const uint32_t n = p.div_img.div(m);
            const uint32_t rem = m - n * (p.OH * p.OW);
            const uint32_t oy = p.div_row.div(rem);
            const uint32_t ox = rem - oy * p.OW;
            a_y[i] = (int)oy * p.stride - p.pad;
            a_x[i] = (int)ox * p.stride - p.pad;
            a_off[i] = (((int)n * p.H + a_y[i]) * p.W + a_x[i]) * p.C + 4 * q8;
        }
    }
    // B: lane = (filter row tid / 4 of a 64-row pass, 16-byte piece tid % 4 of the chunk's 64 bytes)
    const int q4 = tid & 3, row4 = tid >> 2;
    const int rsc = p.R * p.S * p.C;
    int b_off[PB];
    bool b_ok[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int r = row4 + 64 * i;
        b_ok[i] = r < BN && n0 + r < p.K;
        b_off[i] = b_ok[i] ? (int)(((unsigned)(n0 + r) * rsc + 8 * q4) * 2u) : 0;          // bytes
    }
    const __amdgpu_buffer_rsrc_t r_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w16, 0, p.w_bytes, 0x00020000);

    int cur_r = 0, cur_s = 0, cur_c = 0, cur_step = 0;       // wave-uniform reduction cursor
    f32x4 ra[PA];
    u32x4 rb[PB];

    auto load_chunk = [&]() {
        const int u_off = (cur_r * p.W + cur_s) * p.C + cur_c;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const bool ok = ((unsigned)(a_y[i] + cur_r) < (unsigned)p.H) && ((unsigned)(a_x[i] + cur_s) < (unsigned)p.W);
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_x, ok ? (int)((unsigned)(a_off[i] + u_off) * 4u) : OOBV, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < PB; ++i)
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(r_w, b_ok[i] ? b_off[i] + cur_step * (BK * 2) : OOBV, 0, 0);
        cur_c += BK;
        if (cur_c >= p.C) {
            cur_c = 0;
            if (++cur_s >= p.S) { cur_s = 0; ++cur_r; }
        }
        ++cur_step;
    };

    auto store_chunk = [&](int buf) {
        char* da = smem + buf * (SZA + SZB);
        char* db = da + SZA;
#pragma unroll
        for (int i = 0; i < PA; ++i)
            *(u32x2*)(da + (row8 + 32 * i) * ROWB + q8 * 8) = u32x2{pack2(ra[i][0], ra[i][1]), pack2(ra[i][2], ra[i][3])};
#pragma unroll
        for (int i = 0; i < PB; ++i)
            if (row4 + 64 * i < BN) *(u32x4*)(db + (row4 + 64 * i) * ROWB + q4 * 16) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment addresses: lane = (row l & 31 of a 32-row tile, group l >> 5 of 8 consecutive k)
    const int arow = wm * (TM * 32) + li;
    const int brow = wn * (TN * 32) + li;
    const int fa = arow * ROWB + lh * 16;
    const int fb = brow * ROWB + lh * 16;

    load_chunk();
    store_chunk(0);
    __syncthreads();
    for (int st = 0; st < p.ksteps; ++st) {
        const bool more = st + 1 < p.ksteps;
        if (more) load_chunk();
        const char* ca = smem + (st & 1) * (SZA + SZB);
        const char* cb = ca + SZA;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = *(const bf16x8*)(ca + fa + i * 32 * ROWB + ks * 32);
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = *(const bf16x8*)(cb + fb + j * 32 * ROWB + ks * 32);
            // the filters as the first operand: a lane's accumulator then holds 4-element runs along K (16-byte stores)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bv[j], av[i], acc[i][j], 0, 0, 0);
        }
        if (more) store_chunk((st + 1) & 1);
        __syncthreads();
    }

    // ---------------- epilogue: the lane owns pixel m = .. + li, filters 8g + 4h .. +3 in registers 4g .. 4g+3 ----------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + arow + 32 * i;
        if (m >= p.M) continue;
        const long row = (long)m * p.K;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * (TN * 32) + 32 * j + 8 * g + 4 * lh;
                if (n >= p.K) continue;
                f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                if (p.bias) v += *(const f32x4*)(p.bias + n);
                if (p.add) v += *(const f32x4*)(p.add + row + n);
                if (p.relu) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
                }
                *(f32x4*)(p.y + row + n) = v;
            }
        }
    }
}

// w16[i] = bf16(w[i]), round to nearest-even; one pair per thread
__global__ __launch_bounds__(256) void filter_to_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ w16, long n) {
    const long i = 2 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (i + 1 < n) {
        *(unsigned*)(w16 + i) = pack2(w[i], w[i + 1]);
    } else if (i < n) {
        w16[i] = (unsigned short)(pack2(w[i], 0.f) & 0xFFFFu);
    }
}

template <int BN>
int launch_bf16(Bf16Params& p, hipStream_t stream) {
    constexpr int BM = 128;
    p.tiles_n = ceil_div(p.K, BN);
    const int tiles_m = ceil_div(p.M, BM);
    const int prof = denet_prof_begin(21, BM, BN, 0, stream);          // ops.kernel_symbol: conv_bf16_kernel<BM, BN>
    hipLaunchKernelGGL((conv_bf16_kernel<BM, BN>), dim3((unsigned)(tiles_m * p.tiles_n)), dim3(256), 0, stream, p);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("conv_fwd_bf16");
    return DENET_OK;
}

}  // namespace

extern "C" int denet_filter_to_bf16(const float* w, void* w16, long n, hipStream_t stream) {
    DENET_CHECK_ARG(n > 0 && n < (1L << 40), "filter_to_bf16: element count %ld out of range", n);
    DENET_CHECK_ARG(w && w16, "filter_to_bf16: null pointer");
    const long pairs = (n + 1) / 2;
    hipLaunchKernelGGL(filter_to_bf16_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, stream, w, (unsigned short*)w16, n);
    DENET_CHECK_LAUNCH("filter_to_bf16");
    return DENET_OK;
}

extern "C" int denet_conv_fwd_bf16(const float* x, const void* w16, const float* bias, const float* add, float* y, int relu, int N,
                                   int H, int W, int C, int K, int R, int S, int S_real, int stride, int pad, int OH, int OW,
                                   hipStream_t stream) {
    int rc = check_conv_bf16("conv_fwd_bf16", N, H, W, C, K, R, S, S_real, stride, pad, OH, OW);
    if (rc) return rc;
    DENET_CHECK_ARG(x && w16 && y, "conv_fwd_bf16: null tensor");
    Bf16Params p = {};
    p.x = x; p.w16 = (const unsigned short*)w16; p.bias = bias; p.add = add; p.y = y; p.relu = relu ? 1 : 0;
    p.N = N; p.H = H; p.W = W; p.C = C; p.K = K; p.R = R; p.S = S; p.stride = stride; p.pad = pad; p.OH = OH; p.OW = OW;
    p.M = N * OH * OW;
    p.ksteps = R * S * C / BK;
    p.div_img.init((uint32_t)(OH * OW));
    p.div_row.init((uint32_t)OW);
    p.x_bytes = (unsigned)((long)N * H * W * C * 4);
    p.w_bytes = (unsigned)((long)K * R * S * C * 2);
    if (K >= 96) return launch_bf16<128>(p, stream);
    if (K >= 64) return launch_bf16<64>(p, stream);
    return launch_bf16<32>(p, stream);
}
