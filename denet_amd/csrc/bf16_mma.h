// What the kernels on the bf16 matrix cores share (conv_bf16.hip, conv_bf16_train.hip, gemm3b.hip): the operand vector types, the
// fp32 -> bf16 packing, the LDS row of a 32-wide bf16 chunk and the geometry rules of the bf16 convolution entry points.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int ROWB = 80;                              // bytes per LDS row: 32 bf16 + 16 bytes of padding
constexpr int OOBV = (int)0xF0000000u;                // beyond every extent check_conv_bf16 admits: the lane reads 0

// 2 fp32 -> 2 bf16 in one dword (v_cvt_pk_bf16_f32, round to nearest-even)
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// the geometry rules of conv_bf16.hip's forward kernel, which is the data gradient's kernel too and whose limits the filter
// gradient shares, reported under the caller's name
static inline int check_conv_bf16(const char* who, int N, int H, int W, int C, int K, int R, int S, int S_real, int stride, int pad,
                                  int OH, int OW) {
    DENET_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && R > 0 && S > 0, "%s: non-positive dimension", who);
    DENET_CHECK_ARG(C % 32 == 0, "%s: physical C (%d) must be a multiple of 32", who, C);
    DENET_CHECK_ARG(K % 32 == 0, "%s: physical K (%d) must be a multiple of 32", who, K);
    DENET_CHECK_ARG(R == S && S_real == S, "%s: square filters with every tap real (R %d, S %d, S_real %d)", who, R, S, S_real);
    DENET_CHECK_ARG(ilog2_exact(stride) >= 0, "%s: stride must be a power of two (got %d)", who, stride);
    DENET_CHECK_ARG(pad >= 0, "%s: negative pad", who);
    DENET_CHECK_ARG(H + 2 * pad >= R && OH > 0 && (H + 2 * pad - R) / stride + 1 >= OH, "%s: OH=%d inconsistent", who, OH);
    DENET_CHECK_ARG(W + 2 * pad >= S && OW > 0 && (W + 2 * pad - S) / stride + 1 >= OW, "%s: OW=%d inconsistent", who, OW);
    // operands are addressed through 32-bit buffer descriptors (byte offsets); 0xF0000000 is the out-of-range marker
    DENET_CHECK_ARG((long)N * H * W * C * 4 < 0xF0000000L && (long)N * OH * OW * K * 4 < 0xF0000000L &&
                        (long)K * R * S * C * 4 < 0xF0000000L,
                    "%s: tensor exceeds the 32-bit buffer extent (3.75 GiB)", who);
    return DENET_OK;
}
