// Split-bf16 products on v_mfma_f32_32x32x16_bf16: the helpers of the kernels that run an f32-accurate
// product on the bf16 matrix pipe (potential_logreg.hip states the error analysis).
//
// Every f32 operand v is v1 + v2 + v3 with v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2)
// (the remainders are exact in f32); a product keeps the six plane pairs with i + j <= 4, small
// terms first, each an exact bf16 x bf16 product accumulated in f32.
//
// Fragment layouts of the 32x32x16 form, lane = (i, h) with i = lane & 31, h = lane >> 5:
//   A [32 x 16]: lane (i, h) holds A[i][8 h + j], j = 0..7
//   B [16 x 32]: lane (i, h) holds B[8 h + j][i], j = 0..7
//   C [32 x 32]: register r of lane (i, h) holds C[(r & 3) + 8 (r >> 2) + 4 h][i]
#pragma once
#include <hip/hip_runtime.h>

typedef float nmx_f32x16 __attribute__((ext_vector_type(16)));
typedef float nmx_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned nmx_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 nmx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 nmx_bf16x2 __attribute__((ext_vector_type(2)));

// (bf16(a), bf16(b)) in one word, a in the low half; and the two halves back as f32
__device__ __forceinline__ unsigned nmx_pk_bf16(float a, float b) {
  const nmx_f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, nmx_bf16x2));
}
__device__ __forceinline__ float nmx_pk_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float nmx_pk_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }

// the three planes of eight consecutive k elements of one lane
__device__ __forceinline__ void nmx_split3(const float (&v)[8], nmx_bf16x8& b1, nmx_bf16x8& b2, nmx_bf16x8& b3) {
  nmx_u32x4 w1, w2, w3;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = v[2 * p], x1 = v[2 * p + 1];
    const unsigned u1 = nmx_pk_bf16(x0, x1);
    const float e0 = x0 - nmx_pk_lo(u1), e1 = x1 - nmx_pk_hi(u1);
    const unsigned u2 = nmx_pk_bf16(e0, e1);
    const float f0 = e0 - nmx_pk_lo(u2), f1 = e1 - nmx_pk_hi(u2);
    w1[p] = u1;
    w2[p] = u2;
    w3[p] = nmx_pk_bf16(f0, f1);
  }
  b1 = __builtin_bit_cast(nmx_bf16x8, w1);
  b2 = __builtin_bit_cast(nmx_bf16x8, w2);
  b3 = __builtin_bit_cast(nmx_bf16x8, w3);
}

__device__ __forceinline__ nmx_f32x16 nmx_mma_bf16(const nmx_bf16x8& a, const nmx_bf16x8& b, nmx_f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// acc += A . B of one 16-deep k-block from the operands' planes: the six pairs, small terms first
__device__ __forceinline__ nmx_f32x16 nmx_mma_split(const nmx_bf16x8 (&a)[3], const nmx_bf16x8 (&b)[3],
                                                    nmx_f32x16 acc) {
  acc = nmx_mma_bf16(a[0], b[2], acc);
  acc = nmx_mma_bf16(a[1], b[1], acc);
  acc = nmx_mma_bf16(a[2], b[0], acc);
  acc = nmx_mma_bf16(a[0], b[1], acc);
  acc = nmx_mma_bf16(a[1], b[0], acc);
  return nmx_mma_bf16(a[0], b[0], acc);
}
