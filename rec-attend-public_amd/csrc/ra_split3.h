// The exact three-piece bf16 split of float32 values, shared by the SPLIT forms of the conv kernels (ra_conv_pair8.hip,
// ra_conv_wino.hip, ra_conv_split.hip), and the vector types those files share.
#pragma once
#include <hip/hip_runtime.h>

namespace ra {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// v_cvt_pk_bf16_f32: two floats -> two bf16 (RNE), `lo` in the low half
__device__ inline unsigned pk_bf16(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// (a, b) -> three packed bf16 pairs H, M, L with a = a_H + a_M + a_L exactly (every difference below is exact in float32): a
// float32 value is the sum of three bf16 pieces (8 + 8 + 8 mantissa bits), and products of bf16 numbers are exact in float32
__device__ inline void split3_pair(float a, float b, unsigned &H, unsigned &M, unsigned &L) {
  H = pk_bf16(a, b);
  float ra = a - __builtin_bit_cast(float, H << 16), rb = b - __builtin_bit_cast(float, H & 0xffff0000u);
  M = pk_bf16(ra, rb);
  ra -= __builtin_bit_cast(float, M << 16);
  rb -= __builtin_bit_cast(float, M & 0xffff0000u);
  L = pk_bf16(ra, rb);
}

}  // namespace ra
