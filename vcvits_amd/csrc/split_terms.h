// split_terms.h -- the split-operand arithmetic shared by conv_x3.hip and wgrad_dma.hip: an fp32 operand as three exact bf16
// terms, and the six (or nine) bf16 MFMA products of two split operands, small terms first.
#pragma once

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// one term a_PA * b_PB of the split product on every accumulator tile of the wave (literal plane indices: a computed
// index makes the compiler select fragment registers at run time)
template <int PA, int PB, int TM, int TN>
__device__ __forceinline__ void mma_term(f32x16 (&acc)[TM][TN], const bf16x8 (&a)[TM][3], const bf16x8 (&b)[TN][3]) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
      acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm][PA], b[tn][PB], acc[tm][tn], 0, 0, 0);
}

// the NTERM terms of one split product, small terms first
template <int NTERM, int TM, int TN>
__device__ __forceinline__ void mma_product(f32x16 (&acc)[TM][TN], const bf16x8 (&a)[TM][3], const bf16x8 (&b)[TN][3]) {
  if (NTERM == 9) {
    mma_term<2, 2>(acc, a, b);
    mma_term<1, 2>(acc, a, b);
    mma_term<2, 1>(acc, a, b);
  }
  mma_term<0, 2>(acc, a, b);
  mma_term<2, 0>(acc, a, b);
  mma_term<1, 1>(acc, a, b);
  mma_term<0, 1>(acc, a, b);
  mma_term<1, 0>(acc, a, b);
  mma_term<0, 0>(acc, a, b);
}

__device__ __forceinline__ void split3(float f, __bf16& t0, __bf16& t1, __bf16& t2) {
  t0 = (__bf16)f;
  const float r1 = f - (float)t0;   // exact
  t1 = (__bf16)r1;
  const float r2 = r1 - (float)t1;  // exact, and representable in 8 bits
  t2 = (__bf16)r2;
}
