// The exact three-term bf16 split of an fp32 value, shared by the forward GEMM (isg_gemm.hip) and the weight gradient
// (isg_linear_bwd.hip): x = x1 + x2 + x3 with xk the bf16 rounding (RNE) of the remainder, 8 + 8 + 8 significant bits.
#pragma once
#include "isg_common.hpp"

namespace isg {

__device__ __forceinline__ float bf16_to_f32(__bf16 v) {
  return __uint_as_float(((unsigned)__builtin_bit_cast(unsigned short, v)) << 16);
}

// x -> (x1, x2, x3), xk = bf16(remainder)
__device__ __forceinline__ void split3(float x, __bf16 &p1, __bf16 &p2, __bf16 &p3) {
  p1 = (__bf16)x;
  const float r1 = x - bf16_to_f32(p1);
  p2 = (__bf16)r1;
  const float r2 = r1 - bf16_to_f32(p2);
  p3 = (__bf16)r2;
}

}  // namespace isg
