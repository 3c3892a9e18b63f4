// The operands of isg_gather_add and the value of one float4 of one of its rows: shared by the forward (csrc/isg_sgenc.hip) and by
// its backward (csrc/isg_sgenc_bwd.hip), which evaluates the pre-activation again with these very statements.
#pragma once
#include "isg_common.hpp"

namespace isg {

struct GatherAddArgs {
  const float4 *A;
  const int64_t *ia;
  const float4 *B;
  const int64_t *ib;
  const float4 *T;
  const int64_t *it;
  const float *sign;
  const float4 *D;
  const float4 *bias;
  float4 *out;
  _Float16 *planes;       // the rows as the planes32 operand of isg_linear_h3p (csrc/isg_gemm_h3p.hip), or NULL
  float *planes_inv;
  int64_t E;
  int Q;        // float4 per row
  int lda, ldb, ldt, ldd;   // row strides in float4
  int act;
};

__device__ __forceinline__ float4 gather_add_value(const GatherAddArgs &a, int64_t e, int c) {
  float4 v = a.A[(size_t)a.ia[e] * a.lda + c];
  if (a.B) {
    const float4 b = a.B[(size_t)a.ib[e] * a.ldb + c];
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  }
  if (a.T) {
    const float4 w = a.T[(size_t)a.it[e] * a.ldt + c];
    const float s = a.sign ? a.sign[e] : 1.f;
    v.x += s * w.x; v.y += s * w.y; v.z += s * w.z; v.w += s * w.w;
  }
  if (a.D) {
    const float4 d = a.D[(size_t)e * a.ldd + c];
    v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
  }
  if (a.bias) {
    const float4 b = a.bias[c];
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  }
  if (a.act == 1) { v.x = gelu_exact(v.x); v.y = gelu_exact(v.y); v.z = gelu_exact(v.z); v.w = gelu_exact(v.w); }
  return v;
}

}  // namespace isg
