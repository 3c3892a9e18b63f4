// Mask optimisation (include/ext/isg_maskopt.h, where the function is stated word for word): one iteration's arithmetic of a
// GNNExplainer run -- the gradient rows' dot with the unmasked rows, the sigmoid's derivative, the two regularisers, one Adam step
// on the row's logit, the next masked rows -- as one launch.
//
// Bandwidth-bound, no LDS and no matrix work; the work mapping of ig_attribution_kernel (csrc/isg_ig.hip): sixteen lanes per row,
// 16 bytes per lane and access, the row's segment by a binary search over the B + 1 range starts, the sixteen partial sums
// combined by a fixed xor-butterfly inside the lane group.  The sixteen lanes of a row compute its scalars alike (a dozen
// operations, cheaper than a broadcast) and lane 0 stores them: no atomics, one writer per output word.  Every number read from
// memory that becomes an address is compared first.
#include "isg_common.hpp"

#include "../../include/ext/isg_maskopt.h"

namespace isg {

constexpr int MO_THREADS = 256, MO_LANES = 16, MO_ROWS_PER_BLOCK = MO_THREADS / MO_LANES;
constexpr int MO_U = 5;          // float4 per lane and pass: 300 channels are 75 float4, five per lane

struct MaskoptArgs {
  const float *x;                // [N, 4 C4] row stride ldx
  int64_t ldx;
  const float *g;                // [N, 4 C4] row stride ldg; NULL: the apply-only form
  int64_t ldg;
  const int *seg;                // int32 [B + 1]
  int B;
  float *theta;                  // [N]
  float *exp_avg;                // [N]; may be NULL when g is
  float *exp_avg_sq;             // [N]; may be NULL when g is
  float *x_out;                  // [N, 4 C4] row stride ldxo
  int64_t ldxo;
  float *d_theta;                // optional [N]
  int64_t N;
  int C4;                        // float4 per row
  float a_size, a_ent;           // the header's A, E
  float w1, b2, w2, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// the header's sigmoid: rn(1 / rn(1 + expf(-t)))
__device__ __forceinline__ float mo_sigmoid(float t) { return div_rn(1.f, add_rn(1.f, expf(-t))); }

__device__ __forceinline__ bool mo_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(MO_THREADS) void maskopt_step_kernel(MaskoptArgs a) {
  const int lane = threadIdx.x & (MO_LANES - 1);
  const int64_t r = (int64_t)blockIdx.x * MO_ROWS_PER_BLOCK + threadIdx.x / MO_LANES;
  if (r >= a.N) return;                                          // (all sixteen lanes of a row leave together)
  // the first segment whose range ends behind row r (segments without rows are passed over); indices stay in [0, B]
  int lo = 0, hi = a.B - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a.seg[mid + 1] > r) hi = mid;
    else lo = mid + 1;
  }
  const int64_t r0 = a.seg[lo], r1 = a.seg[lo + 1];
  if (!(r0 <= r && r < r1)) return;                              // no segment holds this row: nothing of it is written
  const float4 *xin = reinterpret_cast<const float4 *>(a.x + r * a.ldx);
  float th = a.theta[r];
  if (a.g) {
    const float4 *gin = reinterpret_cast<const float4 *>(a.g + r * a.ldg);
    float s = 0.f;
    for (int c0 = lane; c0 < a.C4; c0 += MO_LANES * MO_U) {      // MO_U quads' loads in flight together, summed ascending
      float4 gv[MO_U], xv[MO_U];
#pragma unroll
      for (int u = 0; u < MO_U; ++u)
        if (c0 + u * MO_LANES < a.C4) {
          gv[u] = gin[c0 + u * MO_LANES];
          xv[u] = xin[c0 + u * MO_LANES];
        }
#pragma unroll
      for (int u = 0; u < MO_U; ++u)
        if (c0 + u * MO_LANES < a.C4) s = add_rn(s, dot4_rn(gv[u], xv[u]));
    }
    // the fixed butterfly inside the row's sixteen lanes; every lane of the group is here
#pragma unroll
    for (int m = MO_LANES / 2; m > 0; m >>= 1) s = add_rn(s, __shfl_xor(s, m, MO_LANES));
    const float m = mo_sigmoid(th);
    const float reg = div_rn(sub_rn(a.a_size, mul_rn(a.a_ent, th)), (float)(r1 - r0));
    const float d = mul_rn(add_rn(s, reg), mul_rn(m, sub_rn(1.f, m)));
    if (lane == 0 && a.d_theta) a.d_theta[r] = d;
    if (mo_finite(d)) {                                          // else: the row's update is skipped, x_out comes from the old logit
      float ea = a.exp_avg[r], es = a.exp_avg_sq[r];
      ea = add_rn(ea, mul_rn(sub_rn(d, ea), a.w1));
      es = add_rn(mul_rn(es, a.b2), mul_rn(mul_rn(d, d), a.w2));
      const float denom = add_rn(div_rn(sqrtf(es), a.bc2_sqrt), a.eps);
      th = sub_rn(th, mul_rn(a.step_size, div_rn(ea, denom)));
      if (lane == 0) {
        a.exp_avg[r] = ea;
        a.exp_avg_sq[r] = es;
        a.theta[r] = th;
      }
    }
  }
  const float mk = mo_sigmoid(th);
  float4 *dst = reinterpret_cast<float4 *>(a.x_out + r * a.ldxo);
  for (int c0 = lane; c0 < a.C4; c0 += MO_LANES * MO_U) {
    float4 v[MO_U];
#pragma unroll
    for (int u = 0; u < MO_U; ++u)
      if (c0 + u * MO_LANES < a.C4) v[u] = xin[c0 + u * MO_LANES];
#pragma unroll
    for (int u = 0; u < MO_U; ++u)
      if (c0 + u * MO_LANES < a.C4)
        dst[c0 + u * MO_LANES] = make_float4(mul_rn(mk, v[u].x), mul_rn(mk, v[u].y), mul_rn(mk, v[u].z), mul_rn(mk, v[u].w));
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_maskopt_abi_version(void) { return ISG_MASKOPT_ABI_VERSION; }

static inline bool mo_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }
static inline bool mo_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

extern "C" int isg_maskopt_step(const float *x, int32_t ldx, const float *g, int32_t ldg, const int32_t *seg, int64_t B,
                                float *theta, float *exp_avg, float *exp_avg_sq, float *x_out, int32_t ldxo, float *d_theta,
                                int64_t N, int32_t C, double a_size, double a_ent, double lr, double beta1, double beta2, double eps,
                                double bc1, double bc2, void *stream) {
  if (N < 0 || B < 0) return ISG_EINVAL;
  const bool step_ok = g && bc1 > 0.0 && bc2 > 0.0;              // (the apply-only form looks at neither bias correction)
  MaskoptArgs a = {.x = x, .ldx = ldx, .g = g, .ldg = ldg, .seg = seg, .B = (int)B, .theta = theta, .exp_avg = exp_avg,
                   .exp_avg_sq = exp_avg_sq, .x_out = x_out, .ldxo = ldxo, .d_theta = d_theta, .N = N, .C4 = C / 4,
                   .a_size = (float)a_size, .a_ent = (float)a_ent, .w1 = (float)(1.0 - beta1), .b2 = (float)beta2,
                   .w2 = (float)(1.0 - beta2), .step_size = step_ok ? (float)(lr / bc1) : 0.f,
                   .bc2_sqrt = step_ok ? (float)sqrt(bc2) : 1.f, .eps = (float)eps};
  if (a.N > 0 && (C < 1 || ldx < C || ldxo < C || !a.x || !a.seg || !a.theta || !a.x_out || B == 0)) return ISG_EINVAL;
  if (a.N > 0 && a.g && (ldg < C || !a.exp_avg || !a.exp_avg_sq || !step_ok)) return ISG_EINVAL;
  if (mo_too_large(N) || mo_too_large(B)) return ISG_EUNSUPPORTED;
  if (a.N > 0 && (((C | ldx | ldxo) & 3) || mo_misaligned(a.x) || mo_misaligned(a.x_out) ||
                  (a.g && ((ldg & 3) || mo_misaligned(a.g)))))
    return ISG_EUNSUPPORTED;
  if (a.N == 0) return ISG_OK;
  const int64_t blocks = (N + MO_ROWS_PER_BLOCK - 1) / MO_ROWS_PER_BLOCK;
  maskopt_step_kernel<<<(unsigned)blocks, MO_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
