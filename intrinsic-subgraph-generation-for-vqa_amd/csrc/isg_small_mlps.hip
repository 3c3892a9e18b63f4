// Up to four narrow MLPs over the same number of rows as ONE launch: chain = Linear(+GELU) or Linear, GELU, Linear(+GELU),
// every width a multiple of 32 and at most 128 (the question side of a step: the masked layers' ques_nn, the read-out's ques_nn).
//
// Each of these Linears is 0.13 GFLOP at 4096 rows: on isg_gemm.hip's 128 x 128 tiles it is 32 workgroups on 256 CUs, alone in
// the stream, 10-12 us.  Here a workgroup takes 32 rows of one chain (grid = row blocks x chains), so one launch puts
// 128 x chains workgroups on the chip, and a two-Linear chain keeps its intermediate in LDS.
//
// The bits are linear_bf16x6_kernel's (isg_gemm.hip), which is what makes this a drop-in: an output element of that kernel
// depends on its own row's three bf16 planes, the weight planes, the MFMA shape and lane map, the k order and the order of
// the six products -- none of which involves the number of rows a workgroup holds.  All of them are restated here:
//   split    x = p1 + p2 + p3, each plane the bf16 rounding (RNE) of what the previous ones left
//   MFMA     v_mfma_f32_32x32x16_bf16, lane l: A[row l & 31][k = 8 (l >> 5) .. + 7], W[n = l & 31][same k]
//   k order  16-wide steps in ascending k, ONE accumulator from zero (K <= 128: never the dual-accumulator form)
//   products (a1 b3) (a3 b1) (a2 b2) (a1 b2) (a2 b1) (a1 b1) per step, small terms first
//   epilogue + bias (or + 0.f), exact GELU (gelu_exact)
// and the intermediate of a two-Linear chain is the fp32 value the first launch would have stored, split again as rows
// loaded from memory are.  isg_gemm.hip itself is not touched.
//
//   A        the block's 32 rows are loaded once (32 x K fp32 <= 16 KB), split, and stay in LDS as [plane][row][K + 8 pad] bf16
//            (272-byte rows: the 16-byte fragment reads are conflict-free)
//   W        a wave owns 32 output columns over all 32 rows, so no other wave reads its weight rows: the fragments go from
//            the cached planes (isg_split_bf16x3, L2-resident: <= 96 KB per Linear) straight into registers, all k-steps at once
//   result   through an fp32 LDS block [32][128 + 4 pad]: the next Linear's operand, or 16-byte row stores
#include "isg_common.hpp"
#include "../../include/isg_fused.h"

#include <stdlib.h>

namespace isg {

typedef __attribute__((ext_vector_type(8))) __bf16 sm_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 sm_bf16x4;
typedef __attribute__((ext_vector_type(16))) float sm_f32x16;

constexpr int SM_ROWS = 32, SM_MAXW = ISG_SMALL_MLPS_MAX_WIDTH, SM_LD = SM_MAXW + 8, SM_MID_LD = SM_MAXW + 4, SM_THREADS = 256;
constexpr int SM_MAX_CHAINS = ISG_SMALL_MLPS_MAX_CHAINS;
constexpr int SM_MAX_KS = SM_MAXW / 16;

struct SmLinear {
  const __bf16 *w;       // planes[3][N][K] (K a multiple of 32: no padding)
  const float *bias;     // [N] or NULL
  int N, K, act;         // act: 0 none, 1 exact GELU
};
struct SmChain {
  const float *x;        // [M, lin[0].K], row stride ldx
  float *out;            // [M, last N], row stride ldo
  int ldx, ldo, n_lin;
  SmLinear lin[2];
};
struct SmArgs {
  SmChain c[SM_MAX_CHAINS];
  int M;
};

__device__ __forceinline__ float sm_bf16_to_f32(__bf16 v) {
  return __uint_as_float(((unsigned)__builtin_bit_cast(unsigned short, v)) << 16);
}
// isg_gemm.hip's split3, operation for operation
__device__ __forceinline__ void sm_split3(float x, __bf16 &p1, __bf16 &p2, __bf16 &p3) {
  p1 = (__bf16)x;
  const float r1 = x - sm_bf16_to_f32(p1);
  p2 = (__bf16)r1;
  const float r2 = r1 - sm_bf16_to_f32(p2);
  p3 = (__bf16)r2;
}

__global__ __launch_bounds__(SM_THREADS) void small_mlps_kernel(SmArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 sA[3][SM_ROWS][SM_LD];        // 26,112 B
  __shared__ __attribute__((aligned(16))) float mid[SM_ROWS][SM_MID_LD];       // 16,896 B
  const SmChain &ch = a.c[blockIdx.y];
  const int M = a.M;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * SM_ROWS;
  const int fr = lane & 31, fk = (lane >> 5) * 8, h = lane >> 5;

  // the block's rows -> registers (never a conditional load: clamp the address, mask at store time)
  const int K0 = ch.lin[0].K;
  float4 ra[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + SM_THREADS * u;
    const int row = i >> 5, c4 = i & 31;
    const int gr = min(m0 + row, M - 1), gk = min(c4 * 4, K0 - 4);
    ra[u] = *reinterpret_cast<const float4 *>(ch.x + (int64_t)gr * ch.ldx + gk);
  }

  for (int l = 0; l < ch.n_lin; ++l) {
    const SmLinear &lin = ch.lin[l];
    const int N = lin.N, K = lin.K, nks = K >> 4;
    const bool active = wave * 32 < N;      // wave-uniform: this wave's 32 columns exist
    // ---- this wave's weight fragments, every k-step at once (steps past K repeat the last one and are not used) ----
    sm_bf16x8 b[SM_MAX_KS][3];
    float bv = 0.f;
    if (active) {
      const int64_t plane_stride = (int64_t)N * K;
      const __bf16 *wrow = lin.w + (int64_t)(wave * 32 + fr) * K + fk;
#pragma unroll
      for (int ks = 0; ks < SM_MAX_KS; ++ks) {
        const int kk = min(ks, nks - 1) * 16;
#pragma unroll
        for (int q = 0; q < 3; ++q) b[ks][q] = *reinterpret_cast<const sm_bf16x8 *>(wrow + q * plane_stride + kk);
      }
      if (lin.bias) bv = lin.bias[wave * 32 + fr];
    }
    // ---- the operand rows -> three bf16 planes in LDS ----
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + SM_THREADS * u;
      const int row = i >> 5, c4 = i & 31;
      if (c4 * 4 < K) {
        float4 av;
        if (l == 0) {
          av = ra[u];
          if (m0 + row >= M) av = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          av = *reinterpret_cast<const float4 *>(&mid[row][c4 * 4]);
        }
        sm_bf16x4 p0, p1, p2;
        __bf16 t0, t1, t2;
        sm_split3(av.x, t0, t1, t2); p0[0] = t0; p1[0] = t1; p2[0] = t2;
        sm_split3(av.y, t0, t1, t2); p0[1] = t0; p1[1] = t1; p2[1] = t2;
        sm_split3(av.z, t0, t1, t2); p0[2] = t0; p1[2] = t1; p2[2] = t2;
        sm_split3(av.w, t0, t1, t2); p0[3] = t0; p1[3] = t1; p2[3] = t2;
        *reinterpret_cast<sm_bf16x4 *>(&sA[0][row][c4 * 4]) = p0;
        *reinterpret_cast<sm_bf16x4 *>(&sA[1][row][c4 * 4]) = p1;
        *reinterpret_cast<sm_bf16x4 *>(&sA[2][row][c4 * 4]) = p2;
      }
    }
    __syncthreads();      // the planes are complete; everyone has read what it needed of `mid`
    if (active) {
      sm_f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < SM_MAX_KS; ++ks) {
        if (ks < nks) {
          sm_bf16x8 af[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) af[q] = *reinterpret_cast<const sm_bf16x8 *>(&sA[q][fr][ks * 16 + fk]);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], b[ks][2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], b[ks][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], b[ks][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], b[ks][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], b[ks][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], b[ks][0], c, 0, 0, 0);
        }
      }
      // acc: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = c[r];
        v += bv;
        if (lin.act == 1) v = gelu_exact(v);
        mid[(r & 3) + 8 * (r >> 2) + 4 * h][wave * 32 + fr] = v;
      }
    }
    __syncthreads();      // the result block is complete; everyone is done with the planes
  }

  // ---- the last Linear's block -> 16-byte row stores ----
  const int NO = ch.lin[ch.n_lin - 1].N;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + SM_THREADS * u;
    const int row = i >> 5, c4 = i & 31;
    if (c4 * 4 < NO && m0 + row < M)
      *reinterpret_cast<float4 *>(ch.out + (int64_t)(m0 + row) * ch.ldo + c4 * 4) = *reinterpret_cast<const float4 *>(&mid[row][c4 * 4]);
  }
}

}  // namespace isg

using namespace isg;

static bool sm_width_ok(int64_t w) { return w >= 32 && w <= SM_MAXW && (w & 31) == 0; }

extern "C" int isg_fused_abi_version(void) { return ISG_FUSED_ABI_VERSION; }

// chains: HOST int64[n_chains][ISG_SMALL_MLPS_FIELDS], see include/isg_fused.h
extern "C" int isg_small_mlps(const int64_t *chains, int32_t n_chains, int64_t M, void *stream) {
  if (n_chains < 0 || n_chains > SM_MAX_CHAINS || M < 0) return ISG_EINVAL;
  if (n_chains == 0 || M == 0) return ISG_OK;
  if (!chains) return ISG_EINVAL;
  if (M >= (1ll << 31) - SM_ROWS) return ISG_EUNSUPPORTED;
  // isg_linear_bf16x6's diagnostic switches change ITS accumulation order: this launch would no longer be its drop-in
  static const bool other_order = [] {
    const char *r = getenv("ISG_GEMM_KROT"), *d = getenv("ISG_GEMM_DUAL_K");
    return (r && atoi(r) != 0) || (d && atoi(d) < SM_MAXW);
  }();
  if (other_order) return ISG_EUNSUPPORTED;
  SmChain cs[SM_MAX_CHAINS];
  for (int i = 0; i < SM_MAX_CHAINS; ++i) {
    const int64_t *f = chains + (int64_t)(i < n_chains ? i : 0) * ISG_SMALL_MLPS_FIELDS;     // unused slots repeat chain 0 (never run)
    const float *x = reinterpret_cast<const float *>(f[0]);
    float *out = reinterpret_cast<float *>(f[2]);
    const int64_t ldx = f[1], ldo = f[3], n_lin = f[4];
    if (n_lin < 1 || n_lin > 2 || !x || !out) return ISG_EINVAL;
    SmLinear lin[2];
    for (int l = 0; l < 2; ++l) {
      const int64_t *g = f + 5 + 5 * (l < n_lin ? l : 0);
      const int64_t N = g[2], K = g[3], act = g[4];
      if (!g[0] || act < 0 || act > 1) return ISG_EINVAL;
      if (!sm_width_ok(N) || !sm_width_ok(K)) return ISG_EUNSUPPORTED;
      if ((g[0] & 15) != 0 || (g[1] & 3) != 0) return ISG_EUNSUPPORTED;
      lin[l] = SmLinear{reinterpret_cast<const __bf16 *>(g[0]), reinterpret_cast<const float *>(g[1]), (int)N, (int)K, (int)act};
    }
    if (n_lin == 2 && lin[1].K != lin[0].N) return ISG_EINVAL;
    const int NO = lin[n_lin - 1].N;
    if (ldx < lin[0].K || ldo < NO || ldx >= (1ll << 31) || ldo >= (1ll << 31)) return ISG_EINVAL;
    if ((ldx & 3) != 0 || (ldo & 3) != 0 || (f[0] & 15) != 0 || (f[2] & 15) != 0) return ISG_EUNSUPPORTED;
    cs[i] = SmChain{x, out, (int)ldx, (int)ldo, (int)n_lin, {lin[0], lin[1]}};
  }
  SmArgs a = {{cs[0], cs[1], cs[2], cs[3]}, (int)M};
  dim3 grid((unsigned)((M + SM_ROWS - 1) / SM_ROWS), (unsigned)n_chains), block(SM_THREADS);
  small_mlps_kernel<<<grid, block, 0, as_stream(stream)>>>(a);
  return check_launch();
}
