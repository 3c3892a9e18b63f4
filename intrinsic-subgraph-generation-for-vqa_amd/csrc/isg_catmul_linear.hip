// D[M,N] = act(cat(a, b, a * b)[M,3C] . W[N,3C]^T + bias) without the concatenation in memory: the answer head's embedding
// Linear (isubgvqa.py:288-291), which ran as isg_cat_mul_rowmax (6 MB written, then read back) + isg_linear_f16x3_tile on
// 128 x 128 tiles (128 workgroups at 4096 rows).  Here a workgroup takes 32 rows x 128 columns (512 workgroups at 4096 x 512).
//
// The bits are those two launches': an element of linear_f16x3_tile_kernel's result (its 16x16x32 form) depends on its row's
// scale and two fp16 planes, the weight planes and inverse scales, the MFMA shape and lane map, the k order and the order of the
// three products -- not on the rows a workgroup holds.  Restated here:
//   row      [a | b | a * b], the product ONE fp32 multiply (cat_mul_rowmax_kernel's); mx = max |row| over all 3C values (a maximum
//            does not depend on the order it is taken in); h3_scale(mx) -> s, 1 / s
//   planes   v = x * s (exact: s is a power of two); hi = fp16(v), mid = fp16(v - hi)
//   MFMA     v_mfma_f32_16x16x32_f16, lane l: row / column l & 15, k = 8 (l >> 4) .. + 7 of a 32-wide k-tile; per k-tile
//            (a_hi w_mid) (a_mid w_hi) (a_hi w_hi); k-tiles ascending, one accumulator from zero (3C <= 640: one K-chunk)
//   epilogue (acc * 1/s_row) * 1/s_col, + bias, exact GELU (gelu_exact2), max |.| per 32 columns -> d_rowmax
// A block's planes stay in LDS for the whole K ([2][32][3C + 8] fp16, 50 KB at C = 128); a wave owns 32 columns, so its weight
// fragments go from the cached planes (isg_split_f16x2_rows) straight into registers, one k-tile ahead.
#include "isg_f16x3.hpp"
#include "../../include/isg_fused.h"

#include <stdlib.h>

namespace isg {

constexpr int CM_ROWS = 32, CM_COLS = 128, CM_MAXC = ISG_CATMUL_MAX_C, CM_LD = 3 * CM_MAXC + 8, CM_THREADS = 256;

struct CmArgs {
  const float *a;          // [M, C]
  const float *b;          // [M, C]
  const _Float16 *w;       // planes[2][N][3C]
  const float *w_inv;      // [N]
  const float *bias;       // [N] or NULL
  float *d;                // [M, N], row stride ldd
  float *d_rowmax;         // [M, N / 32] or NULL
  int M, N, C, ldd, act;
};

__global__ __launch_bounds__(CM_THREADS) void catmul_linear_kernel(CmArgs p) {
  __shared__ __attribute__((aligned(16))) _Float16 sA[2][CM_ROWS][CM_LD];      // 50,176 B
  __shared__ float s_inv[CM_ROWS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = p.M, N = p.N, C = p.C, K = 3 * C;
  const int m0 = blockIdx.y * CM_ROWS, n0 = blockIdx.x * CM_COLS;

  // ---- the block's rows of a and b: 8 lanes per row, up to 4 float4 of each per lane; scale; planes -------------------------
  {
    const int row = tid >> 3, t8 = tid & 7, Q = C >> 2;
    const int gr = min(m0 + row, M - 1);
    float4 va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = min(t8 + 8 * u, Q - 1);       // never a conditional load: clamp, mask below
      va[u] = reinterpret_cast<const float4 *>(p.a + (int64_t)gr * C)[c];
      vb[u] = reinterpret_cast<const float4 *>(p.b + (int64_t)gr * C)[c];
    }
    float mx = 0.f;
    float4 vp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (t8 + 8 * u >= Q || m0 + row >= M) {
        va[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        vb[u] = va[u];
      }
      const float4 x = va[u], y = vb[u];
      vp[u] = make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w);
      mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w))),
                           fmaxf(fmaxf(fabsf(y.x), fabsf(y.y)), fmaxf(fabsf(y.z), fabsf(y.w)))));
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(vp[u].x), fabsf(vp[u].y)), fmaxf(fabsf(vp[u].z), fabsf(vp[u].w))));
    }
    mx = fmaxf(mx, dpp_mov<ISG_DPP_XOR1>(mx));
    mx = fmaxf(mx, dpp_mov<ISG_DPP_XOR2>(mx));
    mx = fmaxf(mx, dpp_mov<ISG_DPP_HMIRROR>(mx));      // the 8 lanes of a row
    float s, inv;
    h3_scale(mx, s, inv);
    if (t8 == 0) s_inv[row] = inv;
    auto put = [&](int col, float4 v) {
      v.x *= s; v.y *= s; v.z *= s; v.w *= s;
      const hf16x4 hi = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
      const hf16x4 mid = {(_Float16)(v.x - (float)hi[0]), (_Float16)(v.y - (float)hi[1]), (_Float16)(v.z - (float)hi[2]),
                          (_Float16)(v.w - (float)hi[3])};
      *reinterpret_cast<hf16x4 *>(&sA[0][row][col]) = hi;
      *reinterpret_cast<hf16x4 *>(&sA[1][row][col]) = mid;
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = t8 + 8 * u;
      if (c < Q) {
        put(c * 4, va[u]);
        put(C + c * 4, vb[u]);
        put(2 * C + c * 4, vp[u]);
      }
    }
  }
  __syncthreads();

  const int wcol = n0 + wave * 32;
  if (wcol >= N) return;                 // wave-uniform; no barrier follows
  const int l15 = lane & 15, lk = (lane >> 4) * 8;
  const int64_t plane = (int64_t)N * K;
  const _Float16 *w0 = p.w + (int64_t)(wcol + l15) * K + lk;          // column tile j: + 16 * K
  hf32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = hf32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = K >> 5;
  hf16x8 bc[2][2], bn[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 2; ++q) bc[j][q] = *reinterpret_cast<const hf16x8 *>(w0 + q * plane + (int64_t)j * 16 * K);
  for (int kt = 0; kt < nk; ++kt) {
    const int kn = min(kt + 1, nk - 1) * 32;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) bn[j][q] = *reinterpret_cast<const hf16x8 *>(w0 + q * plane + (int64_t)j * 16 * K + kn);
    hf16x8 af[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 2; ++q) af[i][q] = *reinterpret_cast<const hf16x8 *>(&sA[q][i * 16 + l15][kt * 32 + lk]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        hf32x4 c = acc[i][j];
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], bc[j][1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][1], bc[j][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], bc[j][0], c, 0, 0, 0);
        acc[i][j] = c;
      }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) bc[j][q] = bn[j][q];
  }

  // ---- epilogue: acc[i][j][r] is row i * 16 + 4 (lane >> 4) + r, column wcol + j * 16 + (lane & 15) ---------------------------
  float wi[2], bv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    wi[j] = p.w_inv[wcol + j * 16 + l15];
    bv[j] = p.bias ? p.bias[wcol + j * 16 + l15] : 0.f;
  }
  const int NP = N >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float v[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ia = s_inv[i * 16 + 4 * (lane >> 4) + r];
        v[j][r] = (acc[i][j][r] * ia) * wi[j];
        if (p.bias) v[j][r] += bv[j];
      }
      if (p.act == 1) {
        const isg_f32x2 g0 = gelu_exact2(isg_f32x2{v[j][0], v[j][1]}), g1 = gelu_exact2(isg_f32x2{v[j][2], v[j][3]});
        v[j][0] = g0.x; v[j][1] = g0.y; v[j][2] = g1.x; v[j][3] = g1.y;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + i * 16 + 4 * (lane >> 4) + r;
      if (p.d_rowmax) {
        float mx = fmaxf(fabsf(v[0][r]), fabsf(v[1][r]));
        mx = fmaxf(mx, dpp_mov<ISG_DPP_XOR1>(mx));
        mx = fmaxf(mx, dpp_mov<ISG_DPP_XOR2>(mx));
        mx = fmaxf(mx, dpp_mov<ISG_DPP_HMIRROR>(mx));
        mx = fmaxf(mx, dpp_mov<ISG_DPP_MIRROR>(mx));      // the 16 lanes that hold the row's 32 columns
        if (l15 == 0 && row < M) p.d_rowmax[(int64_t)row * NP + (wcol >> 5)] = mx;
      }
      if (row < M) {
        float *dst = p.d + (int64_t)row * p.ldd + wcol + l15;
        dst[0] = v[0][r];
        dst[16] = v[1][r];
      }
    }
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_linear_f16x3_catmul(const float *a, const float *b, const uint16_t *w_planes, const float *w_inv_scale,
                                       const float *bias, float *d, float *d_rowmax, int64_t M, int32_t N, int32_t C,
                                       int32_t ldd, int32_t act, void *stream) {
  if (M < 0 || N <= 0 || C <= 0 || ldd < N || act < 0 || act > 1) return ISG_EINVAL;
  if (M == 0) return ISG_OK;
  if (!a || !b || !w_planes || !w_inv_scale || !d) return ISG_EINVAL;
  if ((C & 31) != 0 || C > CM_MAXC || (N & 31) != 0 || M >= (1ll << 31) - CM_ROWS) return ISG_EUNSUPPORTED;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(w_planes)) & 15) != 0)
    return ISG_EUNSUPPORTED;
  const long long mt = (M + CM_ROWS - 1) / CM_ROWS;
  if (mt > 65535) return ISG_EUNSUPPORTED;
  // the tile kernel's 32x32x16 form (a diagnostic switch) accumulates in another order: this launch is the 16x16x32 form's drop-in
  static const bool other_order = [] { const char *e = getenv("ISG_F16X3_MFMA"); return e && atoi(e) == 32; }();
  if (other_order) return ISG_EUNSUPPORTED;
  CmArgs p = {a, b, reinterpret_cast<const _Float16 *>(w_planes), w_inv_scale, bias, d, d_rowmax, (int)M, N, C, ldd, act};
  dim3 grid((unsigned)((N + CM_COLS - 1) / CM_COLS), (unsigned)mt), block(CM_THREADS);
  catmul_linear_kernel<<<grid, block, 0, as_stream(stream)>>>(p);
  return check_launch();
}
