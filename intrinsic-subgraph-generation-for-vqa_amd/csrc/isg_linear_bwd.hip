// A Linear's backward (include/isg_linear_train.h).
//
// 1. isg_linear_bwd_prep: one pass over the upstream gradient g [M, N] that applies the activation's derivative (dz) and sums the
//    columns of dz into partial rows for the bias gradient.  Bound by memory: g and the saved tensor are read once, dz written once.
//
// 2. isg_linear_wgrad_bf16x6: dW[N, K] = g^T x on v_mfma_f32_32x32x16_bf16.  isg_wgrad.hip's shape (a split-M GEMM: grid =
//    (N / 128) x (K / 128) x splits, a workgroup reduces its rows into a 128 x 128 partial tile, the caller adds the partials in
//    split order, the rows of the next two stages are fetched into registers while the current ones are multiplied), with the
//    fp32-input matrix instruction (vector rate) replaced by the forward's six bf16 products.
//    The bf16 instruction wants, for both operands, eight consecutive values along the contraction axis -- here the ROW index m of
//    the row-major g and x -- for the column `lane & 31`: a transpose of both.  gfx950's transposed LDS read (ds_read_b64_tr_b16)
//    does it on the way out of LDS: the three bf16 planes of a value (split3 of isg_bf16x3.hpp, the forward's) are written as
//    [plane][row m][128 columns] images of 16-bit elements, 256-byte rows, and a 16-lane group reads a block of 4 rows x 16
//    columns column-major: lane 4 q + p of the group addresses row q, columns 4 p .. 4 p + 3, lane i receives column i of the four
//    rows.  Two such reads (rows 8 h .. 8 h + 3 and 8 h + 4 .. 8 h + 7, h = lane >> 5) make the operand of one 16-row step.
//    The 16-byte chunks of a row are XOR-swizzled (chunk ^ (((row & 3) << 2) | ((row >> 2) & 3))): with plain 256-byte rows the
//    four rows of a block sit on the same banks and the read is 4-way conflicted.  Every lane's address is 8-byte aligned, and
//    the reads run with all 64 lanes active: rows beyond a split's end and columns beyond N / K are ZERO-FILLED in LDS, never
//    masked out.
//    LDS: stages of 16 rows, two of them (2 stages x 2 operands x 3 planes x 16 x 128 x 2 B = 48 KB static), so that one barrier
//    per stage suffices (stage s + 1 is written while slower waves still read stage s) and two workgroups share a CU (96 of 160 KB):
//    the second workgroup's MFMAs cover the first one's split / LDS-write phase.  32-row stages would need 96 KB for two, one
//    workgroup per CU; a single 32-row stage needs two barriers per step with nothing to cover the write phase inside a workgroup.
//    Per 16-row step a wave issues 12 MFMAs (2 tiles x 6 products, 32 cycles each) and 18 transposed reads.
#include "isg_common.hpp"
#include "isg_bf16x3.hpp"
#include "isg_diag.hpp"
#include "../../include/isg_linear_train.h"

#include <stdlib.h>

namespace isg {

// ------------------------------------------------------------------------------------------------
// prep: dz and the bias partials
// ------------------------------------------------------------------------------------------------
constexpr int LP_THREADS = 256;
constexpr int LP_MAX_PARTS = 1024;
constexpr int LP_MIN_ROWS = 32;   // rows a workgroup owns at least (M permitting): below that a launch is all prologue

template <int MODE>
__device__ __forceinline__ float lp_apply(float g, float s) {
  if (MODE == 1) {          // GELU'(z) = Phi(z) + z phi(z), the erf form of aten.gelu_backward
    const float cdf = 0.5f * (1.0f + erff(s * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * s * s) * 0.39894228040143267794f;
    return g * (cdf + s * pdf);
  }
  if (MODE == 2) return mul_rn(g, s > 0.f ? 1.0f : 0.0f);   // a product: Inf or NaN in g at a masked position gives NaN
  return g;
}

// Columns are taken in groups of four that start on 16-byte boundaries of the rows (`off` = floats by which column 0 lies past
// one, 0 when the tensors do not share it): group j = columns 4 j - off .. 4 j - off + 3.  A group inside [0, N) moves as float4
// when `vec`; everything else as guarded scalars.  Thread (ty, tx) of TY x TX = 256 takes the groups tx, tx + TX, ... and, of
// every block of TY rows, row ty; the TY chains of a group are added in chain order by the threads ty = 0.
template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void linear_bwd_prep_kernel(const float *__restrict__ g, int ldg,
                                                                     const float *__restrict__ saved, int lds,
                                                                     float *__restrict__ dz, int lddz,
                                                                     float *__restrict__ db_part, int M, int N, int rows_per_wg,
                                                                     int tx_log2, int off, int vec) {
  __shared__ float4 red[LP_THREADS];
  const int tid = threadIdx.x;
  const int TX = 1 << tx_log2, TY = LP_THREADS >> tx_log2;
  const int tx = tid & (TX - 1), ty = tid >> tx_log2;
  const int64_t m_begin64 = (int64_t)blockIdx.x * rows_per_wg;
  const int m_begin = (int)(m_begin64 < M ? m_begin64 : M);
  const int m_end = (int)(m_begin64 + rows_per_wg < M ? m_begin64 + rows_per_wg : M);
  const int groups = (N + off + 3) >> 2;
  for (int jb = 0; jb < groups; jb += TX) {     // uniform over the workgroup: the barriers below are reached by every thread
    const int j = jb + tx;
    const int c0 = 4 * j - off;
    const bool live = j < groups;
    const bool full = live && vec && c0 >= 0 && c0 + 4 <= N;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      for (int m = m_begin + ty; m < m_end; m += TY) {
        const float *gp = g + (int64_t)m * ldg + c0;
        float4 v;
        if (full) {
          v = *reinterpret_cast<const float4 *>(gp);
          if (MODE != 0) {
            const float4 s = *reinterpret_cast<const float4 *>(saved + (int64_t)m * lds + c0);
            v.x = lp_apply<MODE>(v.x, s.x);
            v.y = lp_apply<MODE>(v.y, s.y);
            v.z = lp_apply<MODE>(v.z, s.z);
            v.w = lp_apply<MODE>(v.w, s.w);
          }
          if (dz) *reinterpret_cast<float4 *>(dz + (int64_t)m * lddz + c0) = v;
        } else {
          float e[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = c0 + u;
            e[u] = 0.f;
            if (c >= 0 && c < N) {
              float val = gp[u];
              if (MODE != 0) val = lp_apply<MODE>(val, saved[(int64_t)m * lds + c]);
              if (dz) dz[(int64_t)m * lddz + c] = val;
              e[u] = val;
            }
          }
          v = make_float4(e[0], e[1], e[2], e[3]);
        }
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
    if (db_part) {
      if (TY > 1) {
        red[tid] = acc;
        __syncthreads();
        if (ty == 0) {
          for (int t = 1; t < TY; ++t) {
            const float4 o = red[(t << tx_log2) + tx];
            acc.x += o.x;
            acc.y += o.y;
            acc.z += o.z;
            acc.w += o.w;
          }
        }
        __syncthreads();
      }
      if (ty == 0 && live) {
        float *dst = db_part + (int64_t)blockIdx.x * N;
        const float e[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + u;
          if (c >= 0 && c < N) dst[c] = e[u];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// dW on the bf16 matrix cores
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 lb_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 lb_bf16x4;
typedef __attribute__((ext_vector_type(4))) short lb_i16x4;
typedef __attribute__((ext_vector_type(8))) short lb_i16x8;
typedef __attribute__((ext_vector_type(16))) float lb_f32x16;

constexpr int LB_T = 128;            // output tile (n and k)
constexpr int LB_BM = 16;            // rows per stage = the contraction depth of one MFMA
constexpr int LB_ROW_BYTES = LB_T * 2;
constexpr int LB_PLANE_BYTES = LB_BM * LB_ROW_BYTES;         // 4 KB
constexpr int LB_OPERAND_BYTES = 3 * LB_PLANE_BYTES;         // 12 KB
constexpr int LB_STAGE_BYTES = 2 * LB_OPERAND_BYTES;         // g and x: 24 KB
constexpr int LB_SMEM_BYTES = 2 * LB_STAGE_BYTES;            // 48 KB

// byte offset of 16-byte chunk `ch` (0..15) of row `row` (0..15) inside a plane image: 256-byte rows, chunks XOR-swizzled
__device__ __forceinline__ int lb_off(int row, int ch) {
  return LB_ROW_BYTES * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef __attribute__((address_space(3))) lb_i16x4 lb_lds_i16x4;

// the eight values along m (rows 8 h .. 8 h + 7 of the stage) of column `lane & 31` of a 32-column block: two transposed reads.
// a0 / a1: this lane's byte addresses for the rows 8 h + q and 8 h + 4 + q (lb_tr_addr)
__device__ __forceinline__ lb_bf16x8 lb_tr_read(const unsigned char *plane, int a0, int a1) {
  const lb_i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lb_lds_i16x4 *)(plane + a0));
  const lb_i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lb_lds_i16x4 *)(plane + a1));
  const lb_i16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(lb_bf16x8, v);
}

// lane -> its address in the block of 4 rows from r0 and 16 columns from column c0 (a multiple of 16): lane 4 q + p of the
// 16-lane group supplies row r0 + q, columns c0 + 4 p .. + 3
__device__ __forceinline__ int lb_tr_addr(int lane, int r0, int cblock) {
  const int i = lane & 15, q = i >> 2, p = i & 3;
  const int c0 = cblock + 16 * ((lane >> 4) & 1);     // the two groups of a 32-lane half take the two 16-column blocks
  return lb_off(r0 + q, (c0 >> 3) + (p >> 1)) + 8 * (p & 1);
}

// GV / XV: g / x moves as float4 (base 16-byte aligned, pitch and column count multiples of 4: a float4 then lies wholly inside
// the matrix or wholly outside); otherwise as scalars
template <bool GV, bool XV>
__global__ __launch_bounds__(512, 2) void wgrad_bf16x6_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                              float *__restrict__ partial, int M, int N, int K, int ldg,
                                                              int ldx, int rows_per_split) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LB_SMEM_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 3, wn = wave >> 2;
  const int n0 = blockIdx.x * LB_T, k0 = blockIdx.y * LB_T;
  const int64_t mb64 = (int64_t)blockIdx.z * rows_per_split;
  const int m_begin = (int)(mb64 < M ? mb64 : M);
  const int m_end = (int)(mb64 + rows_per_split < M ? mb64 + rows_per_split : M);
  lb_f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

  // a stage = 16 rows x 128 columns = 512 float4 per operand: one per thread (row lr, float4 column c4)
  const int lr = tid >> 5, c4 = tid & 31;
  // never a conditional load (the compiler would wait for it at once): clamp the address, mask when the stage is written
  auto load4 = [&](const float *base, int ld, int64_t row, int col0, int ncols, auto vec) -> float4 {   // int64: M may be 2^31 - 1
    const float *p = base + (size_t)(row < m_end ? row : m_end - 1) * ld;
    if constexpr (decltype(vec)::value) return *reinterpret_cast<const float4 *>(p + min(col0, ncols - 4));
    float4 v;
    v.x = p[min(col0 + 0, ncols - 1)];
    v.y = p[min(col0 + 1, ncols - 1)];
    v.z = p[min(col0 + 2, ncols - 1)];
    v.w = p[min(col0 + 3, ncols - 1)];
    return v;
  };
  auto mask4 = [&](const float4 &v, int64_t row, int col0, int ncols) -> float4 {   // rows beyond the split, columns beyond the matrix: zeros
    const bool in = row < m_end;
    return make_float4(in && col0 + 0 < ncols ? v.x : 0.f, in && col0 + 1 < ncols ? v.y : 0.f,
                       in && col0 + 2 < ncols ? v.z : 0.f, in && col0 + 3 < ncols ? v.w : 0.f);
  };
  // two register images (stages s + 1 and s + 2): a stage's global loads get two MFMA phases to land
  float4 rg0, rx0, rg1, rx1;
  auto fetch = [&](float4 &rg, float4 &rx, int64_t m0) {
    rg = load4(g, ldg, m0 + lr, n0 + c4 * 4, N, std::integral_constant<bool, GV>());
    rx = load4(x, ldx, m0 + lr, k0 + c4 * 4, K, std::integral_constant<bool, XV>());
  };
  // where this thread's four values go in a plane image: chunk c4 >> 1, its low or high 8 bytes
  const int st_off = lb_off(lr, c4 >> 1) + 8 * (c4 & 1);
  auto stage = [&](unsigned char *operand, const float4 &v) {
    lb_bf16x4 p0, p1, p2;
    __bf16 t0, t1, t2;
    split3(v.x, t0, t1, t2); p0[0] = t0; p1[0] = t1; p2[0] = t2;
    split3(v.y, t0, t1, t2); p0[1] = t0; p1[1] = t1; p2[1] = t2;
    split3(v.z, t0, t1, t2); p0[2] = t0; p1[2] = t1; p2[2] = t2;
    split3(v.w, t0, t1, t2); p0[3] = t0; p1[3] = t1; p2[3] = t2;
    *reinterpret_cast<lb_bf16x4 *>(operand + st_off) = p0;
    *reinterpret_cast<lb_bf16x4 *>(operand + LB_PLANE_BYTES + st_off) = p1;
    *reinterpret_cast<lb_bf16x4 *>(operand + 2 * LB_PLANE_BYTES + st_off) = p2;
  };
  // transposed-read addresses: rows 8 h + 0..3 and 8 h + 4..7; the n block of this wave, its two k blocks
  const int h = lane >> 5;
  const int ga0 = lb_tr_addr(lane, 8 * h, wm * 32), ga1 = lb_tr_addr(lane, 8 * h + 4, wm * 32);
  const int xa0 = lb_tr_addr(lane, 8 * h, wn * 64), xa1 = lb_tr_addr(lane, 8 * h + 4, wn * 64);
  const int xb0 = lb_tr_addr(lane, 8 * h, wn * 64 + 32), xb1 = lb_tr_addr(lane, 8 * h + 4, wn * 64 + 32);

  const int steps = m_end > m_begin ? (m_end - m_begin + LB_BM - 1) / LB_BM : 0;
  auto step = [&](float4 &rg, float4 &rx, int s) {
    unsigned char *sG = smem + (s & 1) * LB_STAGE_BYTES, *sX = sG + LB_OPERAND_BYTES;
    stage(sG, mask4(rg, m_begin + (int64_t)s * LB_BM + lr, n0 + c4 * 4, N));
    stage(sX, mask4(rx, m_begin + (int64_t)s * LB_BM + lr, k0 + c4 * 4, K));
    // stage s is written; every wave that arrives here has its reads of stage s - 1 behind it, so stage s + 1 (the buffer of
    // s - 1) may be written after this barrier while slower waves still read stage s
    ISG_WAIT(0xC07F);   // lgkmcnt(0): my LDS writes have landed (the loads of the next rows stay in flight)
    ISG_BARRIER();
    // unconditional (load4 clamps the row): with a branch around it the compiler could not count the loads in flight and would
    // wait for all of them where the next stage needs the older pair only
    fetch(rg, rx, m_begin + (int64_t)(s + 2) * LB_BM);
    lb_bf16x8 a[3], b0[3], b1[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      a[q] = lb_tr_read(sG + q * LB_PLANE_BYTES, ga0, ga1);
      b0[q] = lb_tr_read(sX + q * LB_PLANE_BYTES, xa0, xa1);
      b1[q] = lb_tr_read(sX + q * LB_PLANE_BYTES, xb0, xb1);
    }
    // the forward's six products, small terms first
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b0[2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b1[2], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b0[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b1[0], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b0[1], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b1[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b0[1], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b1[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b0[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b1[0], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b0[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b1[0], acc1, 0, 0, 0);
  };
  if (steps > 0) {
    fetch(rg0, rx0, m_begin);
    fetch(rg1, rx1, (int64_t)m_begin + LB_BM);
  }
  for (int s = 0; s < steps; s += 2) {   // stages in pairs: an odd count ends with a stage of zeros (mask4), which adds nothing
    step(rg0, rx0, s);
    step(rg1, rx1, s + 1);
  }
  // partial[z][n][k]; acc element r of a lane: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
  float *out = partial + (size_t)blockIdx.z * N * K;
  const int ac = lane & 31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (n < N) {
      const int ka = k0 + wn * 64 + ac, kb = ka + 32;
      if (ka < K) out[(size_t)n * K + ka] = acc0[r];
      if (kb < K) out[(size_t)n * K + kb] = acc1[r];
    }
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_linear_train_abi_version(void) { return ISG_LINEAR_TRAIN_ABI_VERSION; }

extern "C" int64_t isg_linear_bwd_prep_parts(int64_t M, int32_t N) {
  (void)N;
  int64_t p = (M + LP_MIN_ROWS - 1) / LP_MIN_ROWS;
  if (p > LP_MAX_PARTS) p = LP_MAX_PARTS;
  if (p < 1) p = 1;
  return p;
}

extern "C" int isg_linear_bwd_prep(const float *g, int32_t ldg, const float *saved, int32_t lds, int32_t mode, float *dz,
                                   int32_t lddz, float *db_part, int64_t M, int32_t N, void *stream) {
  if (M < 0 || N <= 0 || mode < 0 || mode > 2) return ISG_EINVAL;
  if (!g || (mode != 0 && !saved) || (!dz && !db_part)) return ISG_EINVAL;
  if (ldg < N || (mode != 0 && lds < N) || (dz && lddz < N)) return ISG_EINVAL;
  if (M >= (1ll << 31)) return ISG_EUNSUPPORTED;
  if (M == 0) return ISG_OK;
  const int64_t P = isg_linear_bwd_prep_parts(M, N);
  const int rows_per_wg = (int)((M + P - 1) / P);
  // float4 bodies: every tensor in play at the same offset from a 16-byte boundary, every pitch in play a multiple of 4
  const uintptr_t og = reinterpret_cast<uintptr_t>(g) & 15;
  bool vec = (ldg & 3) == 0;
  if (mode != 0) vec = vec && (lds & 3) == 0 && (reinterpret_cast<uintptr_t>(saved) & 15) == og;
  if (dz) vec = vec && (lddz & 3) == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == og;
  const int off = vec ? (int)(og >> 2) : 0;
  const int groups = (N + off + 3) >> 2;
  int tx_log2 = 0;
  while ((1 << tx_log2) < groups && tx_log2 < 8) ++tx_log2;
  hipStream_t st = as_stream(stream);
#define LP_LAUNCH(MODE_)                                                                                                \
  linear_bwd_prep_kernel<MODE_><<<(unsigned)P, LP_THREADS, 0, st>>>(g, ldg, saved, lds, dz, lddz, db_part, (int)M, N,  \
                                                                    rows_per_wg, tx_log2, off, vec ? 1 : 0)
  if (mode == 0) LP_LAUNCH(0);
  else if (mode == 1) LP_LAUNCH(1);
  else LP_LAUNCH(2);
#undef LP_LAUNCH
  return check_launch();
}

extern "C" int64_t isg_linear_wgrad_bf16x6_splits(int64_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int64_t tiles = (int64_t)((N + LB_T - 1) / LB_T) * ((K + LB_T - 1) / LB_T);
  const char *env = getenv("ISG_WGRAD_BF16_WGS");         // tuning switch: total workgroups aimed at
  // two resident rounds (256 CUs x 2 workgroups x 2): measured against 256 and 512 at the training step's seven shapes, 1024 is
  // 8 - 13 % faster than 512 at the five shapes whose tiles do not fill a round evenly and within 1 % at the other two
  const int64_t target = env ? atoll(env) : 1024;
  int64_t s = (target + tiles - 1) / tiles;
  const int64_t by_rows = (M + 255) / 256;                // at least 256 rows per split
  if (s > by_rows) s = by_rows;
  if (s < 1) s = 1;
  if (s > 65535) s = 65535;
  return s;
}

extern "C" int isg_linear_wgrad_bf16x6(const float *grad_out, const float *x, float *partial, int64_t M, int32_t N, int32_t K,
                                       int32_t ldg, int32_t ldx, int64_t splits, void *stream) {
  if (M < 0 || N <= 0 || K <= 0 || ldg < N || ldx < K || splits <= 0) return ISG_EINVAL;
  if (!grad_out || !x || !partial) return ISG_EINVAL;
  if (M >= (1ll << 31) || splits > 65535 || (N + LB_T - 1) / LB_T > 65535 || (K + LB_T - 1) / LB_T > 65535)
    return ISG_EUNSUPPORTED;
  int64_t rows = (M + splits - 1) / splits;
  rows = (rows + LB_BM - 1) / LB_BM * LB_BM;
  if (rows < LB_BM) rows = LB_BM;
  dim3 grid((unsigned)((N + LB_T - 1) / LB_T), (unsigned)((K + LB_T - 1) / LB_T), (unsigned)splits), block(512);
  const bool gv = (ldg & 3) == 0 && (N & 3) == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0;
  const bool xv = (ldx & 3) == 0 && (K & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#define LB_LAUNCH(GV_, XV_)                                                                                             \
  wgrad_bf16x6_kernel<GV_, XV_><<<grid, block, 0, as_stream(stream)>>>(grad_out, x, partial, (int)M, N, K, ldg, ldx, (int)rows)
  if (gv && xv) LB_LAUNCH(true, true);
  else if (gv) LB_LAUNCH(true, false);
  else if (xv) LB_LAUNCH(false, true);
  else LB_LAUNCH(false, false);
#undef LB_LAUNCH
  return check_launch();
}
