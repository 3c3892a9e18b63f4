// Training of the question side (include/isg_train.h): dropout that a backward regenerates from (seed, position), the
// short-sequence attention with dropout on its probabilities and its backward, add + LayerNorm with dropout on the sublayer's
// result and its backward.  nn.TransformerEncoderLayer / DecoderLayer put a dropout on the attention probabilities, one in front
// of every residual add and one behind the FFN's ReLU (ISubGVQA/models/isubgvqa.py:133,156 train them at 0.1); none of the masks
// is stored here: every kernel draws element (i, j) of its operand from Philox block (i, j >> 2), word j & 3, and the backward
// draws it again.  No atomics in global memory anywhere: sums over rows run inside one workgroup in ascending order, or leave as
// one partial row per workgroup.
#include "isg_common.hpp"
#include "../../include/isg_train.h"

namespace isg {

// The four words of the block that holds elements (i, 4 jq .. 4 jq + 3): Philox::draw's counter and key schedule, all of c[].
__device__ __forceinline__ void philox_draw4(uint64_t seed, uint32_t i, uint32_t jq, uint32_t (&c)[4]) {
  c[0] = i; c[1] = jq; c[2] = 0x1571u; c[3] = 0x9E37u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    Philox::round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
__device__ __forceinline__ float keep_factor(uint32_t word, float p, float inv) {
  return (float)(word >> 8) * (1.0f / 16777216.0f) >= p ? inv : 0.f;
}
// keep / (1 - p) of the four elements of one block (p > 0)
__device__ __forceinline__ float4 keep4(uint64_t seed, uint32_t i, uint32_t jq, float p, float inv) {
  uint32_t c[4];
  philox_draw4(seed, i, jq, c);
  return make_float4(keep_factor(c[0], p, inv), keep_factor(c[1], p, inv), keep_factor(c[2], p, inv), keep_factor(c[3], p, inv));
}
// ... of one element (the attention strips: lane = key)
__device__ __forceinline__ float keep1(uint64_t seed, uint32_t i, uint32_t j, float p, float inv) {
  uint32_t c[4];
  philox_draw4(seed, i, j >> 2, c);
  const uint32_t lo = (j & 1) ? c[1] : c[0], hi = (j & 1) ? c[3] : c[2];
  return keep_factor((j & 2) ? hi : lo, p, inv);
}
// a dropped element is 0 whatever it held (not x * 0: an infinity would leave a NaN)
__device__ __forceinline__ float dropped(float x, float f) { return f != 0.f ? x * f : 0.f; }

// ---- dropout --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_kernel(const float *__restrict__ x, float *__restrict__ out, int64_t M, int nv,
                                                      int ldx, int ldo, float p, float inv, uint64_t seed) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * nv) return;
  const int64_t row = idx / nv;
  const int c = (int)(idx - row * nv);
  float4 t = reinterpret_cast<const float4 *>(x + row * ldx)[c];
  if (p > 0.f) {
    const float4 f = keep4(seed, (uint32_t)row, (uint32_t)c, p, inv);
    t.x = dropped(t.x, f.x); t.y = dropped(t.y, f.y); t.z = dropped(t.z, f.z); t.w = dropped(t.w, f.w);
  }
  reinterpret_cast<float4 *>(out + row * ldo)[c] = t;
}

// ---- attention ------------------------------------------------------------------------------------------------------------
// One query row's probabilities, a wave: mha_small_kernel's arithmetic (csrc/isg_attn.hip), statement for statement -- PARTS lanes
// share a key's dot product over interleaved float4 slices of the head, combined by the DPP butterfly; scale, bias, wave max,
// libm expf, wave sum, IEEE divide.  P is left in pw[0 .. Tk) and returned: p0 = P[lane], p1 = P[64 + lane] (0 beyond Tk).
template <int PARTS>
__device__ __forceinline__ void softmax_row(const float *qw, const float *Ks, int kp, int hd, int Tk, float scale,
                                            const float *bias, float *pw, int lane, float &p0, float &p1) {
  constexpr int KPL = 64 / PARTS;
  const int part = lane % PARTS, kslot = lane / PARTS;
  float mx = -INFINITY;
  for (int s0 = 0; s0 < Tk; s0 += KPL) {
    const int s = s0 + kslot;
    float dot = 0.f;
    if (s < Tk) {
      const float *kr = Ks + s * kp;
      for (int c = part * 4; c < hd; c += 4 * PARTS) {
        const float4 qv = *reinterpret_cast<const float4 *>(qw + c), kv = *reinterpret_cast<const float4 *>(kr + c);
        dot = fmaf(qv.x, kv.x, dot); dot = fmaf(qv.y, kv.y, dot); dot = fmaf(qv.z, kv.z, dot); dot = fmaf(qv.w, kv.w, dot);
      }
    }
    if (PARTS >= 2) dot += dpp_mov<ISG_DPP_XOR1>(dot);
    if (PARTS >= 4) dot += dpp_mov<ISG_DPP_XOR2>(dot);
    if (s < Tk && part == 0) {
      dot *= scale;
      if (bias) dot += bias[s];
      pw[s] = dot;
      mx = fmaxf(mx, dot);
    }
  }
  mx = wave_max(mx);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float e0 = 0.f, e1 = 0.f;
  if (lane < Tk) e0 = expf(pw[lane] - mx);
  if (64 + lane < Tk) e1 = expf(pw[64 + lane] - mx);
  const float den = wave_sum(e0 + e1);
  __builtin_amdgcn_wave_barrier();
  p0 = p1 = 0.f;
  if (lane < Tk) pw[lane] = p0 = e0 / den;
  if (64 + lane < Tk) pw[64 + lane] = p1 = e1 / den;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// out[s] = <a, R[s]> for the Tk rows of R (row stride kp), the same lane assignment: dP~[t, s] = <dO[t], V[s]>
template <int PARTS>
__device__ __forceinline__ void row_dots(const float *aw, const float *Rs, int kp, int hd, int Tk, float *out, int lane) {
  constexpr int KPL = 64 / PARTS;
  const int part = lane % PARTS, kslot = lane / PARTS;
  for (int s0 = 0; s0 < Tk; s0 += KPL) {
    const int s = s0 + kslot;
    float dot = 0.f;
    if (s < Tk) {
      const float *rr = Rs + s * kp;
      for (int c = part * 4; c < hd; c += 4 * PARTS) {
        const float4 av = *reinterpret_cast<const float4 *>(aw + c), rv = *reinterpret_cast<const float4 *>(rr + c);
        dot = fmaf(av.x, rv.x, dot); dot = fmaf(av.y, rv.y, dot); dot = fmaf(av.z, rv.z, dot); dot = fmaf(av.w, rv.w, dot);
      }
    }
    if (PARTS >= 2) dot += dpp_mov<ISG_DPP_XOR1>(dot);
    if (PARTS >= 4) dot += dpp_mov<ISG_DPP_XOR2>(dot);
    if (s < Tk && part == 0) out[s] = dot;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct MhaTrainArgs {
  const float *q, *k, *v, *key_bias;      // key_bias [B, Tk] or NULL
  const float *d_out;                     // backward only (NULL in the forward)
  float *out;                             // forward only (NULL in the backward)
  float *d_q, *d_k, *d_v;                 // backward only (NULL in the forward)
  int B, H, hd, Tq, Tk, ldq, ldk, ldv, ldo, lddq, lddk, lddv;
  float scale, p, inv;
  uint64_t seed;
};

// rows [T][hd] of one head of a [T*B, ld] operand (row t * B + b) into LDS rows of stride `rs`
__device__ __forceinline__ void stage_rows(float *dst, int rs, const float *src, int ld, int T, int h4, int B, int b, int col0,
                                           int tid, int nt) {
  for (int idx = tid; idx < T * h4; idx += nt) {
    const int t = idx / h4, c = idx - t * h4;
    *reinterpret_cast<float4 *>(dst + t * rs + 4 * c) =
        *reinterpret_cast<const float4 *>(src + ((size_t)t * B + b) * ld + col0 + 4 * c);
  }
}

// Forward with dropout on the probabilities: one workgroup per (batch item, head), a wave per query row.
template <int PARTS>
__global__ __launch_bounds__(256) void mha_small_train_kernel(MhaTrainArgs a) {
  extern __shared__ float smem[];
  const int hd = a.hd, Tk = a.Tk, Tq = a.Tq, kp = hd + 4, h4 = hd >> 2;
  float *Ks = smem;                        // [Tk][hd + 4]
  float *Vs = Ks + (size_t)Tk * kp;        // [Tk][hd]
  float *Qs = Vs + (size_t)Tk * hd;        // [Tq][hd]
  float *ps = Qs + (size_t)Tq * hd;        // [4][128]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H, col0 = h * hd;
  stage_rows(Ks, kp, a.k, a.ldk, Tk, h4, a.B, b, col0, tid, 256);
  stage_rows(Vs, hd, a.v, a.ldv, Tk, h4, a.B, b, col0, tid, 256);
  stage_rows(Qs, hd, a.q, a.ldq, Tq, h4, a.B, b, col0, tid, 256);
  __syncthreads();
  float *pw = ps + wave * 128;
  const float *bias = a.key_bias ? a.key_bias + (size_t)b * Tk : nullptr;
  for (int tq = wave; tq < Tq; tq += 4) {
    float p0, p1;
    softmax_row<PARTS>(Qs + tq * hd, Ks, kp, hd, Tk, a.scale, bias, pw, lane, p0, p1);
    const uint32_t i = (uint32_t)blockIdx.x * (uint32_t)Tq + (uint32_t)tq;
    if (lane < Tk) pw[lane] = dropped(p0, keep1(a.seed, i, (uint32_t)lane, a.p, a.inv));
    if (64 + lane < Tk) pw[64 + lane] = dropped(p1, keep1(a.seed, i, (uint32_t)(64 + lane), a.p, a.inv));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < hd) {
      float o = 0.f;
      for (int s = 0; s < Tk; ++s) o = fmaf(pw[s], Vs[s * hd + lane], o);
      a.out[((size_t)tq * a.B + b) * a.ldo + col0 + lane] = o;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// Backward: one workgroup per (batch item, head); Q, K, V, dO and the [Tq][Tk] strips of P~ and dS in LDS.
//   phase one, a wave per query row t:  P (softmax_row), dP~ = <dO[t], V[s]>, dP = dP~ keep / (1 - p), dS = P (dP - sum_s P dP),
//              dQ[t] = scale sum_s dS[t, s] K[s] (lane = channel);  the strips keep P~ = P keep / (1 - p) and dS
//   phase two, a wave per key s, lane = channel:  dV[s] = sum_t P~[t, s] dO[t],  dK[s] = scale sum_t dS[t, s] Q[t], t ascending
// K and V rows are padded by a float4 (lane = key reads down a column); lane = channel reads are consecutive floats.
template <int PARTS>
__global__ __launch_bounds__(256) void mha_small_bwd_kernel(MhaTrainArgs a) {
  extern __shared__ float smem[];
  const int hd = a.hd, Tk = a.Tk, Tq = a.Tq, kp = hd + 4, h4 = hd >> 2;
  float *Ks = smem;                        // [Tk][hd + 4]
  float *Vs = Ks + (size_t)Tk * kp;        // [Tk][hd + 4]
  float *Qs = Vs + (size_t)Tk * kp;        // [Tq][hd]
  float *Gs = Qs + (size_t)Tq * hd;        // [Tq][hd]   dO
  float *Pt = Gs + (size_t)Tq * hd;        // [Tq][Tk]   P, then P~
  float *Ds = Pt + (size_t)Tq * Tk;        // [Tq][Tk]   dP~, then dS
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H, col0 = h * hd;
  stage_rows(Ks, kp, a.k, a.ldk, Tk, h4, a.B, b, col0, tid, 256);
  stage_rows(Vs, kp, a.v, a.ldv, Tk, h4, a.B, b, col0, tid, 256);
  stage_rows(Qs, hd, a.q, a.ldq, Tq, h4, a.B, b, col0, tid, 256);
  stage_rows(Gs, hd, a.d_out, a.ldo, Tq, h4, a.B, b, col0, tid, 256);
  __syncthreads();
  const float *bias = a.key_bias ? a.key_bias + (size_t)b * Tk : nullptr;
  for (int tq = wave; tq < Tq; tq += 4) {
    float *pw = Pt + (size_t)tq * Tk, *dw = Ds + (size_t)tq * Tk;
    float p0, p1;
    softmax_row<PARTS>(Qs + tq * hd, Ks, kp, hd, Tk, a.scale, bias, pw, lane, p0, p1);
    row_dots<PARTS>(Gs + tq * hd, Vs, kp, hd, Tk, dw, lane);
    float f0 = 1.f, f1 = 1.f, dp0 = 0.f, dp1 = 0.f;
    if (a.p > 0.f) {
      const uint32_t i = (uint32_t)blockIdx.x * (uint32_t)Tq + (uint32_t)tq;
      if (lane < Tk) f0 = keep1(a.seed, i, (uint32_t)lane, a.p, a.inv);
      if (64 + lane < Tk) f1 = keep1(a.seed, i, (uint32_t)(64 + lane), a.p, a.inv);
    }
    if (lane < Tk) dp0 = dropped(dw[lane], f0);
    if (64 + lane < Tk) dp1 = dropped(dw[64 + lane], f1);
    // a key without weight (bias -inf) takes no part, whatever its V holds
    const float w0 = p0 != 0.f ? p0 * dp0 : 0.f, w1 = p1 != 0.f ? p1 * dp1 : 0.f;
    const float rs = wave_sum(w0 + w1);
    __builtin_amdgcn_wave_barrier();
    if (lane < Tk) {
      dw[lane] = p0 != 0.f ? p0 * (dp0 - rs) : 0.f;
      pw[lane] = dropped(p0, f0);
    }
    if (64 + lane < Tk) {
      dw[64 + lane] = p1 != 0.f ? p1 * (dp1 - rs) : 0.f;
      pw[64 + lane] = dropped(p1, f1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < hd) {
      float g = 0.f;
      for (int s = 0; s < Tk; ++s) g = fmaf(dw[s], Ks[s * kp + lane], g);
      a.d_q[((size_t)tq * a.B + b) * a.lddq + col0 + lane] = g * a.scale;
    }
  }
  __syncthreads();
  for (int s = wave; s < Tk; s += 4) {
    if (lane < hd) {
      float gv = 0.f, gk = 0.f;
      for (int t = 0; t < Tq; ++t) {
        gv = fmaf(Pt[t * Tk + s], Gs[t * hd + lane], gv);
        gk = fmaf(Ds[t * Tk + s], Qs[t * hd + lane], gk);
      }
      const size_t row = (size_t)s * a.B + b;
      a.d_v[row * a.lddv + col0 + lane] = gv;
      a.d_k[row * a.lddk + col0 + lane] = gk * a.scale;
    }
  }
}

// ---- add + LayerNorm ------------------------------------------------------------------------------------------------------
// One row into registers, as add_layernorm_kernel (csrc/isg_attn.hip) does it: v = r + dropout(x), the mean, the residue of the
// centred values, the variance.  On return v holds v - mean - residue; `keep` the factors of x (p > 0 only).
template <int NV>
__device__ __forceinline__ float ln_row_stats(const float *__restrict__ xr, const float *__restrict__ rr, int nv, int D, int lane,
                                              uint32_t row, float p, float inv, uint64_t seed, float eps, float4 (&v)[NV],
                                              float4 (&keep)[NV]) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    keep[i] = make_float4(1.f, 1.f, 1.f, 1.f);
    if (c < nv) {
      v[i] = reinterpret_cast<const float4 *>(xr)[c];
      if (p > 0.f) {
        keep[i] = keep4(seed, row, (uint32_t)c, p, inv);
        v[i].x = dropped(v[i].x, keep[i].x); v[i].y = dropped(v[i].y, keep[i].y);
        v[i].z = dropped(v[i].z, keep[i].z); v[i].w = dropped(v[i].w, keep[i].w);
      }
      if (rr) {
        const float4 t = reinterpret_cast<const float4 *>(rr)[c];
        v[i].x += t.x; v[i].y += t.y; v[i].z += t.z; v[i].w += t.w;
      }
      sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float mean = wave_sum(sum) / (float)D;
  float res = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (lane + 64 * i < nv) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      res += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  res = wave_sum(res) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (lane + 64 * i < nv) {
      v[i].x -= res; v[i].y -= res; v[i].z -= res; v[i].w -= res;
      sq += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  }
  return 1.0f / sqrtf(wave_sum(sq) / (float)D + eps);
}

template <int NV>
__global__ __launch_bounds__(256) void dropout_add_layernorm_kernel(const float *__restrict__ x, const float *__restrict__ r,
                                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                    float eps, float *__restrict__ out, int M, int D, int ldx,
                                                                    int ldr, int ldo, float p, float inv, uint64_t seed) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const int nv = D >> 2;
  float4 v[NV], keep[NV];
  const float rstd = ln_row_stats<NV>(x + (int64_t)row * ldx, r ? r + (int64_t)row * ldr : nullptr, nv, D, lane, (uint32_t)row, p,
                                      inv, seed, eps, v, keep);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) {
      const float4 g = reinterpret_cast<const float4 *>(gamma)[c];
      const float4 bb = beta ? reinterpret_cast<const float4 *>(beta)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 o;
      o.x = v[i].x * rstd * g.x + bb.x;
      o.y = v[i].y * rstd * g.y + bb.y;
      o.z = v[i].z * rstd * g.z + bb.z;
      o.w = v[i].w * rstd * g.w + bb.w;
      reinterpret_cast<float4 *>(out + (int64_t)row * ldo)[c] = o;
    }
  }
}

// Backward: a wave per row, the rows of a workgroup's four waves strided over the grid; d_gamma / d_beta accumulate in registers
// over a wave's rows (ascending), the four waves' sums meet in LDS in wave order, and the workgroup writes ONE partial row.
template <int NV>
__global__ __launch_bounds__(256) void add_layernorm_bwd_kernel(const float *__restrict__ x, const float *__restrict__ r,
                                                                const float *__restrict__ gamma, float eps,
                                                                const float *__restrict__ d_out, float *__restrict__ d_x,
                                                                float *__restrict__ d_r, float *__restrict__ dg_part,
                                                                float *__restrict__ db_part, int M, int D, int ldx, int ldr,
                                                                int lddo, int lddx, int lddr, float p, float inv, uint64_t seed) {
  extern __shared__ float smem[];           // [3][D]: the sums of waves 1 .. 3
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nv = D >> 2;
  float4 dg[NV], db[NV], gm[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    dg[i] = db[i] = gm[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane + 64 * i < nv) gm[i] = reinterpret_cast<const float4 *>(gamma)[lane + 64 * i];
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
    float4 v[NV], keep[NV], go[NV];
    const float rstd = ln_row_stats<NV>(x + row * ldx, r ? r + row * ldr : nullptr, nv, D, lane, (uint32_t)row, p, inv, seed, eps,
                                        v, keep);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      go[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < nv) {
        go[i] = reinterpret_cast<const float4 *>(d_out + row * lddo)[c];
        v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;          // xhat
        dg[i].x += go[i].x * v[i].x; dg[i].y += go[i].y * v[i].y; dg[i].z += go[i].z * v[i].z; dg[i].w += go[i].w * v[i].w;
        db[i].x += go[i].x; db[i].y += go[i].y; db[i].z += go[i].z; db[i].w += go[i].w;
        go[i].x *= gm[i].x; go[i].y *= gm[i].y; go[i].z *= gm[i].z; go[i].w *= gm[i].w;      // g = d_out * gamma
        s1 += (go[i].x + go[i].y) + (go[i].z + go[i].w);
        s2 += (go[i].x * v[i].x + go[i].y * v[i].y) + (go[i].z * v[i].z + go[i].w * v[i].w);
      }
    }
    const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        float4 dv;
        dv.x = rstd * ((go[i].x - m1) - v[i].x * m2);
        dv.y = rstd * ((go[i].y - m1) - v[i].y * m2);
        dv.z = rstd * ((go[i].z - m1) - v[i].z * m2);
        dv.w = rstd * ((go[i].w - m1) - v[i].w * m2);
        if (d_r) reinterpret_cast<float4 *>(d_r + row * lddr)[c] = dv;
        if (p > 0.f) {
          dv.x = dropped(dv.x, keep[i].x); dv.y = dropped(dv.y, keep[i].y);
          dv.z = dropped(dv.z, keep[i].z); dv.w = dropped(dv.w, keep[i].w);
        }
        reinterpret_cast<float4 *>(d_x + row * lddx)[c] = dv;
      }
    }
  }
  // gamma's partial row, then beta's through the same LDS
  for (int pass = 0; pass < 2; ++pass) {
    float *part = pass == 0 ? dg_part : db_part;
    if (!part) continue;                    // uniform over the workgroup
    if (pass == 1) __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (lane + 64 * i < nv) reinterpret_cast<float4 *>(smem + (size_t)(wave - 1) * D)[lane + 64 * i] = pass == 0 ? dg[i] : db[i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
          float4 t = pass == 0 ? dg[i] : db[i];
#pragma unroll
          for (int w = 0; w < 3; ++w) {
            const float4 u = reinterpret_cast<const float4 *>(smem + (size_t)w * D)[c];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
          }
          reinterpret_cast<float4 *>(part + (size_t)blockIdx.x * D)[c] = t;
        }
      }
    }
  }
}

static inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static inline int mha_parts(int hd, int Tk) { return Tk <= 16 && (hd & 15) == 0 ? 4 : Tk <= 32 && (hd & 7) == 0 ? 2 : 1; }
static inline int64_t mha_bwd_lds(int hd, int Tq, int Tk) {
  return 4ll * (2ll * Tk * (hd + 4) + 2ll * Tq * hd + 2ll * Tq * Tk);
}
constexpr int64_t MHA_BWD_LDS_MAX = 160 * 1024;       // gfx950: LDS of a CU, one workgroup may hold all of it
constexpr int LN_BWD_ROWS_PER_PART = 16, LN_BWD_PARTS_MAX = 1024;

}  // namespace isg

using namespace isg;

extern "C" int isg_train_abi_version(void) { return ISG_TRAIN_ABI_VERSION; }

extern "C" int isg_dropout(const float *x, int32_t ldx, float *out, int32_t ldo, int64_t M, int32_t D, float p, uint64_t seed,
                           void *stream) {
  if (M < 0 || D <= 0 || ldx < D || ldo < D || !(p >= 0.f && p < 1.f)) return ISG_EINVAL;
  if (M == 0) return ISG_OK;
  if (!x || !out) return ISG_EINVAL;
  const int64_t n = M * (D >> 2);
  if ((D & 3) || (ldx & 3) || (ldo & 3) || misaligned(x) || misaligned(out) || M >= (1ll << 31) || (n + 255) / 256 >= (1ll << 31))
    return ISG_EUNSUPPORTED;
  dropout_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(x, out, M, D >> 2, ldx, ldo, p, 1.0f / (1.0f - p), seed);
  return check_launch();
}

extern "C" int isg_mha_small_train(const float *q, int32_t ldq, const float *k, int32_t ldk, const float *v, int32_t ldv,
                                   const float *key_bias, float *out, int32_t ldo, int64_t B, int32_t H, int32_t hd, int32_t Tq,
                                   int32_t Tk, float p, uint64_t seed, void *stream) {
  if (!(p >= 0.f && p < 1.f)) return ISG_EINVAL;
  if (p == 0.f)       // nothing is drawn: the inference kernel, bit for bit
    return isg_mha_small(q, ldq, k, ldk, v, ldv, key_bias, out, ldo, nullptr, B, H, hd, Tq, Tk, nullptr, nullptr, stream);
  if (B < 0 || H <= 0 || hd <= 0 || Tq < 0 || Tk <= 0) return ISG_EINVAL;
  if (B == 0 || Tq == 0) return ISG_OK;
  if (!q || !k || !v || !out) return ISG_EINVAL;
  if (hd > 64 || Tk > 128 || B * H >= (1ll << 31) || B * H * Tq >= (1ll << 32)) return ISG_EUNSUPPORTED;
  if (ldq < H * hd || ldk < H * hd || ldv < H * hd || ldo < H * hd) return ISG_EINVAL;
  if ((hd & 3) || (ldq & 3) || (ldk & 3) || (ldv & 3) || misaligned(q) || misaligned(k) || misaligned(v)) return ISG_EUNSUPPORTED;
  const size_t lds = ((size_t)Tk * (2 * hd + 4) + (size_t)Tq * hd + 4 * 128) * sizeof(float);
  if (lds > 64 * 1024) return ISG_EUNSUPPORTED;
  MhaTrainArgs a{q, k, v, key_bias, nullptr, out, nullptr, nullptr, nullptr, (int)B, H, hd, Tq, Tk, ldq, ldk, ldv, ldo, 0, 0, 0,
                 (float)(1.0 / sqrt((double)hd)), p, 1.0f / (1.0f - p), seed};
  const unsigned grid = (unsigned)(B * H);
  hipStream_t st = as_stream(stream);
  const int parts = mha_parts(hd, Tk);
  if (parts == 4) mha_small_train_kernel<4><<<grid, 256, lds, st>>>(a);
  else if (parts == 2) mha_small_train_kernel<2><<<grid, 256, lds, st>>>(a);
  else mha_small_train_kernel<1><<<grid, 256, lds, st>>>(a);
  return check_launch();
}

extern "C" int64_t isg_mha_small_bwd_lds_bytes(int32_t hd, int32_t Tq, int32_t Tk) {
  return hd <= 0 || Tq < 0 || Tk < 0 ? 0 : mha_bwd_lds(hd, Tq, Tk);
}

extern "C" int isg_mha_small_bwd(const float *q, int32_t ldq, const float *k, int32_t ldk, const float *v, int32_t ldv,
                                 const float *key_bias, const float *d_out, int32_t lddo, float *d_q, int32_t lddq, float *d_k,
                                 int32_t lddk, float *d_v, int32_t lddv, int64_t B, int32_t H, int32_t hd, int32_t Tq, int32_t Tk,
                                 float p, uint64_t seed, void *stream) {
  if (B < 0 || H <= 0 || hd <= 0 || Tq < 0 || Tk <= 0 || !(p >= 0.f && p < 1.f)) return ISG_EINVAL;
  if (B == 0) return ISG_OK;
  if (!k || !v || !d_k || !d_v || (Tq > 0 && (!q || !d_out || !d_q))) return ISG_EINVAL;
  if (hd > 64 || Tk > 128 || B * H >= (1ll << 31) || B * H * Tq >= (1ll << 32)) return ISG_EUNSUPPORTED;
  const int D = H * hd;
  if (ldq < D || ldk < D || ldv < D || lddo < D || lddq < D || lddk < D || lddv < D) return ISG_EINVAL;
  if ((hd & 3) || (ldq & 3) || (ldk & 3) || (ldv & 3) || (lddo & 3) || misaligned(q) || misaligned(k) || misaligned(v) ||
      misaligned(d_out))
    return ISG_EUNSUPPORTED;
  // the forward's limit too: a shape the forward refuses has no backward here
  if (((size_t)Tk * (2 * hd + 4) + (size_t)Tq * hd + 4 * 128) * sizeof(float) > 64 * 1024) return ISG_EUNSUPPORTED;
  const int64_t lds = mha_bwd_lds(hd, Tq, Tk);
  if (lds > MHA_BWD_LDS_MAX) return ISG_EUNSUPPORTED;
  MhaTrainArgs a{q, k, v, key_bias, d_out, nullptr, d_q, d_k, d_v, (int)B, H, hd, Tq, Tk, ldq, ldk, ldv, lddo, lddq, lddk, lddv,
                 (float)(1.0 / sqrt((double)hd)), p, 1.0f / (1.0f - p), seed};
  const unsigned grid = (unsigned)(B * H);
  hipStream_t st = as_stream(stream);
  const int parts = mha_parts(hd, Tk);
#define ISG_MHA_BWD(P_)                                                                                            \
  do {                                                                                                             \
    if (lds > 64 * 1024 && !dyn_lds_ok<&mha_small_bwd_kernel<P_>>((int)lds)) return ISG_EUNSUPPORTED;              \
    mha_small_bwd_kernel<P_><<<grid, 256, (size_t)lds, st>>>(a);                                                   \
  } while (0)
  if (parts == 4) ISG_MHA_BWD(4);
  else if (parts == 2) ISG_MHA_BWD(2);
  else ISG_MHA_BWD(1);
#undef ISG_MHA_BWD
  return check_launch();
}

extern "C" int isg_dropout_add_layernorm(const float *x, int32_t ldx, const float *r, int32_t ldr, const float *gamma,
                                         const float *beta, float eps, float *out, int32_t ldo, int64_t M, int32_t D, float p,
                                         uint64_t seed, void *stream) {
  if (!(p >= 0.f && p < 1.f)) return ISG_EINVAL;
  if (p == 0.f)       // nothing is drawn: the inference kernel, bit for bit
    return isg_add_layernorm(x, ldx, r, ldr, gamma, beta, eps, out, ldo, nullptr, M, D, nullptr, nullptr, stream);
  if (M < 0 || D <= 0 || ldx < D || ldo < D || (r && ldr < D)) return ISG_EINVAL;
  if (M == 0) return ISG_OK;
  if (!x || !gamma || !out) return ISG_EINVAL;
  if ((D & 3) || D > 2048 || (ldx & 3) || (ldo & 3) || (r && (ldr & 3)) || misaligned(x) || misaligned(out) || (r && misaligned(r)) ||
      misaligned(gamma) || (beta && misaligned(beta)) || M >= (1ll << 31))
    return ISG_EUNSUPPORTED;
  const unsigned grid = (unsigned)((M + 3) / 4);
  hipStream_t st = as_stream(stream);
  const float inv = 1.0f / (1.0f - p);
#define ISG_DLN(NV_) dropout_add_layernorm_kernel<NV_><<<grid, 256, 0, st>>>(x, r, gamma, beta, eps, out, (int)M, D, ldx, ldr, ldo, p, inv, seed)
  if (D <= 256) ISG_DLN(1);
  else if (D <= 512) ISG_DLN(2);
  else if (D <= 1024) ISG_DLN(4);
  else ISG_DLN(8);
#undef ISG_DLN
  return check_launch();
}

extern "C" int32_t isg_add_layernorm_bwd_parts(int64_t M) {
  if (M <= 0) return 0;
  const int64_t parts = (M + LN_BWD_ROWS_PER_PART - 1) / LN_BWD_ROWS_PER_PART;
  return (int32_t)(parts < LN_BWD_PARTS_MAX ? parts : LN_BWD_PARTS_MAX);
}

extern "C" int isg_add_layernorm_bwd(const float *x, int32_t ldx, const float *r, int32_t ldr, const float *gamma, float eps,
                                     const float *d_out, int32_t lddo, float *d_x, int32_t lddx, float *d_r, int32_t lddr,
                                     float *d_gamma_part, float *d_beta_part, int64_t M, int32_t D, float p, uint64_t seed,
                                     void *stream) {
  if (M < 0 || D <= 0 || ldx < D || lddo < D || lddx < D || (r && ldr < D) || (d_r && lddr < D) || !(p >= 0.f && p < 1.f))
    return ISG_EINVAL;
  if (M == 0) return ISG_OK;
  if (!x || !gamma || !d_out || !d_x || !d_gamma_part) return ISG_EINVAL;
  if ((D & 3) || D > 2048 || (ldx & 3) || (lddo & 3) || (lddx & 3) || (r && (ldr & 3)) || (d_r && (lddr & 3)) || misaligned(x) ||
      misaligned(d_out) || misaligned(d_x) || (r && misaligned(r)) || (d_r && misaligned(d_r)) || misaligned(gamma) ||
      misaligned(d_gamma_part) || (d_beta_part && misaligned(d_beta_part)) || M >= (1ll << 31))
    return ISG_EUNSUPPORTED;
  const unsigned grid = (unsigned)isg_add_layernorm_bwd_parts(M);
  const size_t lds = (size_t)3 * D * sizeof(float);
  hipStream_t st = as_stream(stream);
  const float inv = 1.0f / (1.0f - p);
#define ISG_LNB(NV_)                                                                                               \
  add_layernorm_bwd_kernel<NV_><<<grid, 256, lds, st>>>(x, r, gamma, eps, d_out, d_x, d_r, d_gamma_part, d_beta_part, (int)M, D, ldx, \
                                                        ldr, lddo, lddx, lddr, p, inv, seed)
  if (D <= 256) ISG_LNB(1);
  else if (D <= 512) ISG_LNB(2);
  else if (D <= 1024) ISG_LNB(4);
  else ISG_LNB(8);
#undef ISG_LNB
  return check_launch();
}
