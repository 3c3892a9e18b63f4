// Training of the scene-graph encoder without its concatenations (include/isg_sgenc_train.h; forward: csrc/isg_sgenc.hip).
//
// The forward replaced a Linear over cat([x[row], x[col], e]) by gathers of rows projected once per node / per token.  The
// backward of a gather is a scatter: d A[i] is the sum of dz over the edges that read row i.  All three scatters of a gather-add
// (by source, by destination, by token), and the one of the node tokens' embedding sum, are the SAME operation over different
// CSRs, so there is one kernel for it, isg_segment_rows_sum, without atomics.
//
// The segments are badly skewed: one relation or the pad token owns tens of thousands of entries, the median segment a handful.
// A wave per segment would run as long as its longest list, so the SLOT range is cut, not the segment list: a group of sixteen
// lanes walks SEG_CHUNK consecutive slots (finding its first segment by bisecting rowptr), stores the segments that end AND
// begin inside its piece, and leaves at most two partial rows in the workspace -- slot 0: the run that continues a segment
// begun in an earlier piece, slot 1: the run that begins a segment which goes on into the next piece.  A second launch over the
// segments writes zeros for the empty (and the skipped) ones and adds a crossing segment's partial rows in piece order.
// Sixteen lanes per row: C = 300 is 75 float4, five passes of sixteen lanes (the lane map of gather_add_planes32_kernel).
#include "isg_sgenc.hpp"

#include "../../include/isg_sgenc_train.h"

namespace isg {

constexpr int SEG_CHUNK = 256;    // slots per piece (isg_segment_rows_chunk)
constexpr int SEG_PASSES = 5;     // float4 per lane and column block: 16 * 5 float4 = 320 channels per walk of a piece
constexpr int SEG_U = 4;          // rows in flight per group

__device__ __forceinline__ void f4_add(float4 &a, const float4 &g) {
  a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
}
__device__ __forceinline__ void f4_fma(float4 &a, float s, const float4 &g) {
  a.x = fmaf(s, g.x, a.x); a.y = fmaf(s, g.y, a.y); a.z = fmaf(s, g.z, a.z); a.w = fmaf(s, g.w, a.w);
}

// pass 1: one group of 16 lanes per piece of SEG_CHUNK slots
__global__ __launch_bounds__(256) void segment_rows_chunk_kernel(const int *__restrict__ rowptr, const int *__restrict__ eid,
                                                                 const float *__restrict__ w, const float4 *__restrict__ G,
                                                                 int ldg, int gdiv, float4 *__restrict__ out, int ldo,
                                                                 float4 *__restrict__ ws, int S, int M, int Q, int skip,
                                                                 int chunks) {
  const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  if (k >= chunks) return;
  const int t0 = k * SEG_CHUNK, t1 = min(t0 + SEG_CHUNK, M);
  int lo = 0, hi = S;               // rowptr[lo] <= t0 < rowptr[hi]  (rowptr[0] = 0, rowptr[S] = M > t0)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= t0) lo = mid; else hi = mid;
  }
  for (int cb = 0; cb < Q; cb += 16 * SEG_PASSES) {        // a row wider than 320 channels: the piece is walked again
    int s = lo, t = t0;
    while (t < t1 && s < S) {
      const int rb = rowptr[s], re = rowptr[s + 1];
      const int b = min(re, t1);
      if (b <= t) { ++s; continue; }                       // an empty segment
      const bool starts = t == rb, ends = b == re;
      if (s != skip) {
        float4 acc[SEG_PASSES];
#pragma unroll
        for (int p = 0; p < SEG_PASSES; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int u0 = t; u0 < b; u0 += SEG_U) {
          int id[SEG_U];
          float wv[SEG_U];
          float4 g[SEG_U][SEG_PASSES];
#pragma unroll
          for (int u = 0; u < SEG_U; ++u) {
            id[u] = eid[min(u0 + u, b - 1)];
            wv[u] = w ? w[id[u]] : 1.f;
          }
#pragma unroll
          for (int u = 0; u < SEG_U; ++u) {
            const float4 *row = G + (size_t)(id[u] / gdiv) * ldg;
#pragma unroll
            for (int p = 0; p < SEG_PASSES; ++p) {
              const int c = cb + l + 16 * p;
              g[u][p] = c < Q ? row[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
          }
#pragma unroll
          for (int u = 0; u < SEG_U; ++u) {
            if (u0 + u < b) {                              // slot order: row u is added before row u + 1
#pragma unroll
              for (int p = 0; p < SEG_PASSES; ++p) {
                if (w) f4_fma(acc[p], wv[u], g[u][p]); else f4_add(acc[p], g[u][p]);
              }
            }
          }
        }
        float4 *dst = starts && ends ? out + (size_t)s * ldo : ws + ((size_t)k * 2 + (starts ? 1 : 0)) * Q;
#pragma unroll
        for (int p = 0; p < SEG_PASSES; ++p) {
          const int c = cb + l + 16 * p;
          if (c < Q) dst[c] = acc[p];
        }
      }
      t = b;
      if (ends) ++s;
    }
  }
}

// pass 2: one group of 16 lanes per segment -- zeros, or the partial rows of a crossing segment in piece order
__global__ __launch_bounds__(256) void segment_rows_finish_kernel(const int *__restrict__ rowptr, float4 *__restrict__ out, int ldo,
                                                                  const float4 *__restrict__ ws, int S, int Q, int skip) {
  const int s = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  if (s >= S) return;
  const int rb = rowptr[s], re = rowptr[s + 1];
  float4 *dst = out + (size_t)s * ldo;
  if (re <= rb || s == skip) {
    for (int c = l; c < Q; c += 16) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int k0 = rb / SEG_CHUNK, k1 = (re - 1) / SEG_CHUNK;
  if (k0 == k1) return;                                     // pass 1 stored it
  for (int c = l; c < Q; c += 16) {
    float4 acc = ws[((size_t)k0 * 2 + 1) * Q + c];
    for (int k = k0 + 1; k <= k1; k += SEG_U) {
      float4 g[SEG_U];
#pragma unroll
      for (int u = 0; u < SEG_U; ++u) g[u] = ws[(size_t)min(k + u, k1) * 2 * Q + c];
#pragma unroll
      for (int u = 0; u < SEG_U; ++u)
        if (k + u <= k1) f4_add(acc, g[u]);
    }
    dst[c] = acc;
  }
}

// d/dt [0.5 t (1 + erf(t / sqrt 2))]: the formula of torch's gelu_backward and of csrc/isg_tail_bwd.hip
__device__ __forceinline__ float gelu_exact_grad(float t) {
  return 0.5f * (1.0f + erff(t * 0.70710678118654752440f)) + t * 0.3989422804014327f * expf(-0.5f * t * t);
}

constexpr int GAB_PARTS_MAX = 1024;

// dz = d_out * act'(z), z from the forward's gather_add_value with the activation taken off; a workgroup owns a contiguous range
// of rows, its sixteen groups take every sixteenth row of it and their column sums meet in LDS in group order
__global__ __launch_bounds__(256) void gather_add_bwd_kernel(GatherAddArgs a, const float4 *__restrict__ d_out, int lddo,
                                                             float4 *__restrict__ dz, int lddz, float4 *__restrict__ d_bias_part,
                                                             int act, int rows_per_block) {
  __shared__ float4 s_part[16][16 * SEG_PASSES];
  const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int64_t e0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t e1 = e0 + rows_per_block < a.E ? e0 + rows_per_block : a.E;
  for (int cb = 0; cb < a.Q; cb += 16 * SEG_PASSES) {
    float4 acc[SEG_PASSES];
#pragma unroll
    for (int p = 0; p < SEG_PASSES; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t e = e0 + grp; e < e1; e += 16) {
#pragma unroll
      for (int p = 0; p < SEG_PASSES; ++p) {
        const int c = cb + l + 16 * p;
        if (c >= a.Q) continue;
        float4 g = d_out[(size_t)e * lddo + c];
        if (act == 1) {
          const float4 z = gather_add_value(a, e, c);
          g.x *= gelu_exact_grad(z.x); g.y *= gelu_exact_grad(z.y); g.z *= gelu_exact_grad(z.z); g.w *= gelu_exact_grad(z.w);
        }
        dz[(size_t)e * lddz + c] = g;
        f4_add(acc[p], g);
      }
    }
    if (!d_bias_part) continue;                              // (uniform over the workgroup)
#pragma unroll
    for (int p = 0; p < SEG_PASSES; ++p) s_part[grp][l + 16 * p] = acc[p];
    __syncthreads();
    if (threadIdx.x < 16 * SEG_PASSES && cb + (int)threadIdx.x < a.Q) {
      float4 sum = s_part[0][threadIdx.x];
#pragma unroll
      for (int g = 1; g < 16; ++g) f4_add(sum, s_part[g][threadIdx.x]);
      d_bias_part[(size_t)blockIdx.x * a.Q + cb + threadIdx.x] = sum;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void scatter_mean_bwd_kernel(const float4 *__restrict__ d_out, int lddo, const int64_t *__restrict__ dst,
                                                               const int *__restrict__ rowptr, float4 *__restrict__ d_msg, int lddm,
                                                               int64_t E, int Q) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= E * Q) return;
  const int64_t e = t / Q;
  const int c = (int)(t - e * Q);
  const int64_t i = dst[e];
  const float cnt = (float)max(rowptr[i + 1] - rowptr[i], 1);
  float4 g = d_out[(size_t)i * lddo + c];
  g.x /= cnt; g.y /= cnt; g.z /= cnt; g.w /= cnt;
  d_msg[(size_t)e * lddm + c] = g;
}

// forward (csrc/isg_norm_pool.hip): o = x - mean(x) * ms;  y = w o / sqrt(mean(o^2) + eps) + b, per graph and channel.
// A thread owns a channel and walks the graph's column in node order, like the GraphNorm inside tail_bwd_kernel.
template <typename T>
__global__ __launch_bounds__(512) void graph_norm_bwd_kernel(const float *__restrict__ x, const int *__restrict__ ptr,
                                                             const float *__restrict__ weight, const float *__restrict__ mean_scale,
                                                             T eps, const float *__restrict__ g_out, float *__restrict__ d_x,
                                                             T *__restrict__ partial, int C) {
  const int g = blockIdx.x;
  const int nb = ptr[g], n = ptr[g + 1] - nb;
  T *pw = partial + (size_t)g * 3 * C;                      // [d weight | d bias | d mean_scale] of this graph
  if (n <= 0) {
    for (int ch = threadIdx.x; ch < C; ch += blockDim.x) pw[ch] = pw[C + ch] = pw[2 * C + ch] = (T)0;
    return;
  }
  const T cnt = (T)n;
  for (int ch = threadIdx.x; ch < C; ch += blockDim.x) {
    const float *col = x + (size_t)nb * C + ch;
    const float *gcol = g_out + (size_t)nb * C + ch;
    float *dcol = d_x + (size_t)nb * C + ch;
    T sum = (T)0;
    for (int k = 0; k < n; ++k) sum += (T)col[(size_t)k * C];
    const T mean = sum / cnt, ms = (T)mean_scale[ch], mean_ms = mean * ms;
    T sq = (T)0;
    for (int k = 0; k < n; ++k) {
      const T o = (T)col[(size_t)k * C] - mean_ms;
      sq += o * o;
    }
    const T var = sq / cnt, rstd = (T)1 / sqrt(var + eps), w = (T)weight[ch];
    T db = (T)0, dw = (T)0, gwo = (T)0;
    for (int k = 0; k < n; ++k) {
      const T gk = (T)gcol[(size_t)k * C];
      const T o = (T)col[(size_t)k * C] - mean_ms;
      db += gk;
      dw += gk * o * rstd;
      gwo += gk * w * o;
    }
    const T dvar = (T)-0.5 * gwo * rstd * rstd * rstd;
    T sdo = (T)0;
    for (int k = 0; k < n; ++k) {
      const T gk = (T)gcol[(size_t)k * C];
      const T o = (T)col[(size_t)k * C] - mean_ms;
      sdo += gk * w * rstd + dvar * (T)2 * o / cnt;
    }
    for (int k = 0; k < n; ++k) {
      const T gk = (T)gcol[(size_t)k * C];
      const T o = (T)col[(size_t)k * C] - mean_ms;
      const T d_o = gk * w * rstd + dvar * (T)2 * o / cnt;
      dcol[(size_t)k * C] = (float)(d_o - ms * sdo / cnt);
    }
    pw[ch] = dw;
    pw[C + ch] = db;
    pw[2 * C + ch] = -mean * sdo;
  }
}

static int gn_block(int C) { return C <= 64 ? 64 : (C <= 128 ? 128 : (C <= 256 ? 256 : (C <= 320 ? 320 : (C <= 384 ? 384 : 512)))); }

static bool rows_ok(const void *p, int32_t ld) { return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace isg

using namespace isg;

extern "C" int isg_sgenc_train_abi_version(void) { return ISG_SGENC_TRAIN_ABI_VERSION; }

extern "C" int32_t isg_segment_rows_chunk(void) { return SEG_CHUNK; }

extern "C" int64_t isg_segment_rows_ws_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0) return 0;
  return (M + SEG_CHUNK - 1) / SEG_CHUNK * 2 * (int64_t)C * 4;
}

extern "C" int isg_segment_rows_sum(const int32_t *rowptr, const int32_t *eid, const float *w, const float *G, int32_t ldg,
                                    int32_t gdiv, float *out, int32_t ldo, int64_t S, int64_t M, int32_t C, int64_t skip, void *ws,
                                    int64_t ws_bytes, void *stream) {
  if (S < 0 || M < 0 || C <= 0 || gdiv < 1 || skip < -1) return ISG_EINVAL;
  if (S == 0) return M == 0 ? ISG_OK : ISG_EINVAL;
  if (!rowptr || !out || (M > 0 && (!eid || !G || !ws))) return ISG_EINVAL;
  if ((C & 3) || !rows_ok(out, ldo) || (M > 0 && (!rows_ok(G, ldg) || !rows_ok(ws, 0))) || M >= (1ll << 31) - SEG_CHUNK ||
      S >= (1ll << 31) - 16 || ldo < C || (M > 0 && ldg < C))
    return ISG_EUNSUPPORTED;
  if (ws_bytes < isg_segment_rows_ws_bytes(M, C)) return ISG_EINVAL;
  const int Q = C >> 2, sk = skip >= S ? -1 : (int)skip;
  const int chunks = (int)((M + SEG_CHUNK - 1) / SEG_CHUNK);
  if (chunks > 0)
    segment_rows_chunk_kernel<<<(unsigned)((chunks + 15) / 16), 256, 0, as_stream(stream)>>>(
        rowptr, eid, w, (const float4 *)G, ldg >> 2, gdiv, (float4 *)out, ldo >> 2, (float4 *)ws, (int)S, (int)M, Q, sk, chunks);
  segment_rows_finish_kernel<<<(unsigned)((S + 15) / 16), 256, 0, as_stream(stream)>>>(rowptr, (float4 *)out, ldo >> 2,
                                                                                     (const float4 *)ws, (int)S, Q, sk);
  return check_launch();
}

extern "C" int32_t isg_gather_add_bwd_parts(int64_t E) {
  if (E <= 0) return 0;
  const int64_t blocks = (E + 15) / 16;
  return (int32_t)(blocks < GAB_PARTS_MAX ? blocks : GAB_PARTS_MAX);
}

extern "C" int isg_gather_add_bwd(const float *A, const int64_t *ia, int32_t lda, const float *B, const int64_t *ib, int32_t ldb,
                                  const float *T, const int64_t *it, const float *sign, int32_t ldt, const float *D, int32_t ldd,
                                  const float *bias, const float *d_out, int32_t lddo, float *dz, int32_t lddz, float *d_bias_part,
                                  int64_t E, int32_t C, int32_t act, void *stream) {
  if (E < 0 || C <= 0 || act < 0 || act > 1) return ISG_EINVAL;
  if (E == 0) return ISG_OK;
  if (!A || !ia || !d_out || !dz || (B && !ib) || (T && !it)) return ISG_EINVAL;
  if ((C & 3) || !rows_ok(A, lda) || (B && !rows_ok(B, ldb)) || (T && !rows_ok(T, ldt)) || (D && !rows_ok(D, ldd)) ||
      (bias && !rows_ok(bias, 0)) || !rows_ok(d_out, lddo) || !rows_ok(dz, lddz) || (d_bias_part && !rows_ok(d_bias_part, 0)) ||
      lddo < C || lddz < C || E >= (1ll << 31) * 16)
    return ISG_EUNSUPPORTED;
  // the forward's operands with the activation taken off: gather_add_value then returns z
  GatherAddArgs a{(const float4 *)A, ia, (const float4 *)B, ib, (const float4 *)T, it, sign, (const float4 *)D,
                  (const float4 *)bias, nullptr, nullptr, nullptr, E, C >> 2, lda >> 2, ldb >> 2, ldt >> 2, ldd >> 2, 0};
  const int parts = isg_gather_add_bwd_parts(E);
  const int64_t rows = (E + parts - 1) / parts;
  if (rows >= (1ll << 31)) return ISG_EUNSUPPORTED;
  gather_add_bwd_kernel<<<(unsigned)parts, 256, 0, as_stream(stream)>>>(a, (const float4 *)d_out, lddo >> 2, (float4 *)dz, lddz >> 2,
                                                                        (float4 *)d_bias_part, act, (int)rows);
  return check_launch();
}

extern "C" int isg_scatter_mean_bwd(const float *d_out, int32_t lddo, const int64_t *dst, const int32_t *rowptr, float *d_msg,
                                    int32_t lddm, int64_t N, int64_t E, int32_t C, void *stream) {
  if (N < 0 || E < 0 || C <= 0) return ISG_EINVAL;
  if (E == 0) return ISG_OK;
  if (N == 0 || !d_out || !dst || !rowptr || !d_msg) return ISG_EINVAL;
  const int64_t total = E * (C >> 2);
  if ((C & 3) || !rows_ok(d_out, lddo) || !rows_ok(d_msg, lddm) || lddo < C || lddm < C || (total + 255) / 256 >= (1ll << 31))
    return ISG_EUNSUPPORTED;
  scatter_mean_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      (const float4 *)d_out, lddo >> 2, dst, rowptr, (float4 *)d_msg, lddm >> 2, E, C >> 2);
  return check_launch();
}

extern "C" int isg_graph_norm_bwd(const float *x, const int32_t *ptr, const float *weight, const float *mean_scale, double eps,
                                  int32_t accumulate_fp64, const float *d_out, float *d_x, void *partial, int64_t B, int32_t C,
                                  void *stream) {
  if (B < 0 || C <= 0) return ISG_EINVAL;
  if ((C & 3) != 0 || B >= (1ll << 31)) return ISG_EUNSUPPORTED;
  if (B == 0) return ISG_OK;
  if (!x || !ptr || !weight || !mean_scale || !d_out || !d_x || !partial) return ISG_EINVAL;
  if (accumulate_fp64)
    graph_norm_bwd_kernel<double><<<(unsigned)B, gn_block(C), 0, as_stream(stream)>>>(x, ptr, weight, mean_scale, eps, d_out, d_x,
                                                                                     (double *)partial, C);
  else
    graph_norm_bwd_kernel<float><<<(unsigned)B, gn_block(C), 0, as_stream(stream)>>>(x, ptr, weight, mean_scale, (float)eps, d_out,
                                                                                    d_x, (float *)partial, C);
  return check_launch();
}
