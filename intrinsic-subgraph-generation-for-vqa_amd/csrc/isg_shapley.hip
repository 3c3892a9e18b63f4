// Shapley sampling (include/ext/isg_shapley.h, where both functions and the estimator are stated word for word): the seeded
// permutations of every listed graph's nodes with the keep rows of all their prefixes as one launch, and the reduction of the
// instances' probabilities to per-node Shapley estimates, their sums of squares and every graph's completeness gap as another.
//
// shapley_keep_bits_kernel: one 64-lane wave (one workgroup) per (listed graph, draw).  The Philox keys of the draw go to LDS;
// lane l counts, for each of its nodes l, l + 64, ..., the keys that come before it -- four of its nodes per pass over the graph,
// every lane reading the same four LDS words (a broadcast, no bank conflict), curve_keep_bits_kernel's counting rank; positions
// go back to LDS; a row's words are 64-bit ballots.  The wave writes its draw's rows and, under antithetic, the reversed twin's.
// shapley_values_kernel: one wave per listed graph; a ballot sets the skip flag, then lane l walks its nodes and the draws in order.
// No atomics; one writer per output word; every number read from memory that becomes an address is compared first.
#include "isg_common.hpp"

#include <cstring>

#include "../../include/ext/isg_shapley.h"

namespace isg {

constexpr int SV_WORDS_MAX = 64, SV_PERMUTATIONS_MAX = 1024;
constexpr uint32_t SV_STREAM = 0x80000000u;      // the top bit of a key's slot word: apart from the samplers' (g, slot) draws

__device__ __forceinline__ int sv_clamp(int v, int hi) { return min(max(v, 0), hi); }

// the node range of graph g (compared by the caller: 0 <= g < G), cut at cap nodes; returns n and sets lo, over
__device__ __forceinline__ int sv_range(const int *__restrict__ ptr, int g, int N, int cap, int &lo, bool &over) {
  lo = sv_clamp(ptr[g], N);
  const int hi = max(sv_clamp(ptr[g + 1], N), lo);
  over = hi - lo > cap;
  return min(hi - lo, cap);
}

__global__ __launch_bounds__(ISG_WAVE) void shapley_keep_bits_kernel(const int *__restrict__ ptr, const int *__restrict__ graphs,
                                                                     const int *__restrict__ row_ptr, int N, int G, int R, int M,
                                                                     int Q, int antithetic, uint64_t seed, int W,
                                                                     int *__restrict__ pos, int *__restrict__ index,
                                                                     uint32_t *__restrict__ keep, int *__restrict__ status) {
  extern __shared__ uint32_t sv_lds[];             // [32 W] keys, then [32 W] positions
  const int cap = 32 * W;
  uint32_t *key = sv_lds;
  int *pk = reinterpret_cast<int *>(sv_lds + cap);
  const int lane = threadIdx.x, r = blockIdx.x, t = blockIdx.y;
  const int g = graphs[r];
  const bool listed = g >= 0 && g < G;
  int lo = 0, n = 0;
  bool over = false;
  if (listed) n = sv_range(ptr, g, N, cap, lo, over);
  const int64_t first = row_ptr[r], need = (int64_t)M * max(n - 1, 0);
  const bool writes = listed && first >= 0 && first + need <= (int64_t)Q;
  if (writes && n > 0) {                                         // (uniform over the wave: the barriers below are reached by all or none)
    for (int i = lane; i < cap; i += ISG_WAVE)                   // (a pad is the largest key behind every node: it counts for nobody)
      key[i] = i < n ? Philox::draw(seed, (uint32_t)g, SV_STREAM | ((uint32_t)t << 11) | (uint32_t)i) : 0xffffffffu;
    __syncthreads();
    const int m0 = antithetic ? 2 * t : t;
    for (int i0 = lane; i0 < n; i0 += 4 * ISG_WAVE) {
      uint32_t ki[4];
      int c[4] = {0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < 4; ++u) ki[u] = key[min(i0 + u * ISG_WAVE, cap - 1)];
      for (int j = 0; j < n; j += 4) {                           // cap is a multiple of 4
        const uint4 kj = *reinterpret_cast<const uint4 *>(key + j);
        const uint32_t kv[4] = {kj.x, kj.y, kj.z, kj.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * ISG_WAVE;
#pragma unroll
          for (int v = 0; v < 4; ++v) c[u] += (kv[v] < ki[u]) | ((kv[v] == ki[u]) & (j + v < i));
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * ISG_WAVE;
        if (i < n) {
          pk[i] = c[u];
          pos[(int64_t)m0 * N + lo + i] = c[u];
          if (antithetic) pos[(int64_t)(m0 + 1) * N + lo + i] = n - 1 - c[u];
        }
      }
    }
    __syncthreads();
    for (int twin = 0; twin <= antithetic; ++twin) {
      const int64_t q0 = first + (int64_t)(m0 + twin) * (n - 1);
      for (int k = 1 + lane; k < n; k += ISG_WAVE) index[q0 + k - 1] = g;
      for (int c0 = 0; c0 < W; c0 += 2) {                        // 64 nodes: one ballot per row, two words
        const int i = c0 * 32 + lane;
        const int p = i < n ? (twin ? n - 1 - pk[i] : pk[i]) : n;                // (a pad is in no prefix)
        for (int k = 1; k < n; ++k) {
          const unsigned long long b = __ballot(p < k);
          uint32_t *row = keep + (q0 + k - 1) * W;
          if (lane == 0) row[c0] = (uint32_t)b;
          if (lane == 1 && c0 + 1 < W) row[c0 + 1] = (uint32_t)(b >> 32);
        }
      }
    }
  }
  if (r == 0 && t == 0) {                                        // the one writer of status: this wave reads every entry
    bool any_over = false, outside = false, bad = false;
    for (int x = lane; x < R; x += ISG_WAVE) {
      const int gx = graphs[x];
      int nx = 0, lx = 0;
      bool ox = false;
      if (gx < 0 || gx >= G) {
        outside = true;
      } else {
        nx = sv_range(ptr, gx, N, cap, lx, ox);
        any_over |= ox;
      }
      const int64_t fx = row_ptr[x], needx = (int64_t)M * max(nx - 1, 0);
      bad |= fx < 0 || fx + needx > (int64_t)Q || (int64_t)row_ptr[x + 1] != fx + needx;
    }
    const bool s0 = __ballot(any_over) != 0ull, s1 = __ballot(outside) != 0ull, s2 = __ballot(bad) != 0ull;
    if (lane == 0) {
      status[0] = s0 ? 1 : 0;
      status[1] = s1 ? 1 : 0;
      status[2] = s2 ? 1 : 0;
      status[3] = Q;
    }
  }
}

__device__ __forceinline__ bool sv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// d = v(P_pos+1) - v(P_pos) of one node in permutation m; ps is read from memory: clamped before it forms a row number
__device__ __forceinline__ float sv_marginal(const float *__restrict__ slice, int m, int n, int ps, float pg, float v_empty) {
  ps = sv_clamp(ps, n - 1);
  const float *row = slice + (int64_t)m * (n - 1);
  const float v_hi = ps + 1 >= n ? pg : row[ps];
  const float v_lo = ps == 0 ? v_empty : row[ps - 1];
  return sub_rn(v_hi, v_lo);
}

__global__ __launch_bounds__(ISG_WAVE) void shapley_values_kernel(const float *__restrict__ p_inst, const float *__restrict__ p,
                                                                  const int *__restrict__ pos, const int *__restrict__ ptr,
                                                                  const int *__restrict__ graphs, const int *__restrict__ row_ptr,
                                                                  int N, int G, int M, int Q, int antithetic, float v_empty, int W,
                                                                  float *__restrict__ phi, float *__restrict__ m2,
                                                                  float *__restrict__ gap, int *__restrict__ flag) {
  const int lane = threadIdx.x, r = blockIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  const int g = graphs[r];
  const bool listed = g >= 0 && g < G;
  int lo = 0, n = 0;
  bool over = false;
  if (listed) n = sv_range(ptr, g, N, 32 * W, lo, over);
  const int64_t first = row_ptr[r], need = (int64_t)M * max(n - 1, 0);
  if (!listed || first < 0 || first + need > (int64_t)Q) {
    if (lane == 0) {
      gap[r] = nan;
      flag[r] = 2;
    }
    return;
  }
  if (n == 0) {
    if (lane == 0) {
      gap[r] = 0.f;
      flag[r] = 0;
    }
    return;
  }
  const float *slice = p_inst + first;             // (first + need <= Q: the graph's rows lie inside p_inst)
  const float pg = p[g];
  bool nonfinite = !sv_finite(pg);
  for (int64_t x = lane; x < need; x += ISG_WAVE) nonfinite |= !sv_finite(slice[x]);
  const bool skip = __ballot(nonfinite) != 0ull;
  const int T = antithetic ? M / 2 : M;
  const float tf = (float)T;
  float mine = 0.f;
  for (int i = lane; i < n; i += ISG_WAVE) {
    float acc = 0.f, sq = 0.f;
    if (skip) {
      acc = nan;
      sq = nan;
    } else {
      const int *col = pos + lo + i;
      for (int t = 0; t < T; ++t) {
        float e;
        if (antithetic) {
          const float d0 = sv_marginal(slice, 2 * t, n, col[(int64_t)(2 * t) * N], pg, v_empty);
          const float d1 = sv_marginal(slice, 2 * t + 1, n, col[(int64_t)(2 * t + 1) * N], pg, v_empty);
          e = mul_rn(0.5f, add_rn(d0, d1));
        } else {
          e = sv_marginal(slice, t, n, col[(int64_t)t * N], pg, v_empty);
        }
        acc = add_rn(acc, e);
        sq = __builtin_fmaf(e, e, sq);
      }
      acc = __fdiv_rn(acc, tf);
    }
    phi[lo + i] = acc;
    if (m2) m2[lo + i] = sq;
    mine = add_rn(mine, acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine = add_rn(mine, __shfl_xor(mine, off));
  if (lane == 0) {
    gap[r] = skip ? nan : sub_rn(mine, sub_rn(pg, v_empty));
    flag[r] = skip ? 1 : 0;
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_shapley_abi_version(void) { return ISG_SHAPLEY_ABI_VERSION; }

static inline bool sv_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }

// the checks both entry points share, in the header's order; ISG_OK: the sizes are admitted
static int sv_check_sizes(int64_t N, int64_t G, int64_t R, int64_t M, int64_t Q, int32_t antithetic, int32_t W, bool v_ok) {
  if (N < 0 || G < 0 || R < 0 || M < 1 || Q < 0 || antithetic < 0 || antithetic > 1 || (antithetic && (M & 1)) || W < 1 || !v_ok)
    return ISG_EINVAL;
  if (W > SV_WORDS_MAX || M > SV_PERMUTATIONS_MAX || sv_too_large(N) || sv_too_large(G) || sv_too_large(R) || sv_too_large(Q))
    return ISG_EUNSUPPORTED;
  if (sv_too_large(M * N)) return ISG_EUNSUPPORTED;               // (M <= 1024 and N < 2^31: no overflow)
  return ISG_OK;
}

extern "C" int isg_shapley_keep_bits(const int32_t *ptr, const int32_t *graphs, const int32_t *row_ptr, int64_t N, int64_t G,
                                     int64_t R, int64_t M, int64_t Q, int32_t antithetic, uint64_t seed, int32_t W, int32_t *pos,
                                     int32_t *index, uint32_t *keep, int32_t *status, void *stream) {
  const int st = sv_check_sizes(N, G, R, M, Q, antithetic, W, true);
  if (st != ISG_OK) return st;
  if (R == 0) return ISG_OK;
  if (!ptr || !graphs || !row_ptr || !status || (N > 0 && !pos) || (Q > 0 && (!index || !keep))) return ISG_EINVAL;
  const dim3 grid((unsigned)R, (unsigned)(antithetic ? M / 2 : M));
  shapley_keep_bits_kernel<<<grid, ISG_WAVE, (size_t)W * 256, as_stream(stream)>>>(ptr, graphs, row_ptr, (int)N, (int)G, (int)R,
                                                                                   (int)M, (int)Q, antithetic, seed, W, pos, index,
                                                                                   keep, status);
  return check_launch();
}

extern "C" int isg_shapley_values(const float *p_inst, const float *p, const int32_t *pos, const int32_t *ptr,
                                  const int32_t *graphs, const int32_t *row_ptr, int64_t N, int64_t G, int64_t R, int64_t M, int64_t Q,
                                  int32_t antithetic, float v_empty, int32_t W, float *phi, float *m2, float *gap, int32_t *flag,
                                  void *stream) {
  uint32_t bits;
  memcpy(&bits, &v_empty, sizeof bits);
  const int st = sv_check_sizes(N, G, R, M, Q, antithetic, W, (bits & 0x7f800000u) != 0x7f800000u);
  if (st != ISG_OK) return st;
  if (R == 0) return ISG_OK;
  if (!ptr || !graphs || !row_ptr || !gap || !flag || (G > 0 && !p) || (N > 0 && (!pos || !phi)) || (Q > 0 && !p_inst))
    return ISG_EINVAL;
  shapley_values_kernel<<<(unsigned)R, ISG_WAVE, 0, as_stream(stream)>>>(p_inst, p, pos, ptr, graphs, row_ptr, (int)N, (int)G, (int)M,
                                                                         (int)Q, antithetic, v_empty, W, phi, m2, gap, flag);
  return check_launch();
}
