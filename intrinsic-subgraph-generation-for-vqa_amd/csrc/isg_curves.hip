// Fidelity curves (include/ext/isg_curves.h, where both functions are stated word for word): the ranking of every listed graph's
// nodes with all nested keep rows of both sides as one launch, and the reduction of the instances' probabilities to areas and
// running totals as another.
//
// curve_keep_bits_kernel: one 64-lane wave (one workgroup) per listed graph.  The scores become order-preserving uint32 keys in
// LDS; lane l counts, for each of its nodes l, l + 64, ..., the keys that come before it -- four of its nodes per pass over the
// graph, every lane reading the same four LDS words (a broadcast, no bank conflict); ranks go back to LDS; a row's words are 64-bit
// ballots.  n^2 / 64 compare steps per lane: nothing at scene-graph sizes, about 65 k at n = 2048.
// curve_sums_kernel: one workgroup of S waves, wave s = side s, lane j = level j, walking the rows in order.
// No atomics; one writer per output word; every number read from memory that becomes an address is compared first.
#include "isg_common.hpp"

#include "../../include/ext/isg_curves.h"

namespace isg {

constexpr int CV_WORDS_MAX = 64, CV_LEVELS_MAX = 64;

struct CurveLevels {             // the L host values of the call, copied into the launch
  int is_frac;
  union {
    float f[CV_LEVELS_MAX];
    int t[CV_LEVELS_MAX];
  };
};

// IEEE order with every NaN below -inf and -0 = +0, as an unsigned order: NaN -> 0, -inf -> 0x007fffff, +0 -> 0x80000000
__device__ __forceinline__ uint32_t cv_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int cv_clamp(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(ISG_WAVE) void curve_keep_bits_kernel(const float *__restrict__ a, const int *__restrict__ ptr,
                                                                   const int *__restrict__ graphs, CurveLevels lv, int N, int G,
                                                                   int R, int L, int sides, int W, int *__restrict__ rank,
                                                                   int *__restrict__ level_k, int *__restrict__ index,
                                                                   uint32_t *__restrict__ keep, int *__restrict__ status) {
  extern __shared__ uint32_t cv_lds[];             // [32 W] keys, then [32 W] ranks
  const int cap = 32 * W;
  uint32_t *key = cv_lds;
  int *rk = reinterpret_cast<int *>(cv_lds + cap);
  const int lane = threadIdx.x, r = blockIdx.x;
  const int S = (sides & 1) + ((sides >> 1) & 1);
  const int g = graphs[r];
  const bool listed = g >= 0 && g < G;
  int lo = 0, n = 0;
  if (listed) {
    lo = cv_clamp(ptr[g], N);
    const int hi = max(cv_clamp(ptr[g + 1], N), lo);
    n = min(hi - lo, cap);
  }
  for (int i = lane; i < cap; i += ISG_WAVE) key[i] = i < n ? cv_key(a[lo + i]) : 0u;     // (a pad is the smallest key, behind every node)
  __syncthreads();
  for (int i0 = lane; i0 < n; i0 += 4 * ISG_WAVE) {
    uint32_t ki[4];
    int c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 4; ++u) ki[u] = key[min(i0 + u * ISG_WAVE, cap - 1)];
    for (int m = 0; m < n; m += 4) {                             // cap is a multiple of 4: the pads count for nobody
      const uint4 km = *reinterpret_cast<const uint4 *>(key + m);
      const uint32_t kv[4] = {km.x, km.y, km.z, km.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * ISG_WAVE;
#pragma unroll
        for (int v = 0; v < 4; ++v) c[u] += (kv[v] > ki[u]) | ((kv[v] == ki[u]) & (m + v < i));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * ISG_WAVE;
      if (i < n) {
        rk[i] = c[u];
        rank[lo + i] = c[u];
      }
    }
  }
  __syncthreads();
  const float nf = (float)n;
  for (int j = 0; j < L; ++j) {
    int t;
    if (lv.is_frac) {
      const float c = ceilf(mul_rn(lv.f[j], nf));
      t = c >= nf ? n : (int)c;
    } else {
      t = lv.t[j];
    }
    for (int s = 0; s < S; ++s) {
      const bool removal = s == 1 || !(sides & 1);
      const int k = n == 0 ? 0 : (removal ? min(n - 1, max(0, t)) : min(n, max(1, t)));
      const int64_t q = ((int64_t)r * L + j) * S + s;
      if (lane == 0) {
        index[q] = g;
        level_k[q] = k;
      }
      for (int c0 = 0; c0 < W; c0 += 2) {                        // 64 nodes: one ballot, two words
        const int i = c0 * 32 + lane;
        const bool bit = i < n && ((rk[i] < k) != removal);
        const unsigned long long b = __ballot(bit);
        if (lane == 0) keep[q * W + c0] = (uint32_t)b;
        if (lane == 1 && c0 + 1 < W) keep[q * W + c0 + 1] = (uint32_t)(b >> 32);
      }
    }
  }
  if (r == 0) {                                                  // the one writer of status: wave 0 reads every entry of graphs
    bool over = false, outside = false;
    for (int x = lane; x < R; x += ISG_WAVE) {
      const int gx = graphs[x];
      if (gx < 0 || gx >= G) {
        outside = true;
      } else {
        const int l = cv_clamp(ptr[gx], N);
        over |= max(cv_clamp(ptr[gx + 1], N), l) - l > cap;
      }
    }
    const bool any_over = __ballot(over) != 0ull, any_outside = __ballot(outside) != 0ull;
    if (lane == 0) {
      status[0] = any_over ? 1 : 0;
      status[1] = any_outside ? 1 : 0;
      status[2] = R * L * S;
      status[3] = 0;
    }
  }
}

__device__ __forceinline__ bool cv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(2 * ISG_WAVE) void curve_sums_kernel(const float *__restrict__ p_inst, const float *__restrict__ w,
                                                                  int R, int L, int S, float *__restrict__ auc,
                                                                  double *__restrict__ totals) {
  const int lane = threadIdx.x & (ISG_WAVE - 1), s = threadIdx.x / ISG_WAVE;       // s < S: the launch has S waves
  const bool mine = lane < L;
  const float wl = mine ? w[lane] : 0.f;
  double level = 0.0, area = 0.0, counted = 0.0, skipped = 0.0;
  for (int r = 0; r < R; ++r) {
    const float p = mine ? p_inst[((int64_t)r * L + lane) * S + s] : 0.f;
    const bool skip = __ballot(!cv_finite(p)) != 0ull;
    float v = 0.f;
    for (int j = 0; j < L; ++j) v = __builtin_fmaf(__shfl(wl, j), __shfl(p, j), v);
    if (skip) {
      skipped = dadd_rn(skipped, 1.0);
      v = __uint_as_float(0x7fc00000u);
    } else {
      level = dadd_rn(level, (double)p);
      area = dadd_rn(area, (double)v);
      counted = dadd_rn(counted, 1.0);
    }
    if (lane == 0) auc[(int64_t)r * S + s] = v;
  }
  double *row = totals + (int64_t)s * (L + 3);
  if (mine) row[lane] = dadd_rn(row[lane], level);
  if (lane == 0) {
    row[L] = dadd_rn(row[L], area);
    row[L + 1] = dadd_rn(row[L + 1], counted);
    row[L + 2] = dadd_rn(row[L + 2], skipped);
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_curve_abi_version(void) { return ISG_CURVES_ABI_VERSION; }

static inline bool cv_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }

extern "C" int isg_curve_keep_bits(const float *a, const int32_t *ptr, const int32_t *graphs, const float *frac,
                                   const int32_t *count, int64_t N, int64_t G, int64_t R, int64_t L, int32_t sides, int32_t W,
                                   int32_t *rank, int32_t *level_k, int32_t *index, uint32_t *keep, int32_t *status, void *stream) {
  if (N < 0 || G < 0 || R < 0 || L < 0 || sides < 1 || sides > 3 || W < 1) return ISG_EINVAL;
  if (L > 0 && ((frac != nullptr) == (count != nullptr))) return ISG_EINVAL;
  const int S = (sides & 1) + ((sides >> 1) & 1);
  if (W > CV_WORDS_MAX || L > CV_LEVELS_MAX || cv_too_large(N) || cv_too_large(G) || cv_too_large(R)) return ISG_EUNSUPPORTED;
  if (cv_too_large(R * L * S)) return ISG_EUNSUPPORTED;          // (R < 2^31 and L S <= 128: no overflow)
  CurveLevels lv;
  lv.is_frac = frac != nullptr;
  for (int j = 0; j < CV_LEVELS_MAX; ++j) {
    if (j >= L) {
      lv.t[j] = 0;
    } else if (frac) {
      if (!(frac[j] >= 0.f)) return ISG_EINVAL;                  // a NaN fails the comparison too
      lv.f[j] = frac[j];
    } else {
      if (count[j] < 0) return ISG_EINVAL;
      lv.t[j] = count[j];
    }
  }
  if (R == 0 || L == 0) return ISG_OK;
  if (!ptr || !graphs || !level_k || !index || !keep || !status || (N > 0 && (!a || !rank))) return ISG_EINVAL;
  curve_keep_bits_kernel<<<(unsigned)R, ISG_WAVE, (size_t)W * 256, as_stream(stream)>>>(a, ptr, graphs, lv, (int)N, (int)G, (int)R,
                                                                                         (int)L, sides, W, rank, level_k, index, keep,
                                                                                         status);
  return check_launch();
}

extern "C" int isg_curve_sums(const float *p_inst, const float *w, int64_t R, int64_t L, int32_t sides, float *auc, double *totals,
                              void *stream) {
  if (R < 0 || L < 0 || sides < 1 || sides > 3) return ISG_EINVAL;
  const int S = (sides & 1) + ((sides >> 1) & 1);
  if (L > CV_LEVELS_MAX || cv_too_large(R) || cv_too_large(R * L * S)) return ISG_EUNSUPPORTED;
  if (R == 0 || L == 0) return ISG_OK;
  if (!p_inst || !w || !auc || !totals) return ISG_EINVAL;
  curve_sums_kernel<<<1, S * ISG_WAVE, 0, as_stream(stream)>>>(p_inst, w, (int)R, (int)L, S, auc, totals);
  return check_launch();
}
