// What the SIMPLE sampler's forward (isg_simple.hip) and the backward of its marginals (isg_simple_bwd.hip) share: the (level, count)
// tables of the exactly-k circuit, built on the host, and the device code that evaluates the circuit's two trees in LDS -- W
// (log-weights, bottom-up) and M (log-marginals, top-down).  The backward reverses the trees the forward built, so it has to build
// them with the forward's own arithmetic: both kernels call sm_build_trees.  Header of isg_simple.hip: the circuit and its two
// padding accidents.
#pragma once
#include "isg_common.hpp"

namespace isg {

constexpr int SM_MAXL = 10;   // n <= 1024
constexpr int SM_MAXK = 16;

struct SimpleTables {
  int n, k, levels, max_elements, max_parents;
  int cap[SM_MAXL + 1];
  unsigned reach[SM_MAXL + 1];                 // bit j: node (l, *, j) reachable
  unsigned char n_par[SM_MAXL + 1][SM_MAXK + 1];
};

// the (level, count) tables of the exactly-k circuit over nmax variables (create_simple_constraint.py:34-66, simple.py:132-200);
// k is clamped to nmax (simple_scheme.py:84).  The caller has checked 0 < nmax <= 2^SM_MAXL and 0 < min(k, nmax) <= SM_MAXK.
inline SimpleTables sm_make_tables(int k, int nmax) {
  SimpleTables c{};
  int L = 0;
  while ((1 << L) < nmax) ++L;
  c.n = 1 << L;
  c.k = k < nmax ? k : nmax;
  c.levels = L;
  int n_elem[SM_MAXL + 1][SM_MAXK + 1] = {};
  for (int l = 0; l <= L; ++l) c.cap[l] = c.k < (1 << l) ? c.k : (1 << l);
  for (int l = 1; l <= L; ++l)
    for (int j = 0; j <= c.cap[l]; ++j)
      for (int jj = 0; jj <= j; ++jj)
        if (jj <= c.cap[l - 1] && j - jj <= c.cap[l - 1]) ++n_elem[l][j];
  c.reach[L] = 1u << c.k;
  for (int l = L - 1; l >= 0; --l)
    for (int j = 0; j <= c.cap[l]; ++j)
      for (int jp = j; jp <= c.cap[l + 1] && jp - j <= c.cap[l]; ++jp)
        if ((c.reach[l + 1] >> jp) & 1) { c.reach[l] |= 1u << j; ++c.n_par[l][j]; }
  for (int l = 1; l <= L; ++l)
    for (int j = 0; j <= c.cap[l]; ++j)
      if (((c.reach[l] >> j) & 1) && n_elem[l][j] > c.max_elements) c.max_elements = n_elem[l][j];
  for (int l = 0; l < L; ++l)
    for (int j = 0; j <= c.cap[l]; ++j)
      if (((c.reach[l] >> j) & 1) && c.n_par[l][j] > c.max_parents) c.max_parents = c.n_par[l][j];
  return c;
}

__device__ __forceinline__ float sm_log1mexp(float x) {   // simple.py:45-57: log(1 - exp(-|x|))
  x = -fabsf(x);
  return x > -0.6931471805599453094f ? logf(-expm1f(x)) : log1pf(-expf(x));
}

// torch.logsumexp over `cnt` values produced by f(t), plus `pads` copies of `padv`
template <typename F>
__device__ __forceinline__ float sm_lse(int cnt, F f, int pads, float padv) {
  float m = pads > 0 ? padv : -INFINITY;
  for (int t = 0; t < cnt; ++t) {
    const float v = f(t);
    m = (v > m || v != v) ? v : m;            // amax propagates NaN
  }
  const float ms = (fabsf(m) == INFINITY) ? 0.f : m;
  float s = pads > 0 ? (float)pads * expf(padv - ms) : 0.f;
  for (int t = 0; t < cnt; ++t) s += expf(f(t) - ms);
  return logf(s) + ms;
}

// offset of level l (n >> l blocks of K1 counts) in a tree of (2n - 1) K1 floats
__device__ __forceinline__ int sm_lvl(int n, int K1, int l) { return (2 * n - (2 * n >> l)) * K1; }

// One wave fills its row's W and M from flat(i), the row's padded score of leaf i.  Ends behind a wave barrier.
template <typename Flat>
__device__ __forceinline__ void sm_build_trees(float *W, float *M, const SimpleTables &c, int lane, Flat flat) {
  const int n = c.n, k = c.k, K1 = k + 1, L = c.levels;
  auto lvl = [&](int l) { return sm_lvl(n, K1, l); };
  // leaves
  for (int i = lane; i < n; i += 64) {
    const float w = flat(i);
    W[i * K1 + 0] = sm_log1mexp(-w);
    W[i * K1 + 1] = w;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // bottom-up: W(l, i, j) = logsumexp_jj (W(l-1, 2i, jj) + W(l-1, 2i+1, j-jj)), dummy-padded to max_elements
  for (int l = 1; l <= L; ++l) {
    const int blocks = n >> l, capl = c.cap[l], capc = c.cap[l - 1];
    const float *Wc = W + lvl(l - 1);
    float *Wl = W + lvl(l);
    for (int idx = lane; idx < blocks * (capl + 1); idx += 64) {
      const int i = idx / (capl + 1), j = idx - i * (capl + 1);
      if (!((c.reach[l] >> j) & 1)) continue;
      const int lo = max(0, j - capc), hi = min(j, capc);
      const float *pl = Wc + (2 * i) * K1, *pr = Wc + (2 * i + 1) * K1;
      Wl[i * K1 + j] = sm_lse(hi - lo + 1, [&](int t) { return pl[lo + t] + pr[j - lo - t]; },
                              c.max_elements - (hi - lo + 1), -2000.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // top-down: M(root) = 0; M(child) = logsumexp over parents (theta(parent, element) + M(parent)), dummy-padded
  if (lane == 0) M[lvl(L) + k] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int l = L - 1; l >= 0; --l) {
    const int blocks = n >> l, capl = c.cap[l], capp = c.cap[l + 1];
    const float *Wc = W + lvl(l), *Wp = W + lvl(l + 1), *Mp = M + lvl(l + 1);
    float *Ml = M + lvl(l);
    for (int idx = lane; idx < blocks * (capl + 1); idx += 64) {
      const int i = idx / (capl + 1), j = idx - i * (capl + 1);
      if (!((c.reach[l] >> j) & 1)) continue;
      const int pi = i >> 1;
      const float *pl = Wc + (2 * pi) * K1, *pr = Wc + (2 * pi + 1) * K1;
      // parents jp in [j, min(capp, j + capl)] that are reachable; gather them into a tiny list first
      int jps[SM_MAXK + 1], np = 0;
      for (int jp = j; jp <= min(capp, j + capl); ++jp)
        if ((c.reach[l + 1] >> jp) & 1) jps[np++] = jp;
      Ml[i * K1 + j] = sm_lse(np, [&](int t) {
        const int jp = jps[t];
        const int jj = (i & 1) ? jp - j : j;          // this child is the sub (right) / the prime (left)
        const float theta = (pl[jj] + pr[jp - jj]) - Wp[pi * K1 + jp];
        return theta + Mp[pi * K1 + jp];
      }, c.max_parents - np, -1000.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace isg
