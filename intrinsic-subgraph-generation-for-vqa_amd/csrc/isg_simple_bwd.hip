// SIMPLE sampler: the backward of the exact marginals, one launch (include/isg_sampler_train.h).
//
// Forward (isg_simple.hip): out = (sample - marg).detach() + marg with marg[i] = exp(M(0, i, 1)): d out / d marg = 1 and the sample
// carries no gradient, so the kernel takes no noise and no seed.  Nothing but the scores is read from the forward: one wave owns one
// row, rebuilds W (bottom-up log-weights) and M (top-down log-marginals) in LDS with the forward's own code (sm_build_trees) and
// reverses them into two more trees of the same shape, dW and dM.
//
// With theta(pi, jp, jj) = W(l, 2pi, jj) + W(l, 2pi+1, jp-jj) - W(l+1, pi, jp) the forward's top-down pass is
//   M(l, c, j) = logsumexp over the reachable parents jp of (theta + M(l+1, pi, jp)), padded with -1000,
// and one theta feeds both children, so per parent (pi, jp) and element jj
//   E(pi, jp, jj) = dM(l, 2pi, jj)      exp(theta + M(l+1, pi, jp) - M(l, 2pi, jj))
//                 + dM(l, 2pi+1, jp-jj) exp(theta + M(l+1, pi, jp) - M(l, 2pi+1, jp-jj)).
// Sweep A, l = 0 .. L-1 (the top-down pass reversed): dM(l+1, pi, jp) = sum_jj E, dW(l+1, pi, jp) = -sum_jj E, and E is added to both
// children's dW.  Sweep B, l = L .. 1 (the bottom-up pass reversed): dW(l, i, j) exp(term - W(l, i, j)) is added to the dW of the two
// children whose sum `term` is.  d scores[i] = dW(0, i, 1); W(0, i, 0) = log1mexp(-w) is detached (simple.py:204).  The dummy pads
// of both logsumexps sit in W and M, i.e. in every denominator, and receive nothing; unreachable (level, count) nodes are skipped.
//
// Every sum is a GATHER in a fixed order: a lane owns a node and adds up what reaches it (E is evaluated once by the parent and
// once by each of the two children it is added to).  No atomic add anywhere: two launches agree bit for bit.
#include "isg_simple.hpp"

namespace isg {

struct SimpleBwdArgs {
  const float *scores;
  const int *ptr;        // NULL -> dense [B, nmax]
  const float *g_out;    // d out in the layout of scores, or NULL -> 0
  const float *g_marg;   // d marginals, dense [B, nmax], or NULL -> 0
  float *d_scores;       // layout of scores
  int B, nmax;
};

__global__ __launch_bounds__(256) void simple_bwd_kernel(SimpleBwdArgs a, SimpleTables c, int rows_per_block) {
  extern __shared__ float s_tree[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave >= rows_per_block) return;
  const int b = blockIdx.x * rows_per_block + wave;
  if (b >= a.B) return;
  const int n = c.n, K1 = c.k + 1, L = c.levels;
  const int tree = (2 * n - 1) * K1;
  float *W = s_tree + (size_t)wave * 4 * tree, *M = W + tree, *dW = M + tree, *dM = dW + tree;
  const int base = a.ptr ? a.ptr[b] : b * a.nmax;
  const int len = a.ptr ? a.ptr[b + 1] - base : a.nmax;
  auto lvl = [&](int l) { return sm_lvl(n, K1, l); };
  auto flat = [&](int i) -> float {
    return i < len ? a.scores[base + i] : (i < a.nmax ? 0.f : -1.0e10f);   // to_dense_batch pad 0.0, then -LARGE_NUMBER
  };
  sm_build_trees(W, M, c, lane, flat);
  // seeds: d M(0, i, 1) = d marg[i] marg[i]; the slots of a ragged row's zero pads have no d out but may have a d marg
  for (int i = lane; i < n; i += 64) {
    float g = 0.f;
    if (i < a.nmax) {
      const float go = (a.g_out && i < len) ? a.g_out[base + i] : 0.f;
      const float gm = a.g_marg ? a.g_marg[(size_t)b * a.nmax + i] : 0.f;
      g = (go + gm) * expf(M[i * K1 + 1]);
    }
    dM[i * K1 + 0] = 0.f;
    dM[i * K1 + 1] = g;
    dW[i * K1 + 0] = 0.f;
    dW[i * K1 + 1] = 0.f;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // sweep A: the top-down pass reversed.  The parents' lanes write level l+1, the children's lanes add to level l: no word is
  // written by one and read by the other, one barrier per level.
  for (int l = 0; l < L; ++l) {
    const int blocks = n >> l, capl = c.cap[l], capp = c.cap[l + 1];
    const float *Wc = W + lvl(l), *Wp = W + lvl(l + 1), *Mc = M + lvl(l), *Mp = M + lvl(l + 1), *dMc = dM + lvl(l);
    float *dWc = dW + lvl(l), *dWp = dW + lvl(l + 1), *dMp = dM + lvl(l + 1);
    auto E = [&](int pi, int jp, int jj) -> float {
      const int cl = (2 * pi) * K1 + jj, cr = (2 * pi + 1) * K1 + (jp - jj);
      const float theta = (Wc[cl] + Wc[cr]) - Wp[pi * K1 + jp];
      const float x = theta + Mp[pi * K1 + jp];
      return dMc[cl] * expf(x - Mc[cl]) + dMc[cr] * expf(x - Mc[cr]);
    };
    for (int idx = lane; idx < (blocks >> 1) * (capp + 1); idx += 64) {
      const int pi = idx / (capp + 1), jp = idx - pi * (capp + 1);
      if (!((c.reach[l + 1] >> jp) & 1)) continue;
      float s = 0.f;
      for (int jj = max(0, jp - capl); jj <= min(jp, capl); ++jj) s += E(pi, jp, jj);
      dMp[pi * K1 + jp] = s;
      dWp[pi * K1 + jp] = -s;
    }
    for (int idx = lane; idx < blocks * (capl + 1); idx += 64) {
      const int i = idx / (capl + 1), j = idx - i * (capl + 1);
      if (!((c.reach[l] >> j) & 1)) continue;
      float s = 0.f;
      for (int jp = j; jp <= min(capp, j + capl); ++jp)
        if ((c.reach[l + 1] >> jp) & 1) s += E(i >> 1, jp, (i & 1) ? jp - j : j);
      dWc[i * K1 + j] += s;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // sweep B: the bottom-up pass reversed; a child's lane gathers from the parents whose logsumexp holds a term with it
  for (int l = L; l >= 1; --l) {
    const int blocks = n >> (l - 1), capl = c.cap[l], capc = c.cap[l - 1];
    const float *Wc = W + lvl(l - 1), *Wl = W + lvl(l), *dWl = dW + lvl(l);
    float *dWc = dW + lvl(l - 1);
    for (int idx = lane; idx < blocks * (capc + 1); idx += 64) {
      const int ci = idx / (capc + 1), jc = idx - ci * (capc + 1);
      if (!((c.reach[l - 1] >> jc) & 1)) continue;
      const int i = ci >> 1;
      const float *pl = Wc + (2 * i) * K1, *pr = Wc + (2 * i + 1) * K1;
      float s = 0.f;
      for (int j = jc; j <= min(capl, jc + capc); ++j) {
        if (!((c.reach[l] >> j) & 1)) continue;
        const int jj = (ci & 1) ? j - jc : jc;
        const float term = pl[jj] + pr[j - jj];
        s += dWl[i * K1 + j] * expf(term - Wl[i * K1 + j]);
      }
      dWc[ci * K1 + jc] += s;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  for (int i = lane; i < min(len, a.nmax); i += 64) a.d_scores[base + i] = dW[i * K1 + 1];
}

// THE shape rule, host only: the LDS bytes of one row -- four trees (W, M, dW, dM) of (2n - 1)(kk + 1) floats, n = nmax rounded up
// to a power of two, kk = min(k, nmax) -- or a negative status for a shape that is refused; *rows = the rows (waves) of one workgroup.
constexpr int64_t SMB_ROW_LIMIT = 150 * 1024;     // a row beyond it is refused (a workgroup may hold 160 KiB)
constexpr int64_t SMB_WG_BUDGET = 48 * 1024;      // rows per workgroup: as many as fit in it, at most 4 (the waves), at least 1

inline int64_t smb_row_rule(int k, int nmax, int *rows) {
  *rows = 0;
  if (k <= 0 || nmax < 0) return ISG_EINVAL;
  if (nmax == 0) return 0;
  const int kk = k < nmax ? k : nmax;
  if (nmax > (1 << SM_MAXL) || kk > SM_MAXK) return ISG_EUNSUPPORTED;
  int64_t n = 1;
  while (n < nmax) n <<= 1;
  const int64_t row_bytes = 4 * (2 * n - 1) * (kk + 1) * (int64_t)sizeof(float);
  if (row_bytes > SMB_ROW_LIMIT) return ISG_EUNSUPPORTED;
  const int64_t fit = SMB_WG_BUDGET / row_bytes;
  *rows = (int)(fit > 4 ? 4 : (fit < 1 ? 1 : fit));
  return row_bytes;
}

}  // namespace isg

using namespace isg;

extern "C" int isg_sampler_train_abi_version(void) { return 1; }

extern "C" int64_t isg_simple_topk_bwd_row_bytes(int32_t k, int32_t nmax) {
  int rows = 0;
  return smb_row_rule(k, nmax, &rows);
}

extern "C" int isg_simple_topk_bwd(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax, int32_t k, const float *g_out,
                                   const float *g_marg, float *d_scores, void *stream) {
  if (B < 0 || nmax < 0 || k <= 0) return ISG_EINVAL;
  if (B == 0 || nmax == 0) return ISG_OK;
  if (B >= (1ll << 31)) return ISG_EUNSUPPORTED;
  SimpleBwdArgs a = {.scores = scores, .ptr = ptr, .g_out = g_out, .g_marg = g_marg, .d_scores = d_scores, .B = (int)B, .nmax = nmax};
  if (!a.scores || !a.d_scores) return ISG_EINVAL;
  int rows = 0;
  const int64_t row_bytes = smb_row_rule(k, nmax, &rows);
  if (row_bytes < 0) return (int)row_bytes;
  const SimpleTables c = sm_make_tables(k, nmax);
  if (rows * row_bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(simple_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(rows * row_bytes)) != hipSuccess)
    return ISG_ELAUNCH;
  simple_bwd_kernel<<<(unsigned)((B + rows - 1) / rows), 256, (size_t)(rows * row_bytes), as_stream(stream)>>>(a, c, rows);
  return check_launch();
}
