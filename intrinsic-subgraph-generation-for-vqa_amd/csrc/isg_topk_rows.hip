// Top-k samplers with a node budget per graph (include/isg_topk_rows.h): the planning kernel that turns a share of
// each graph's nodes into k_rows, and the three sampler entry points that read k per row.  The sampler kernels are the scalar
// entry points' (isg_topk.hpp) instantiated with ROWS = true: a wave loads k_rows[b] once, clamps it to [0, k_cap] and runs the
// same arithmetic, so row b's bits are the scalar entry point's at k = k_rows[b].
#include "isg_topk.hpp"

#include "../../include/isg_topk_rows.h"

namespace isg {

// k_rows[b] = min(k_cap, max(k_min, ceil(ratio * n_b))).  One thread per graph.  The product is mul_rn: one fp32 multiplication
// that nothing contracts, torch's `ratio * n.float()`.  The comparison with k_cap is made on the float, before the conversion: a
// product beyond the int range (any ratio > 0 is admitted) is k_cap, never an out-of-range cast.
__global__ __launch_bounds__(256) void topk_budget_kernel(const int *__restrict__ ptr, int B, float ratio, int k_min, int k_cap,
                                                          int *__restrict__ k_rows) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int n = ptr[b + 1] - ptr[b];
  const float c = ceilf(mul_rn(ratio, (float)n));
  const int k = c >= (float)k_cap ? k_cap : (int)c;
  k_rows[b] = min(k_cap, max(k_min, k));
}

}  // namespace isg

using namespace isg;

extern "C" int isg_topk_rows_abi_version(void) { return 1; }

extern "C" int isg_topk_budget(const int32_t *ptr, int64_t B, float ratio, int32_t k_min, int32_t k_cap, int32_t *k_rows,
                               void *stream) {
  if (B < 0 || !(ratio > 0.f) || k_min < 1 || k_cap < k_min) return ISG_EINVAL;
  if (B > 0 && (!ptr || !k_rows)) return ISG_EINVAL;
  if (B >= (1ll << 31)) return ISG_EUNSUPPORTED;
  if (B == 0) return ISG_OK;
  topk_budget_kernel<<<(unsigned)((B + 255) / 256), 256, 0, as_stream(stream)>>>(ptr, (int)B, ratio, k_min, k_cap, k_rows);
  return check_launch();
}

extern "C" int isg_topk_threshold_rows(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                                       const int32_t *nmax_dev, const float *noise, float noise_scale, uint64_t seed,
                                       const int32_t *graph_ids, const int32_t *k_rows, int32_t k_cap, float *out,
                                       float *dense_out, void *stream) {
  int st = check_rows(scores, B, nmax_host, k_cap, out);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  if (!k_rows) return ISG_EINVAL;
  RowArgs a{scores, ptr, nmax_dev, noise, out, dense_out, (int)B, nmax_host, k_cap, 1.f, noise_scale, seed, graph_ids, k_rows};
  return launch_topk_threshold<true>(a, as_stream(stream));
}

extern "C" int isg_topk_gumbel_rows(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                                    const int32_t *nmax_dev, const float *noise, uint64_t seed, const int32_t *graph_ids,
                                    const int32_t *k_rows, int32_t k_cap, float tau, float *out, float *khot_out, void *stream) {
  int st = check_rows(scores, B, nmax_host, k_cap, out);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  if (!(tau > 0.f) || !k_rows) return ISG_EINVAL;
  RowArgs a{scores, ptr, nmax_dev, noise, out, khot_out, (int)B, nmax_host, k_cap, tau, 0.f, seed, graph_ids, k_rows};
  return launch_topk_gumbel<true>(a, as_stream(stream));
}

extern "C" int isg_topk_gumbel_rows_bwd(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                                        const int32_t *nmax_dev, const float *noise, uint64_t seed, const int32_t *graph_ids,
                                        const int32_t *k_rows, int32_t k_cap, float tau, const float *d_out, float *d_scores,
                                        void *stream) {
  int st = check_rows(scores, B, nmax_host, k_cap, d_scores);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  if (!(tau > 0.f) || !d_out || !k_rows) return ISG_EINVAL;
  RowArgs a{scores, ptr, nmax_dev, noise, nullptr, nullptr, (int)B, nmax_host, k_cap, tau, 0.f, seed, graph_ids, k_rows};
  return launch_topk_gumbel_bwd<true>(a, d_out, d_scores, as_stream(stream));
}
