// Node gate scores and the entry points of the discrete top-k node-mask samplers with one k for the whole batch (Gumbel relaxed
// top-k, I-MLE / AIMLE threshold top-k).  The sampler kernels are in isg_topk.hpp, which the entry points with a k per row
// (isg_topk_rows.hip) share; here they are instantiated with ROWS = false, the code these entry points always ran.
#include "isg_topk.hpp"

namespace isg {

// ---- node gate --------------------------------------------------------------------------------------
// 16 lanes per node (4 nodes per wave); lane l covers float4 columns l, l+16, ...
__global__ __launch_bounds__(256) void node_gate_kernel(const float4 *__restrict__ xn, const float4 *__restrict__ q,
                                                        const int64_t *__restrict__ batch, int dbl,
                                                        float *__restrict__ gate, int N, int Q, float denom) {
  const int lane = threadIdx.x & 63;
  const int grp = lane >> 4, l = lane & 15;
  const int n = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + grp;
  float part = 0.f;
  if (n < N) {
    int64_t b = batch[n];
    if (dbl) b = batch[min(b, (int64_t)N - 1)];   // batch[batch[n]] (quirk Q3)
    const float4 *xr = xn + (size_t)n * Q;
    const float4 *qr = q + (size_t)b * Q;
    for (int c = l; c < Q; c += 16) part += dot4_rn(xr[c], qr[c]);
  }
  const float dot = group_sum<16>(part);
  if (n < N && l == 0) gate[n] = gelu_libm(dot / denom);
}

}  // namespace isg

using namespace isg;

extern "C" int isg_node_gate(const float *xn, const float *q, const int64_t *batch, int32_t double_index, float *gate,
                             int64_t N, int32_t C, void *stream) {
  if (N < 0 || C <= 0) return ISG_EINVAL;
  if (N == 0) return ISG_OK;
  if (!xn || !q || !batch || !gate) return ISG_EINVAL;
  if ((C & 3) != 0 || N >= (1ll << 31)) return ISG_EUNSUPPORTED;
  const float denom = sqrtf((float)C);   // torch.sqrt(torch.tensor(C)) -> fp32 (masking.py:153)
  node_gate_kernel<<<(unsigned)((N + 15) / 16), 256, 0, as_stream(stream)>>>(
      (const float4 *)xn, (const float4 *)q, batch, double_index, gate, (int)N, C >> 2, denom);
  return check_launch();
}

extern "C" int isg_topk_gumbel(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                               const int32_t *nmax_dev, const float *noise, uint64_t seed, const int32_t *graph_ids,
                               int32_t k, float tau, float *out, float *khot_out, void *stream) {
  int st = check_rows(scores, B, nmax_host, k, out);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  if (!(tau > 0.f)) return ISG_EINVAL;
  RowArgs a{scores, ptr, nmax_dev, noise, out, khot_out, (int)B, nmax_host, k, tau, 0.f, seed, graph_ids, nullptr};
  return launch_topk_gumbel<false>(a, as_stream(stream));
}

extern "C" int isg_topk_threshold(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                                  const int32_t *nmax_dev, const float *noise, float noise_scale, uint64_t seed,
                                  const int32_t *graph_ids, int32_t k, float *out, float *dense_out, void *stream) {
  int st = check_rows(scores, B, nmax_host, k, out);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  RowArgs a{scores, ptr, nmax_dev, noise, out, dense_out, (int)B, nmax_host, k, 1.f, noise_scale, seed, graph_ids, nullptr};
  return launch_topk_threshold<false>(a, as_stream(stream));
}

extern "C" int isg_topk_gumbel_bwd(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host,
                                   const int32_t *nmax_dev, const float *noise, uint64_t seed, const int32_t *graph_ids,
                                   int32_t k, float tau, const float *d_out, float *d_scores, void *stream) {
  int st = check_rows(scores, B, nmax_host, k, d_scores);
  if (st != ISG_OK) return st;
  if (B == 0 || nmax_host == 0) return ISG_OK;
  if (!(tau > 0.f) || !d_out) return ISG_EINVAL;
  RowArgs a{scores, ptr, nmax_dev, noise, nullptr, nullptr, (int)B, nmax_host, k, tau, 0.f, seed, graph_ids, nullptr};
  return launch_topk_gumbel_bwd<false>(a, d_out, d_scores, as_stream(stream));
}
