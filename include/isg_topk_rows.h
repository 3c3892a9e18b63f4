/* Top-k samplers with a node budget per graph: k read per row instead of one k for the batch (csrc/isg_topk_rows.hip).
 *
 * Tenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `stream` =
 * hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its own: none of the other
 * headers moves when an entry point here does.
 *
 * The three sampler entry points are isg_topk_threshold, isg_topk_gumbel and isg_topk_gumbel_bwd of isg.h with `k_rows` (device,
 * int32 [B], required) and `k_cap` in place of `k`.  Row b runs the scalar entry point's arithmetic with
 * k = clamp(k_rows[b], 0, k_cap): the same kernels (csrc/isg_topk.hpp), one load per wave more, so row b's bits are the bits the
 * scalar entry point gives that row at k = k_rows[b].  Everything else is as isg.h says: ragged rows with ptr int32 [B + 1] or
 * ptr == NULL and dense [B, nmax]; nmax_host / nmax_dev; the 0.0 pads of a ragged row take part in the selection; explicit noise
 * or the Philox stream keyed by (seed, graph_ids ? graph_ids[b] : b, j); khot_out / dense_out.  The clamp is there so that a bad
 * entry can neither run a loop past k_cap nor index LDS out of range; callers pass entries in [1, k_cap].  k_cap sizes what k
 * sized.
 */
#ifndef ISG_TOPK_ROWS_H
#define ISG_TOPK_ROWS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_TOPK_ROWS_ABI_VERSION 1

int isg_topk_rows_abi_version(void);

/* k_rows[b] = min(k_cap, max(k_min, (int)ceilf(ratio * (float)n_b))), n_b = ptr[b + 1] - ptr[b]: a share of each graph's nodes,
 * between k_min and k_cap.  ptr: int32 [B + 1]; k_rows: int32 [B].  The product is ONE fp32 multiplication, rounded to nearest and
 * never contracted: torch.ceil(torch.tensor(ratio, dtype=torch.float32) * n.float()).  One launch, nothing is read back.
 * ISG_EINVAL unless 0 < ratio (a NaN is refused), 1 <= k_min <= k_cap, B >= 0 and, for B > 0, both pointers non-null;
 * ISG_EUNSUPPORTED for B >= 2^31.  B == 0: ISG_OK, nothing launched. */
int isg_topk_budget(const int32_t *ptr, int64_t B, float ratio, int32_t k_min, int32_t k_cap, int32_t *k_rows, void *stream);

/* isg_topk_threshold with a k per row.  ISG_EINVAL as isg_topk_threshold (k_cap for k) and for k_rows == NULL where a launch
 * would follow. */
int isg_topk_threshold_rows(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host, const int32_t *nmax_dev,
                            const float *noise, float noise_scale, uint64_t seed, const int32_t *graph_ids,
                            const int32_t *k_rows, int32_t k_cap, float *out, float *dense_out, void *stream);

/* isg_topk_gumbel with a k per row. */
int isg_topk_gumbel_rows(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host, const int32_t *nmax_dev,
                         const float *noise, uint64_t seed, const int32_t *graph_ids, const int32_t *k_rows, int32_t k_cap,
                         float tau, float *out, float *khot_out, void *stream);

/* isg_topk_gumbel_bwd with a k per row.  k_cap is the stride of the LDS history: ISG_EUNSUPPORTED unless
 * k_cap * slots * 64 <= 4096, slots = 1, 2, 4, 8, 16 for nmax_host <= 64, 128, 256, 512, 1024 (the scalar entry point's rule at
 * k = k_cap, whatever the rows hold). */
int isg_topk_gumbel_rows_bwd(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax_host, const int32_t *nmax_dev,
                             const float *noise, uint64_t seed, const int32_t *graph_ids, const int32_t *k_rows,
                             int32_t k_cap, float tau, const float *d_out, float *d_scores, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_TOPK_ROWS_H */
