/* Training of the samplers: the backward of the SIMPLE sampler's exact marginals as one launch (csrc/isg_simple_bwd.hip).
 *
 * Ninth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `stream` =
 * hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its own: none of the other
 * headers moves when an entry point here does.
 *
 * isg_simple_topk (include/isg.h) returns out = (sample - marg).detach() + marg with marg[i] = exp(M(0, i, 1)), M the top-down
 * log-marginals of the exactly-k circuit.  d out / d marg = 1 and the sample carries no gradient, so the backward takes neither the
 * uniform draw nor a seed.  It reads nothing of the forward but the scores: one wave per row rebuilds the circuit's two trees in LDS
 * with the forward's own arithmetic and reverses them.  No atomic adds: two launches agree bit for bit.
 */
#ifndef ISG_SAMPLER_TRAIN_H
#define ISG_SAMPLER_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_SAMPLER_TRAIN_ABI_VERSION 1

int isg_sampler_train_abi_version(void);

/* Host only, no device is touched.  The LDS bytes one row of isg_simple_topk_bwd takes: four trees (W, M, dW, dM) of
 * (2n - 1)(kk + 1) floats, n = nmax rounded up to a power of two, kk = min(k, nmax).  ISG_EINVAL for k <= 0 or nmax < 0; 0 for
 * nmax == 0; ISG_EUNSUPPORTED for nmax > 1024, kk > 16 or a row of more than 150 KiB.  One 256-thread workgroup takes as many rows,
 * one wave each, as fit in 48 KiB: at most 4, at least 1.  The launch decides both by the code behind this function. */
int64_t isg_simple_topk_bwd_row_bytes(int32_t k, int32_t nmax);

/* d_scores = d scores of isg_simple_topk for the gradients g_out of `out` and g_marg of `marg_out`.  scores / ptr / B / nmax / k as
 * isg_simple_topk takes them: ragged rows with ptr int32 [B + 1], or ptr == NULL and dense [B, nmax]; nmax the longest row.
 * g_out: the layout of scores, may be NULL (= 0).  g_marg: dense [B, nmax], may be NULL (= 0); on a ragged row its entries at and
 * behind the row's length feed the circuit (the zero pads have marginals) and produce no output.  d_scores: the layout of scores,
 * every entry written.  B == 0 or nmax == 0: ISG_OK, nothing launched.  ISG_EUNSUPPORTED where isg_simple_topk_bwd_row_bytes
 * refuses the shape: the caller differentiates the torch restatement instead. */
int isg_simple_topk_bwd(const float *scores, const int32_t *ptr, int64_t B, int32_t nmax, int32_t k, const float *g_out,
                        const float *g_marg, float *d_scores, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_SAMPLER_TRAIN_H */
