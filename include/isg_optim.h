/* The tail of a training or validation step on the device: softmax cross-entropy with top-1 and running meters, the global
 * gradient norm with torch's clipping coefficient, and Adam over a table of tensors (csrc/isg_optim.hip).
 *
 * Third device header of libisg_hip.so, beside include/isg.h and include/isg_train.h (the status codes and conventions of isg.h
 * hold: raw device pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status,
 * nothing throws).  It has an ABI version of its own: neither of the other two headers moves when an entry point here does.
 *
 * Nothing here returns a device value to the host, and no kernel uses an atomic in global memory: every sum runs in one fixed
 * order (lanes, then the waves of a workgroup, then workgroups / rows / chunks ascending inside ONE finishing workgroup), so two
 * identical calls give the same bits.  Doubles are written with ordinary vector stores.
 *
 * THE TENSOR TABLE of the two isg_mt_* entry points: `table` is a device int64 [T][4] of the addresses of (param, grad, exp_avg,
 * exp_avg_sq) of T fp32 tensors, contiguous and 4-byte aligned (nothing more is assumed: a kernel takes a scalar head up to the
 * first 16-byte boundary, a float4 body and a scalar tail); `numel` is a device int64 [T]; `chunk_prefix` is a device int64
 * [T + 1] with chunk_prefix[t + 1] - chunk_prefix[t] = ceil(numel[t] / isg_mt_chunk_elems()) -- chunk_prefix[0] need not be 0,
 * so a group of consecutive rows of a longer table is addressed by offsetting the three pointers.  `total_chunks` is
 * chunk_prefix[T] - chunk_prefix[0], known to the host because the sizes are.  Work is cut into these chunks; a workgroup finds
 * the tensor of a chunk by bisecting chunk_prefix; the grid is capped (2048 workgroups) and strides over the rest.  T = 0 and
 * tensors of numel 0 are allowed.  isg_mt_sqnorm reads column 1 of the table only.
 */
#ifndef ISG_OPTIM_H
#define ISG_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_OPTIM_ABI_VERSION 1

int isg_optim_abi_version(void);

/* Slots of the running meters `totals` (double [8]) that isg_xent_fwd and isg_mt_adam update in place. */
#define ISG_TOT_LOSS_SUM 0     /* sum of mean_loss * n_rows over the calls whose mean_loss was finite */
#define ISG_TOT_LOSS_ROWS 1    /* sum of n_rows over those calls */
#define ISG_TOT_CORRECT 2      /* sum of n_correct */
#define ISG_TOT_ROWS 3         /* sum of n_rows */
#define ISG_TOT_CALLS 4        /* isg_xent_fwd calls */
#define ISG_TOT_NONFINITE 5    /* ... of which mean_loss was NaN or infinite */
#define ISG_TOT_SKIPPED 6      /* optimizer steps skipped for a nonfinite gradient norm (isg_mt_adam) */
#define ISG_TOT_RESERVED 7

/* Softmax cross-entropy and top-1 over fp32 logits [B, A] (row stride ld >= A, rows only 4-byte aligned) and int64 labels [B].
 * Two launches.  Rows kernel, a wave per row:  row_lse[b] = max + log(sum exp(x - max)), kept in DOUBLE (lanes sum expf in fp32;
 * the lane totals, the logarithm and the addition of the fp32 max are double: rounded to fp32, logits near 1e4 would cost the
 * backward's exp(x - lse) four digits, and a 1-ulp logf a whole ulp of the loss);
 * row_loss[b] = (float)(row_lse[b] - x[label]);  pred[b] = the lowest index among the row's maxima.
 * A row whose label == ignore_index has loss 0 and is neither counted nor correct; any other label outside [0, A) makes
 * row_loss NaN (a counted row: the mean goes NaN and the step is seen as nonfinite; nothing is reported to the host).
 * Finishing kernel, one workgroup, rows ascending, sums in double:
 *   stats = {mean_loss = sum row_loss over counted rows / n_counted (0 / 0 = NaN when none is), n_counted, n_correct, n_rows}.
 * loss (optional): mean_loss once more, rounded to fp32 -- the scalar a caller hands on to autograd.
 * totals (optional): the ISG_TOT_* slots 0-5 above are advanced by this call; the loss sum takes the fp32 loss times n_rows,
 * which is the reference's AverageMeter.update(loss.item(), batch_size).
 * ISG_EINVAL: B < 0, A < 1, ld < A, a null required pointer with B > 0.  ISG_EUNSUPPORTED: B >= 2^31.  At B == 0 only the
 * finishing kernel runs (mean_loss = NaN, counts 0). */
int isg_xent_fwd(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, float *row_loss, double *row_lse,
                 int32_t *pred, double *stats, float *loss, double *totals, int64_t B, int32_t A, void *stream);

/* d_logits[b, a] = (exp(x[b, a] - row_lse[b]) - [a == label[b]]) * g / n_counted for counted rows, 0 for ignored rows, NaN for a
 * row whose label is outside [0, A); recomputed from logits, row_lse and stats (n_counted = stats[1]) in one pass over the logits.
 * g (optional): a device fp32 scalar, the upstream gradient; NULL = 1.  d_logits has row stride ldd >= A. */
int isg_xent_bwd(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, const double *row_lse,
                 const double *stats, const float *g, float *d_logits, int32_t ldd, int64_t B, int32_t A, void *stream);

/* Elements of one chunk of the tensor table, and the doubles isg_mt_sqnorm's `parts` must hold for a table of total_chunks. */
int32_t isg_mt_chunk_elems(void);
int64_t isg_mt_sqnorm_parts(int64_t total_chunks);

/* The global L2 norm of the table's gradients.  Two launches: a chunk's lanes accumulate g * g in fp32 (at most 16 + 1 terms
 * each), the lanes' totals are added in double and written as ONE double per chunk (parts[chunk]); a finishing workgroup sums
 * the parts in double, chunks ascending, and writes
 *   clip = {norm, coef, finite, 0} (float [4]):  coef = min(1, max_norm / (norm + 1e-6)) in fp32, torch's clip_grad_norm_ rule;
 *   coef = 1 when max_norm <= 0 (no clipping);  finite = 1 iff norm is finite.
 * The gradients are not changed: isg_mt_adam applies coef.  At total_chunks == 0 only the finishing kernel runs (norm 0). */
int isg_mt_sqnorm(const int64_t *table, const int64_t *numel, const int64_t *chunk_prefix, int32_t T, int64_t total_chunks,
                  double *parts, float max_norm, float *clip, void *stream);

/* One Adam step over the table, torch's _single_tensor_adam in its statement order (amsgrad is not built).  Two launches.
 * Prologue, one thread: reads clip[2] (clip optional: NULL = no norm was taken, the step always applies) and the device double
 * counter *step.  When the step applies and `advance` != 0, *step += 1; then bc1 = 1 - beta1^step and bc2 = 1 - beta2^step, in
 * double, go to state = {bc1, bc2, applies (1 or 0), step} (double [4]).  When it does not apply, state[2] = 0 and, with
 * `advance` != 0, *skipped += 1 (a device double: slot ISG_TOT_SKIPPED of a totals block, or a counter of the caller's own).
 * A caller with several param groups sets `advance` on the first group's call only: the later ones see the advanced counter.
 * Update, skipped as a whole when state[2] == 0 (params, both moments and the counter keep their bits), else per element
 *   g = grad * coef (coef = clip[1], or 1);   L2 mode: g += wd * p;   decoupled mode: p *= 1 - lr * wd;
 *   m += (g - m) * (1 - beta1);   v = v * beta2 + g * g * (1 - beta2);   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
 * lr, the betas, eps, wd and the mode are host scalars of THIS call.  16 B read and 12 B written per element: float4 accesses
 * where the four tensors of a row share their misalignment (separate allocations always do), scalar ones elsewhere. */
int isg_mt_adam(const int64_t *table, const int64_t *numel, const int64_t *chunk_prefix, int32_t T, int64_t total_chunks,
                const float *clip, double *step, double *state, double *skipped, int32_t advance, double lr, double beta1,
                double beta2, double eps, double wd, int32_t decoupled, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_OPTIM_H */
