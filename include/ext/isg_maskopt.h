/* Mask optimisation (GNNExplainer, Ying et al. 2019, as PyG's GNNExplainer states it for an object-level node mask): ONE
 * iteration's arithmetic between the model's backward and its next forward as ONE launch (csrc/isg_maskopt.hip); DESIGN.md 37.
 * One logit theta[n] per row; the model reads sigmoid(theta[n]) * x[n, :] in place of x[n, :]; the launch turns the gradient
 * rows of the masked rows into d theta (row dot, sigmoid's derivative, the size and entropy regularisers of the row's segment),
 * takes one Adam step on theta and writes the next masked rows.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_maskopt.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative
 * ISG_E* status, nothing throws).  It has an ABI version of its own.
 *
 * No atomics, no LDS.  Every output word has one writer.  Two calls give the same bits.  Every number read from memory that
 * becomes an address is compared first; what fails the comparison is skipped and never used as an address.  rn(.) is ONE fp32
 * operation rounded to nearest (a division and a square root included: both are the correctly rounded ones); the function uses NO
 * fma, and nothing is contracted.
 *
 * KNOWN ANSWER (tests/maskopt_restated.py, smoke()).  One graph of 2 nodes (seg = [0, 2]), C = 4; theta = [0, 0], both moments 0,
 * x = [[1, 2, 3, 4], [-1, 0, 1, 2]], g = [[1, 1, 1, 1], [2, 0, -2, 4]]; a_size = 1, a_ent = 0.1, lr = 0.01, beta1 = 0.9,
 * beta2 = 0.999, eps = 1e-8, step 1 (bc1 = 0.1, bc2 = 0.001):
 *     s = [10, 4],  m = 0.5,  reg = (1 - 0.1 * 0) / 2 = 0.5
 *     d = [(10 + 0.5) * 0.25, (4 + 0.5) * 0.25] = [2.625, 1.125]            exactly
 *     theta_new = [-0.01, -0.01]                                            within 1e-9 (at step 1 Adam moves by lr d / (|d| + eps))
 *     x_out = sigmoid(-0.01) * x
 */
#ifndef ISG_MASKOPT_H
#define ISG_MASKOPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_MASKOPT_ABI_VERSION 1

int isg_maskopt_abi_version(void);

/* THE STEP.  x fp32 [N, C] row stride ldx: the unmasked rows.  g fp32 [N, C] row stride ldg: the gradient of the summed model
 * loss with respect to the MASKED rows (what the last call wrote to x_out); NULL: the apply-only form.  seg int32 [B + 1]: the
 * range starts of B contiguous segments of rows (a GraphPlan's ptr for node rows, the edge ranges for edge rows; PRECONDITION
 * for a right answer: non-decreasing).  theta, exp_avg, exp_avg_sq fp32 [N]: the logits and Adam's two moments, updated in
 * place.  x_out fp32 [N, C] row stride ldxo; it overlaps no input.  d_theta: optional (NULL: not wanted) fp32 [N].
 * The host scalars: a_size, a_ent (the regularisers' coefficients), lr, beta1, beta2, eps (Adam's), bc1 = 1 - beta1^step and
 * bc2 = 1 - beta2^step, computed by the caller in double from the step number (as isg_mt_adam's prologue does, isg_optim.h).
 * Each is rounded to fp32 ONCE, after the double arithmetic named here:  A = (float)a_size, E = (float)a_ent,
 * w1 = (float)(1 - beta1), b2 = (float)beta2, w2 = (float)(1 - beta2), step_size = (float)(lr / bc1), r2 = (float)sqrt(bc2),
 * e = (float)eps.
 *
 * For row n of segment j (seg[j] <= n < seg[j + 1]; j is found by a binary search over seg, the same words for all sixteen lanes
 * of the row), with n_j = seg[j + 1] - seg[j]:
 *     s[n]  = the sum over c of g[n, c] * x[n, c], IN isg_ig_attribution's ORDER (isg_ig.h): the channels in quads c = 4 k .. 4 k + 3;
 *                 a quad's value is p_k = rn(rn(rn(rn(g0 x0) + rn(g1 x1)) + rn(g2 x2)) + rn(g3 x3));
 *                 lane l of sixteen sums its quads k = l, l + 16, l + 32, ... ascending from +0, s_l = rn(s_l + p_k);
 *                 the sixteen s_l are combined by the xor-butterfly  s_l = rn(s_l + s_{l ^ 8}), then ^ 4, ^ 2, ^ 1
 *     m     = sigmoid(theta[n]) = rn(1 / rn(1 + expf(-theta[n])))
 *                 expf is the device library's exponential (__ocml_exp_f32; documented maximum error 1 ulp).  It overflows to
 *                 +inf (m = +0) and underflows to a number below 2^-24 (m = 1) long before |theta| = 90.
 *     reg   = rn(rn(A - rn(E * theta[n])) / (float)n_j)
 *                 the derivative of  a_size * mean sigmoid(theta) + a_ent * mean H(sigmoid(theta))  over the segment, divided by
 *                 sigmoid'(theta): d/dtheta H(sigmoid(theta)) = -theta * sigmoid'(theta) in closed form (H in nats)
 *     d[n]  = rn(rn(s[n] + reg) * rn(m * rn(1 - m)))
 *     Adam, in the statement order of isg_optim.h's (no weight decay, no clipping):
 *         exp_avg[n]    = rn(exp_avg[n] + rn(rn(d - exp_avg[n]) * w1))
 *         exp_avg_sq[n] = rn(rn(exp_avg_sq[n] * b2) + rn(rn(d * d) * w2))
 *         theta[n]      = rn(theta[n] - rn(step_size * rn(exp_avg[n] / rn(rn(rn(sqrt(exp_avg_sq[n])) / r2) + e))))
 *     x_out[n, c] = rn(sigmoid(theta_new[n]) * x[n, c])                      (sigmoid as above, on the updated logit)
 *     d_theta[n] = d[n], when given.
 * APPLY-ONLY FORM (g == NULL): theta and the moments are not written (exp_avg, exp_avg_sq and d_theta are not looked at) and
 * x_out[n, c] = rn(sigmoid(theta[n]) * x[n, c]).  The first iteration uses it, and the final forward.
 * A NON-FINITE d[n] (an inf or a NaN among the row's gradients, say) SKIPS the row's update: theta[n] and its moments stay as
 * they are, x_out is written from the unchanged theta[n]; d_theta[n], when given, still reports the value.
 * SATURATION: theta = +-90 gives m = 1 or +0 and, for a finite s, d = 0 -- never a NaN.
 * A ROW OUTSIDE EVERY SEGMENT (n < seg[0], n >= seg[B], or seg not covering it) leaves every output of that row unwritten.  seg
 * is read at [0, B] only, and compared before use: a bad range never becomes an address.
 * Work mapping: sixteen lanes per row, 16 bytes per lane and access, 256-thread workgroups; the sixteen lanes compute the row's
 * scalars alike, lane 0 stores them.  Bandwidth-bound on the rows of x (read twice, the second time from cache), g and x_out.
 * ISG_EINVAL: a negative count; with rows (N > 0): a width < 1, a stride of x / g / x_out below the width, a missing x, seg,
 * theta or x_out, B == 0; with g given: a missing exp_avg or exp_avg_sq, a bc1 or bc2 that is not > 0.
 * ISG_EUNSUPPORTED: a width or stride that is no multiple of 4 or a row pointer (x, g, x_out) that is not 16-byte aligned, with
 * rows; a count (N, B) of 2^31 - 1024 or more.  N == 0: ISG_OK, nothing is written. */
int isg_maskopt_step(const float *x, int32_t ldx, const float *g, int32_t ldg, const int32_t *seg, int64_t B,
                     float *theta, float *exp_avg, float *exp_avg_sq, float *x_out, int32_t ldxo, float *d_theta,
                     int64_t N, int32_t C, double a_size, double a_ent, double lr, double beta1, double beta2, double eps,
                     double bc1, double bc2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_MASKOPT_H */
