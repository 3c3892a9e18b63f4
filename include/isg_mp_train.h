/* Attention dropout for training the GATv2 message-passing operator: a seeded forward and the backward that draws the mask again
 * (csrc/isg_mp.hip, csrc/isg_mp_graph.hip, csrc/isg_mp_bwd.hip).
 *
 * Eleventh device header of libisg_hip.so (the status codes and conventions of isg.h hold: fp32 device pointers, `ld*` = row
 * stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version
 * of its own: none of the other headers moves when an entry point here does.
 *
 * THE FUNCTION.  The reference drops attention weights between the softmax and the aggregation
 * (alpha = F.dropout(alpha, p, training), ISubGVQA/models/mgat_v2_conv.py:274-279).  For the edge with ORIGINAL edge id e (its
 * column in edge_index, the `eid` of a CSR slot) and head h, under a 64-bit `seed` and a drop probability 0 <= p < 1:
 *     r(e, h) = keep(e, h) * (1.0f / (1.0f - p))
 *     keep(e, h) = the keep rule of include/isg_train.h with i = e, j = h: kept iff
 *         uniform24(word[h & 3] of philox4x32_10((e, h >> 2, 0x1571, 0x9E37), (seed & 0xffffffff, seed >> 32))) >= p
 *     compared in fp32.  One Philox block serves four heads of an edge.
 * Logits and softmax are those of isg_gatv2_mp_fwd; out[i] = sum_e x_l[j] * ((alpha_e * r_e) * m_e) (+ bias), in the slot order of
 * the kernel that runs.  The key is the edge id, not the CSR slot: the mask does not depend on which kernel a shape selects nor on
 * the order of a plan, and a permutation of edge_index permutes the mask with it.
 * No mask is stored; the backward regenerates it.  No kernel uses an atomic: two identical calls give the same bits.
 * At p == 0 nothing is drawn and both calls ARE the launches of isg_gatv2_mp_fwd / isg_gatv2_mp_bwd, bit for bit.
 */
#ifndef ISG_MP_TRAIN_H
#define ISG_MP_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_MP_TRAIN_ABI_VERSION 1

int isg_mp_train_abi_version(void);

/* isg_gatv2_mp_fwd (isg.h: operands, strides, the per-graph arrays, limits and ISG_EUNSUPPORTED cases are the same, and the same
 * kernel runs a given shape) with dropout on the attention weights.  `alpha` [E, H] is required and receives the softmax BEFORE
 * dropout, the bits isg_gatv2_mp_fwd writes on the same inputs; `out` is aggregated from the dropped weights.
 * ISG_EINVAL unless 0 <= p < 1 (a NaN is refused) and alpha != NULL, before anything else is looked at. */
int isg_gatv2_mp_fwd_dropout(const float *x_l, const float *x_r, const float *e_proj, const float *att, const float *bias,
                             const int32_t *rowptr, const int32_t *eid, const int32_t *src, const float *node_mask,
                             const float *edge_mask, float *out, float *alpha, int64_t N, int64_t E, int32_t H, int32_t C,
                             float negative_slope, const int32_t *graph_ptr, const int32_t *graph_eptr, const int32_t *dst,
                             int64_t B, int32_t nmax_host, int32_t emax_host, int32_t ld_l, int32_t ld_r, int32_t ld_e, float p,
                             uint64_t seed, void *stream);

/* isg_gatv2_mp_bwd (isg.h: dense rows, the CSR by source, one partial row of d att per 16 destinations) of the call above with
 * the same (p, seed); `alpha` is what that call returned.  With g = d out_i:  dalpha_e = r_e m_e <g, x_l[j]>;  the term of
 * d m_e that comes through the aggregation is alpha_e r_e <g, x_l[j]>;  d x_l[j] takes (alpha_e r_e) m_e g.  S (both sums in
 * fp64), da_e, ds_e, d att, d x_r and d e_proj follow from those as in isg_gatv2_mp_bwd.
 * ISG_EINVAL unless 0 <= p < 1 (a NaN is refused). */
int isg_gatv2_mp_bwd_dropout(const float *x_l, const float *x_r, const float *e_proj, const float *att, const float *alpha,
                             const float *grad_out, const int32_t *rowptr, const int32_t *eid, const int32_t *src,
                             const int32_t *rowptr_s, const int32_t *eid_s, const int32_t *dst_s, const float *node_mask,
                             const float *edge_mask, float *d_x_l, float *d_x_r, float *d_e_proj, float *d_att_partial,
                             float *d_edge_mask, int64_t N, int64_t E, int32_t H, int32_t C, float negative_slope, float p,
                             uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_MP_TRAIN_H */
