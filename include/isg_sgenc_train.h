/* Training of the scene-graph encoder without its concatenations: the backward kernels of isg_gather_add, isg_scatter_mean and
 * isg_graph_norm, and the segment sum every scatter-shaped gradient of that walk goes through (csrc/isg_sgenc_bwd.hip).
 *
 * Fifth device header of libisg_hip.so, beside include/isg.h (whose status codes and conventions hold here: caller-owned device
 * buffers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws,
 * nothing reads the device from the host, every call can sit in a captured stream).  It has an ABI version of its own.
 * No kernel here uses an atomic in global memory: two identical calls give the same bits.
 */
#ifndef ISG_SGENC_TRAIN_H
#define ISG_SGENC_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_SGENC_TRAIN_ABI_VERSION 1

int isg_sgenc_train_abi_version(void);

/* out[s, :] = sum over t in [rowptr[s], rowptr[s+1]) of w[eid[t]] * G[eid[t] / gdiv, :]      for s in [0, S)
 *
 * A CSR over S segments (rowptr int32[S+1] with rowptr[0] = 0 and rowptr[S] = M, eid int32[M], entries in ascending id inside a
 * segment) over fp32 rows G[*, C] of stride ldg.  w (optional) is one fp32 factor per ENTRY id; gdiv >= 1 lets one row of G serve
 * gdiv consecutive entry ids (the token slots of a node).  `skip` names a segment whose row is written as zeros whatever it holds
 * (padding_idx), or is -1.  Empty segments are written as zeros.  out has stride ldo: it may be a column slice of a wider tensor.
 *
 * The slot range [0, M) is cut into pieces of isg_segment_rows_chunk() slots.  Sixteen lanes walk a piece in slot order, store the
 * segments that lie wholly inside it and leave at most two partial rows in `ws` for the segments that cross its ends; a second
 * launch over the segments writes the zeros and adds each crossing segment's partial rows in piece order.  The order of every sum
 * is a function of the CSR and the piece length alone.  ws: isg_segment_rows_ws_bytes(M, C) bytes, 16-byte aligned.
 * ISG_EUNSUPPORTED unless 4 | C, 4 | ldg, 4 | ldo, 16-byte aligned rows, M < 2^31 and S < 2^31. */
int isg_segment_rows_sum(const int32_t *rowptr, const int32_t *eid, const float *w, const float *G, int32_t ldg, int32_t gdiv,
                         float *out, int32_t ldo, int64_t S, int64_t M, int32_t C, int64_t skip, void *ws, int64_t ws_bytes,
                         void *stream);
int32_t isg_segment_rows_chunk(void);
int64_t isg_segment_rows_ws_bytes(int64_t M, int32_t C);

/* The backward of isg_gather_add down to its pre-activation.  Nothing is saved but the inputs: with the forward's own statements
 *     z[e] = A[ia[e]] + B[ib[e]] + sign[e] * T[it[e]] + D[e] + bias                       (operands and limits of isg_gather_add)
 * is evaluated again and dz[e] = d_out[e] * gelu'(z[e]) (the exact-GELU derivative; d_out itself at act == 0) is written as
 * [E, C] rows of stride lddz.  dz IS the gradient of D; the gradients of A, B and T are isg_segment_rows_sum of dz over the CSRs
 * of ia, ib and it (T's with w = sign).  The gradient of bias leaves as ONE PARTIAL ROW PER WORKGROUP, fp32
 * [isg_gather_add_bwd_parts(E), C] (d_bias_part optional), which the caller sums over the parts in fixed order.  sign and the
 * index arrays get no gradient. */
int isg_gather_add_bwd(const float *A, const int64_t *ia, int32_t lda, const float *B, const int64_t *ib, int32_t ldb, const float *T,
                       const int64_t *it, const float *sign, int32_t ldt, const float *D, int32_t ldd, const float *bias,
                       const float *d_out, int32_t lddo, float *dz, int32_t lddz, float *d_bias_part, int64_t E, int32_t C,
                       int32_t act, void *stream);
int32_t isg_gather_add_bwd_parts(int64_t E);

/* The backward of isg_scatter_mean: d_msg[e] = d_out[dst[e]] / max(deg(dst[e]), 1) with deg(i) = rowptr[i+1] - rowptr[i] of the
 * CSR by destination the forward summed over (dst int64[E]: edge_index[1]).  4 | C, 4 | ld*, 16-byte aligned rows. */
int isg_scatter_mean_bwd(const float *d_out, int32_t lddo, const int64_t *dst, const int32_t *rowptr, float *d_msg, int32_t lddm,
                         int64_t N, int64_t E, int32_t C, void *stream);

/* The backward of isg_graph_norm in both of its modes: one workgroup per graph (any graph size) recomputes the graph's statistics
 * per channel, writes d_x [N, C] and leaves [d weight | d bias | d mean_scale] as one partial row per graph in `partial`
 * ([B, 3, C]; fp32, or doubles with accumulate_fp64, where all arithmetic is in double and d_x is rounded once, like the forward's
 * result).  The caller sums the partial rows in graph order.  An empty graph writes zero partial rows.  Limits of isg_graph_norm. */
int isg_graph_norm_bwd(const float *x, const int32_t *ptr, const float *weight, const float *mean_scale, double eps,
                       int32_t accumulate_fp64, const float *d_out, float *d_x, void *partial, int64_t B, int32_t C, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_SGENC_TRAIN_H */
