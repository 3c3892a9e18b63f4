/* Integrated gradients (Sundararajan et al. 2017) on a batch of graph instances: the rows of S points on the straight path from a
 * baseline to the input as ONE instance batch, and the gradient rows of that batch reduced to one attribution per row of the
 * parent batch (csrc/isg_ig.hip); DESIGN.md 36.  Gradient x input is the one-point special case (S = 1, t = 1, w = 1).
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_ig.py on the same handle.  The status codes and conventions
 * of isg.h hold (device pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E*
 * status, nothing throws).  It has an ABI version of its own.
 *
 * No atomics.  Every output word has one writer.  Two calls give the same bits.  Every number read from memory that becomes an
 * address is compared first; what fails the comparison is skipped and never used as an address.  rn(.) is ONE fp32 operation
 * rounded to nearest; fma(a, b, c) is ONE fused multiply-add; nothing else is contracted.
 *
 * KNOWN ANSWER (tests/ig_restated.py, smoke()).  One graph of 2 nodes, C = 4, no edges; S = 2 instances of it, t = [0.25, 0.75],
 * w = [0.5, 0.5]; x = [[1, 2, 3, 4], [-1, 0, 1, 2]], baseline one row b = [1, 0, 1, 0]:
 *     path rows   = [[1, 0.5, 1.5, 1], [0.5, 0, 1, 0.5], [1, 1.5, 2.5, 3], [-0.5, 0, 1, 1.5]]
 * and with the gradient rows g = [[1, 1, 1, 1], [2, 0, -2, 4], [3, -1, 1, 0.5], [0, 2, 2, -4]] of those four rows:
 *     G           = [[2, 0, 1, 0.75], [1, 1, 0, 0]]            (G[0] = 0.5 g[0] + 0.5 g[2],  G[1] = 0.5 g[1] + 0.5 g[3])
 *     x - b       = [[0, 2, 2, 4], [-2, 0, 0, 2]]
 *     attribution = [0*2 + 2*0 + 2*1 + 4*0.75, -2*1 + 0*1 + 0*0 + 2*0] = [5, -2]
 */
#ifndef ISG_IG_H
#define ISG_IG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_IG_ABI_VERSION 1

int isg_ig_abi_version(void);

/* THE PATH ROWS: isg_instance_rows (include/isg_instances.h) with an interpolation.  ONE launch for the node half and the edge
 * half: sixteen lanes per OUTPUT row, 16 bytes per lane and access, rows independent.
 * For instance row i < n_out with source row r = node_src[i] and instance q = inst_of[i] (the instance batch's `batch`), c < Cx:
 *     x_out[i, c] = fma(t[q], x[r, c], rn(rn(1 - t[q]) * b_x[r * ldbx + c]))          b_x given
 *     x_out[i, c] = rn(t[q] * x[r, c])                                                 b_x == NULL (a baseline of zeros)
 * t fp32 [Q].  b_x: NULL, ONE row [Cx] for every source row (ldbx == 0), or rows [x_rows, Cx] with row stride ldbx >= Cx.
 * For finite x and b_x, t[q] == 0 gives the bits of the baseline row and t[q] == 1 the bits of x's row (but for a negative zero
 * met by a positive one, whose sum is +0).
 * The edge half is the same with e, b_e / ldbe, edge_src, einst_of, m_out, e_out, Ce.  path_e == 0 makes the edge half a plain
 * copy, e_out[j, :] = e[edge_src[j], :]: the edge rows stay at the input, and b_e and einst_of are not looked at.
 * A source row number outside [0, x_rows) / [0, e_rows), or (where the half is interpolated) an instance number outside [0, Q),
 * leaves its output row unwritten.  Either half may be empty (n_out == 0 / m_out == 0: its pointers are not looked at).
 * ISG_EINVAL: a negative count; in a half that has rows: a width < 1, a stride of x / x_out below the width, a missing x,
 * node_src or x_out, a baseline stride that is negative or, where it is not 0, below the width; in an INTERPOLATED half that
 * has rows: a missing t or inst_of (einst_of).
 * ISG_EUNSUPPORTED: a width or stride that is no multiple of 4 or a row pointer (x, x_out, b_x) that is not 16-byte aligned in a
 * half that has rows; a count (n_out, m_out, Q) of 2^31 - 1024 or more.  n_out == 0 and m_out == 0: ISG_OK, nothing is written. */
int isg_ig_path_rows(const float *x, int32_t ldx, int64_t x_rows, const float *b_x, int32_t ldbx, const int64_t *node_src,
                     const int64_t *inst_of, int64_t n_out, float *x_out, int32_t ldxo, int32_t Cx,
                     const float *e, int32_t lde, int64_t e_rows, const float *b_e, int32_t ldbe, const int64_t *edge_src,
                     const int64_t *einst_of, int64_t m_out, float *e_out, int32_t ldeo, int32_t Ce,
                     const float *t, int64_t Q, int32_t path_e, void *stream);

/* THE ATTRIBUTION.  With the names of isg_instance_rows_bwd (include/ext/isg_instances_train.h) -- ptr[g] the node range of graph
 * g, erange[g] its edge range, inst_ptr / inst_eptr the node / edge ranges of the Q instances, glist[gptr[g] .. gptr[g + 1]) the
 * instances of graph g in ascending q -- and w fp32 [Q] the quadrature weight of every instance: for node n of graph g
 *     G[n, c]   = the fma chain  acc = +0;  for j = gptr[g] .. gptr[g + 1] - 1 ascending, q = glist[j]:
 *                     acc = fma(w[q], g_xo[inst_ptr[q] + (n - ptr[g]), c], acc)
 *     d[n, c]   = rn(x[n, c] - b_x[n * ldbx + c])          (b_x == NULL: d = x;  ldbx == 0: ONE baseline row)
 *     attr_x[n] = the sum over c of d[n, c] * G[n, c], IN THIS ORDER: the channels in quads c = 4 k .. 4 k + 3; a quad's value is
 *                     p_k = rn(rn(rn(rn(d0 G0) + rn(d1 G1)) + rn(d2 G2)) + rn(d3 G3));
 *                 lane l of sixteen sums its quads k = l, l + 16, l + 32, ... ascending from +0, s_l = rn(s_l + p_k);
 *                 the sixteen s_l are combined by the xor-butterfly  s_l = rn(s_l + s_{l ^ 8}), then ^ 4, ^ 2, ^ 1
 *                 (after which all sixteen hold the same bits).
 * avg_x (optional, NULL: not wanted) fp32 [x_rows, Cx] row stride ldax receives the rows G[n, :].
 * accumulate != 0: attr_x[n] = rn(attr_x[n] + the sum) and avg_x[n, c] = rn(avg_x[n, c] + G[n, c]) -- one fp32 add onto what
 * the caller hands in; the attribution is linear in the copies, so a path forwarded in chunks adds up.
 * The edge half is the same with g_eo, e, b_e, attr_e [e_rows], avg_e, erange and inst_eptr; e_rows == 0 skips it.
 * EVERY row of attr_x / attr_e (and avg) is written: a row with no copy that passes the rules below -- its graph has no
 * instance, or no graph's range holds it -- is +0, or left unchanged under accumulate.
 * The skip rules are those of isg_instance_rows_bwd: a graph's range in glist is clamped to [0, Q]; an instance number outside
 * [0, Q), an instance range that is negative or too short for the row's offset, and a copy's row number outside [0, xo_rows) /
 * [0, eo_rows) are compared and that copy is skipped.  ptr and erange are read at [0, G] only (PRECONDITION for a right answer:
 * both non-decreasing).
 * Work mapping: sixteen lanes per output row; per quad a lane walks the copies with four 16-byte loads in flight (unrolled
 * over j, a remainder loop behind); one lane stores the attribution.  Bandwidth-bound on the N' C 4 bytes of g_xo, read once.
 * ISG_EINVAL: a negative count; in a half that has rows: a width < 1, a stride of g / x / avg below the width, a baseline stride
 * that is negative or, where it is not 0, below the width, G == 0, a missing attr / x / ptr (erange) / inst_ptr (inst_eptr) /
 * gptr, a missing g_xo with xo_rows > 0 (g_eo, eo_rows), a missing glist or w with Q > 0.
 * ISG_EUNSUPPORTED: a width or stride that is no multiple of 4 or a row pointer (g, x, b, avg) that is not 16-byte aligned in a
 * half that has rows; a count (rows, G, Q) of 2^31 - 1024 or more.  x_rows == 0 and e_rows == 0: ISG_OK, nothing is written. */
int isg_ig_attribution(const float *g_xo, int32_t ldgx, int64_t xo_rows, const float *x, int32_t ldx, const float *b_x, int32_t ldbx,
                       float *attr_x, float *avg_x, int32_t ldax, int64_t x_rows, int32_t Cx,
                       const float *g_eo, int32_t ldge, int64_t eo_rows, const float *e, int32_t lde, const float *b_e, int32_t ldbe,
                       float *attr_e, float *avg_e, int32_t ldae, int64_t e_rows, int32_t Ce,
                       const float *w, const int32_t *ptr, const int32_t *erange, const int32_t *inst_ptr, const int32_t *inst_eptr,
                       const int32_t *gptr, const int32_t *glist, int64_t G, int64_t Q, int32_t accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_IG_H */
