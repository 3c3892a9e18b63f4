/* Fidelity curves (deletion and insertion curves of a node ranking): the two steps between an explainer's scores and the curves,
 * each as ONE launch (csrc/isg_curves.hip); DESIGN.md 38.  isg_curve_keep_bits ranks the nodes of every listed graph and writes
 * the nested keep sets of all levels and both sides as rows of keep bits for isg_induced_size / isg_induced_fill
 * (include/ext/isg_induced.h); isg_curve_sums reduces the predicted class's probability on those instances to the area under
 * every graph's curve and to running totals.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_curves.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers unless a parameter says HOST, `stream` = hipStream_t or NULL, ISG_OK or a negative
 * ISG_E* status, nothing throws).  It has an ABI version of its own.
 *
 * No atomics.  Every output word has one writer.  Two calls give the same bits.  Every number read from memory that becomes an
 * address is compared first; what fails the comparison is never used as an address.
 *
 * KNOWN ANSWER (tests/curves_restated.py, smoke()).  One graph of 3 nodes, a = [0.5, 2, 2], count = (1, 2), both sides (sides = 3),
 * W = 1:
 *     rank    = [2, 0, 1]                       (the tie at 2 goes to the lower node index)
 *     keep    = [0b010, 0b101, 0b110, 0b001]    (rows q = 0..3: level 0 keep, level 0 remove, level 1 keep, level 1 remove)
 *     level_k = [[1, 1], [2, 2]]
 *     index   = [0, 0, 0, 0]
 */
#ifndef ISG_CURVES_H
#define ISG_CURVES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_CURVES_ABI_VERSION 1

int isg_curve_abi_version(void);

/* RANKING, LEVEL SIZES AND ALL KEEP ROWS.  a fp32 [N]: a score per node, higher means more important.  ptr int32 [G + 1]: the
 * range starts of the G graphs' nodes.  graphs int32 [R]: the listed graphs.  Exactly one of frac (HOST fp32 [L]: a share of a
 * graph's nodes per level) and count (HOST int32 [L]: a number of nodes per level); the L values are copied into the launch.
 * sides: bit 0 = the keep side, bit 1 = the remove side; S = popcount(sides); the keep side comes first.  W: words of 32 keep
 * bits per row.
 * Outputs: rank int32 [N], written for the nodes of listed graphs only; level_k int32 [R, L, S]; index int32 [R L S];
 * keep uint32 [R L S, W]; status int32 [4].
 *
 * THE RANGE of listed graph g = graphs[r]:  lo = min(max(ptr[g], 0), N),  hi = max(min(max(ptr[g + 1], 0), N), lo): ptr is
 * clamped to [0, N] and to non-decreasing before use.  n = min(hi - lo, 32 W); the nodes with local index >= 32 W take no part:
 * they are neither ranked nor counted in n, their rank is not written, and status[0] is 1.
 * RANK.  For local node i < n:   rank[lo + i] = #{m < n : a[lo + m] > a[lo + i], or a[lo + m] = a[lo + i] and m < i}
 * (a graph listed twice has its ranks stored twice, the same values; listed graphs whose ranges OVERLAP -- a ptr that was not
 * non-decreasing -- store different ranks to the same words in no stated order: rank has one writer per word for a valid ptr)
 * where > is IEEE's with every NaN placed below -inf, NaNs equal among themselves and -0 = +0.  So the ranks of a graph are a
 * permutation of 0 .. n - 1, ties go to the lower node index, NaNs come last in node order.
 * LEVEL SIZE.  t_j = count[j], or t_j = (int)ceilf(rn(frac[j] * (float)n)): ONE fp32 multiplication rounded to nearest, never
 * contracted (isg_topk_budget's rule, isg_topk_rows.h); a product of n or more is n, never an out-of-range cast.
 *     the keep side:    k = min(n, max(1, t_j))            (the k best ranked nodes are the instance)
 *     the remove side:  k = min(n - 1, max(0, t_j))        (the k best ranked nodes are removed)
 * so for n >= 1 no instance is empty.  n == 0: k = 0 and the rows are zero.
 * ROWS.  q = (r L + j) S + s;  index[q] = graphs[r];  level_k[q] = k;  bit i & 31 of word i >> 5 of row q is (rank[lo + i] < k)
 * on the keep side and its negation on the remove side, for i < n; bits at or beyond n are 0; all W words of a row are written.
 * A graphs[r] outside [0, G) gives zero rows and level_k = 0 (index[q] still reports the entry) and status[1] is 1; it is never
 * used as an address.
 * status = [a listed graph has more than 32 W nodes, an entry of graphs is outside [0, G), R L S, 0], all four words written.
 *
 * Work mapping: one 64-lane wave per listed graph.  The graph's scores are staged in LDS as order-preserving uint32 keys (-0
 * canonicalised to +0, NaN the smallest key; 128 W bytes); lane l owns nodes l, l + 64, ... and counts over the whole graph from
 * LDS, every lane reading the same words (a broadcast): n^2 / 64 steps per lane.  The ranks go back to LDS (another 128 W bytes);
 * a row's words come from one 64-bit ballot per 64 nodes, stored by two lanes.  Wave 0 also reads all of graphs and writes status.
 *
 * Checked in this order.  ISG_EINVAL: a negative N, G, R or L; sides outside 1..3; W < 1; with L > 0: both or neither of frac and
 * count.  ISG_EUNSUPPORTED: W > 64; L > 64; N, G or R L S of 2^31 - 1024 or more.  ISG_EINVAL: a NaN or negative frac[j], a
 * negative count[j].  Then R == 0 or L == 0: ISG_OK, nothing is written.  ISG_EINVAL: a missing ptr, graphs, level_k, index, keep
 * or status; with N > 0 a missing a or rank. */
int isg_curve_keep_bits(const float *a, const int32_t *ptr, const int32_t *graphs, const float *frac, const int32_t *count,
                        int64_t N, int64_t G, int64_t R, int64_t L, int32_t sides, int32_t W, int32_t *rank, int32_t *level_k,
                        int32_t *index, uint32_t *keep, int32_t *status, void *stream);

/* INSTANCE PROBABILITIES TO CURVES, AREAS AND RUNNING TOTALS.  p_inst fp32 [R L S]: the predicted class's probability on every
 * instance, in the row order above (q = (r L + j) S + s).  w fp32 [L]: quadrature weights over the nominal level axis, formed by
 * the caller in double and rounded once.  sides as above (only S = popcount matters).
 * auc fp32 [R, S]:  auc[r, s] = the chain  v = +0;  v = fmaf(w[j], p[r, j, s], v)  for j ascending.
 * totals double [S, L + 3], ACCUMULATED INTO; per side: L sums of p over the counted graphs (one per level), the sum of auc over
 * the counted graphs, the graphs counted, the graphs skipped.
 * A graph with a non-finite p at any level of a side is SKIPPED for that side: it is counted in the skipped slot alone and its
 * auc is written as NaN.  All double sums run over r ascending (one thread per column: no reduction tree), so two calls give
 * equal bits.
 * Work mapping: one workgroup of S waves; wave s takes side s, lane j level j; the wave walks the R rows; a row's skip flag is one
 * ballot, its chain is formed by every lane alike from lane-to-lane reads and stored by lane 0.
 * ISG_EINVAL: a negative R or L; sides outside 1..3.  ISG_EUNSUPPORTED: L > 64; R L S of 2^31 - 1024 or more.  R == 0 or L == 0:
 * ISG_OK, nothing is written.  ISG_EINVAL: a missing p_inst, w, auc or totals. */
int isg_curve_sums(const float *p_inst, const float *w, int64_t R, int64_t L, int32_t sides, float *auc, double *totals,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_CURVES_H */
