/* Shapley sampling (permutation sampling of node Shapley values): the two steps around the forwards of a permutation explainer,
 * each as ONE launch (csrc/isg_shapley.hip); DESIGN.md 39.  isg_shapley_keep_bits draws seeded random permutations of every listed
 * graph's nodes and writes the keep rows of all their proper prefixes for isg_induced_size / isg_induced_fill
 * (include/ext/isg_induced.h); isg_shapley_values reduces the predicted class's probability on those instances to a Shapley
 * estimate per node, its sum of squares and the completeness gap of every graph.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_shapley.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers unless a parameter says HOST, `stream` = hipStream_t or NULL, ISG_OK or a negative
 * ISG_E* status, nothing throws).  It has an ABI version of its own.
 *
 * No atomics.  Every output word has one writer.  Two calls give the same bits.  Every number read from memory that becomes an
 * address is compared first; what fails the comparison is never used as an address.
 *
 * THE ESTIMATOR.  For graph g with n nodes, predicted class pred[g] and full-graph probability p[g] (from the batch's own forward):
 *   value function   v(S) = the predicted class's softmax probability on the induced subgraph S (isg_induced_*);
 *   full set         v(full) = p[g]; the full set is not forwarded again;
 *   empty set        v(empty) = v_empty, a host float given by the caller (0 by default on the host side): the model never sees an
 *                    empty graph; with v_empty = 0 the attributions of a graph sum to p[g];
 *   marginal         with M permutations pi_m and pos_m[i] the position of local node i in pi_m:
 *                        d_m[i] = v(P_m,pos+1) - v(P_m,pos),   P_m,k = the first k nodes of pi_m,  P_m,0 = empty,  P_m,n = full;
 *   samples          T = M samples e_t = d_t without antithetic; with antithetic M is even, pi_2t+1 is pi_2t reversed
 *                    (pos_2t+1[i] = n - 1 - pos_2t[i]) and there are T = M / 2 samples e_t = 0.5 (d_2t + d_2t+1);
 *   arithmetic       every operation is one fp32 operation rounded to nearest, never contracted:
 *                        d = sub_rn(v_hi, v_lo);   e = mul_rn(0.5f, add_rn(d0, d1));   acc = add_rn(acc, e) over t ascending from +0;
 *                        phi = acc / (float)T, one correctly rounded division;
 *                        m2 = fmaf(e, e, m2) over t ascending from +0 (optional; it exists for a standard error).
 *
 * KNOWN ANSWER (tests/shapley_restated.py, smoke()).  One graph of 3 nodes, g = 0, seed = 0x100000007, M = 2, antithetic, W = 1,
 * row_ptr = [0, 4]:
 *     key     = [0xB8A65C43, 0x29FF42B2, 0x3C12D07E]        (draw 0; node 1 has the smallest key, node 0 the largest)
 *     pos     = [[2, 0, 1], [0, 2, 1]]                      (row 1 is row 0 reversed: 2 - pos)
 *     keep    = [0b010, 0b110, 0b001, 0b101]                (rows q = 0..3: m = 0 k = 1, m = 0 k = 2, m = 1 k = 1, m = 1 k = 2)
 *     index   = [0, 0, 0, 0],   status = [0, 0, 0, 4]
 * and with p_inst = [0.25, 0.5, 0.125, 0.75], p = [1], v_empty = 0:
 *     phi     = [0.3125, 0.25, 0.4375]                      (node 0: 0.5 ((1 - 0.5) + (0.125 - 0)); their sum is p)
 *     m2      = [0.09765625, 0.0625, 0.19140625],   gap = [0],   flag = [0]
 */
#ifndef ISG_SHAPLEY_H
#define ISG_SHAPLEY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_SHAPLEY_ABI_VERSION 1

int isg_shapley_abi_version(void);

/* SEEDED PERMUTATIONS AND THE KEEP ROWS OF ALL THEIR PREFIXES.  ptr int32 [G + 1]: the range starts of the G graphs' nodes.
 * graphs int32 [R]: the listed graphs.  row_ptr int32 [R + 1]: the first row of every listed graph, formed by the caller.
 * M: permutations per graph.  Q: rows of index and keep.  antithetic: 0 or 1.  seed: the 64-bit Philox key.  W: words of 32 keep
 * bits per row.
 * Outputs: pos int32 [M, N], written for the nodes of listed graphs only; index int32 [Q]; keep uint32 [Q, W]; status int32 [4].
 *
 * THE RANGE of listed graph g = graphs[r] is isg_curve_keep_bits's:  lo = min(max(ptr[g], 0), N),
 * hi = max(min(max(ptr[g + 1], 0), N), lo);  n = min(hi - lo, 32 W); the nodes with local index >= 32 W take no part and
 * status[0] is 1.
 * KEYS.  The draw number is t = m without antithetic and t = m >> 1 with it.  key_i = Philox::draw(seed, (uint32)g,
 * 0x80000000 | (t << 11) | i) for local node i (csrc/isg_common.hpp, oracle/philox.py): the top bit keeps the stream apart from
 * the samplers' (g, slot) draws under the same seed; the key depends on the graph's number g, not on r, so a graph's
 * permutations do not depend on what is listed beside it or in which order.
 * POSITION.  pos_m[i] = #{j < n : key_j < key_i, or key_j = key_i and j < i}: a permutation of 0 .. n - 1, ties to the lower
 * node; an odd m under antithetic is n - 1 - pos_m-1[i].  pos[m N + lo + i] = pos_m[i].
 * ROWS of graph r, for m in [0, M) and k in [1, n - 1]:  q = row_ptr[r] + m (n - 1) + (k - 1);  index[q] = g;  bit i & 31 of
 * word i >> 5 of row q is (pos_m[i] < k); bits at or beyond n are 0; all W words of the row are written.  A graph with n <= 1
 * has no rows: its only subsets are the empty and the full set.
 * ROW_PTR is compared before use.  With need = M max(n - 1, 0) (n = 0 for an entry of graphs outside [0, G)), in 64 bits: a
 * graph whose row_ptr[r] < 0 or row_ptr[r] + need > Q writes no rows and no pos, and status[2] is 1; row_ptr[r + 1] !=
 * row_ptr[r] + need sets status[2] as well.  Under an inconsistent row_ptr the rows of graphs whose row ranges overlap are
 * written in no stated order, and so are the pos words of graphs whose node ranges overlap under a ptr that was not
 * non-decreasing or of a graph listed twice (the same values); nothing else is affected.
 * A graphs[r] outside [0, G) writes nothing, sets status[1] and is never used as an address.
 * status = [a listed graph has more than 32 W nodes, an entry of graphs is outside [0, G), a bad row_ptr, Q], all four words
 * written by one wave.
 *
 * Work mapping: one 64-lane wave per (listed graph, draw).  The n keys are staged in LDS (128 W bytes); lane l owns nodes l,
 * l + 64, ... and counts over the whole graph from LDS, every lane reading the same words (a broadcast); the positions go back
 * to LDS (another 128 W bytes); a row's words come from one 64-bit ballot per 64 nodes, stored by two lanes; the wave writes
 * its draw's rows and, under antithetic, the twin's.  Wave (0, 0) also reads all of graphs and row_ptr and writes status.
 *
 * Checked in this order.  ISG_EINVAL: a negative N, G, R, M or Q; M < 1; antithetic outside {0, 1}; an odd M with antithetic;
 * W < 1.  ISG_EUNSUPPORTED: W > 64; M > 1024; N, G, R, M N or Q of 2^31 - 1024 or more.  Then R == 0: ISG_OK, nothing is
 * written.  ISG_EINVAL: a missing ptr, graphs, row_ptr or status; with N > 0 a missing pos; with Q > 0 a missing index or keep. */
int isg_shapley_keep_bits(const int32_t *ptr, const int32_t *graphs, const int32_t *row_ptr, int64_t N, int64_t G, int64_t R,
                          int64_t M, int64_t Q, int32_t antithetic, uint64_t seed, int32_t W, int32_t *pos, int32_t *index,
                          uint32_t *keep, int32_t *status, void *stream);

/* INSTANCE PROBABILITIES TO SHAPLEY ESTIMATES.  p_inst fp32 [Q]: the predicted class's probability on every instance, in the row
 * order above.  p fp32 [G]: that class's probability on the whole graph.  pos int32 [M, N], ptr, graphs, row_ptr, N, G, R, M, Q,
 * antithetic and W as above.  v_empty: HOST fp32, finite.
 * Outputs: phi fp32 [N]; m2 fp32 [N] or NULL; gap fp32 [R]; flag int32 [R].
 * Per listed graph THE ESTIMATOR above, for local node i < n: v_hi = p[g] where pos + 1 = n, else p_inst[row_ptr[r] + m (n - 1) +
 * pos]; v_lo = v_empty where pos = 0, else p_inst[row_ptr[r] + m (n - 1) + pos - 1].  Every pos read from memory is clamped to
 * [0, n - 1] before it forms a row number (both rows of an antithetic pair are read; none is derived from the other), and
 * row_ptr[r] is held to the bound above.  phi[lo + i] and m2[lo + i] are written for the listed graphs' nodes below 32 W only.
 * flag[r]:  0 fine;  1 a non-finite p[g] or a non-finite p_inst among the graph's M (n - 1) rows: every phi and m2 of the graph
 * is NaN and gap[r] is NaN;  2 a graphs[r] outside [0, G), or row_ptr[r] < 0 or row_ptr[r] + M max(n - 1, 0) > Q: nothing of phi
 * or m2 is written for it and gap[r] is NaN.  n == 0 (decided before p is read): gap = +0, flag = 0.
 * GAP.  gap[r] = sub_rn(sum_i phi_i, sub_rn(p[g], v_empty)), the completeness gap; the sum in this order: lane l adds its nodes
 * l, l + 64, ... ascending from +0, then a xor butterfly over the 64 lanes at offsets 32, 16, 8, 4, 2, 1 (add_rn each).
 *
 * Work mapping: one 64-lane wave per listed graph.  A ballot over the graph's M (n - 1) values and p[g] sets the skip flag
 * first; lane l then walks its nodes and, per node, the draws in order: two gathers per draw from the graph's contiguous slice
 * of p_inst, or p[g] / v_empty at the ends.
 *
 * Checked in this order.  ISG_EINVAL: a negative N, G, R, M or Q; M < 1; antithetic outside {0, 1}; an odd M with antithetic;
 * W < 1; a non-finite v_empty.  ISG_EUNSUPPORTED: W > 64; M > 1024; N, G, R, M N or Q of 2^31 - 1024 or more.  Then R == 0:
 * ISG_OK, nothing is written.  ISG_EINVAL: a missing ptr, graphs, row_ptr, gap or flag; with G > 0 a missing p; with N > 0 a
 * missing pos or phi; with Q > 0 a missing p_inst. */
int isg_shapley_values(const float *p_inst, const float *p, const int32_t *pos, const int32_t *ptr, const int32_t *graphs,
                       const int32_t *row_ptr, int64_t N, int64_t G, int64_t R, int64_t M, int64_t Q, int32_t antithetic,
                       float v_empty, int32_t W, float *phi, float *m2, float *gap, int32_t *flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_SHAPLEY_H */
