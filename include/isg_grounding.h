/* Grounding of the sampled subgraph in GQA's object annotations, on the device: how many of the scene-graph objects a question,
 * its answer and its full answer refer to are among the nodes the node mask kept (csrc/isg_grounding.hip); DESIGN.md 32.
 *
 * Seventeenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `stream` =
 * hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its own: none of the other
 * headers moves when the entry point here does.
 *
 * The rules of include/isg_eval.h hold: every argument is checked, and ISG_EINVAL reported, before any HIP call; nothing is
 * returned to the host; no kernel uses an atomic in global memory; everything is integer and exact, so two identical calls give
 * the same bits.  A bad input sets a count and never faults: every gold index is checked against its graph's node count before it
 * is used as an address, and `ptr` is clamped to [0, N] as isg_token_coo clamps it.
 *
 * GOLD.  `gold` is int32 [B, F, M], 1 <= F <= ISG_GROUND_FACETS, 1 <= M <= ISG_GROUND_GOLD_MAX (datasets.gqa.ObjectAnnotations.encode):
 * facet s of question g lists the LOCAL node indices (0 = the first node of the question's graph) of the objects that facet's
 * words refer to.  ISG_GROUND_PAD (-1) pads a list; ISG_GROUND_UNRESOLVED (-2) stands for an object that is annotated but is not a
 * node of the graph.  Any other entry below 0, and any entry at or above the graph's node count n_g, is a BAD entry: it is counted
 * (column 3) and used for nothing else.  Within a facet, and within the union of the facets, an index counts ONCE: an entry
 * counts only if no earlier entry of the same set (facets ascending, then positions ascending) holds the same index.
 *
 * GROUPS.  `groups` int32 [B, Fg], G, the bad-id rule and `status` int32 [2] are exactly what the head of include/isg_eval.h
 * defines (ids of all facets in one space [0, G), -1 = no group, a row that names one group in two facets is added to it twice).
 * groups == NULL means no groups: Fg and G are not looked at and only row 0 of `totals` is written.
 */
#ifndef ISG_GROUNDING_H
#define ISG_GROUNDING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_GROUNDING_ABI_VERSION 1

int isg_grounding_abi_version(void);

#define ISG_GROUND_FACETS 3          /* F: question, answer, fullAnswer */
#define ISG_GROUND_GOLD_MAX 64       /* M: entries of one facet of one question */
#define ISG_GROUND_PAD (-1)
#define ISG_GROUND_UNRESOLVED (-2)

/* Columns of a question's row of `table` (int32 [B, ISG_GROUND_COLS]). */
#define ISG_GROUND_COL_KEPT 0        /* |P|: kept nodes of the graph */
#define ISG_GROUND_COL_NODES 1       /* n_g */
#define ISG_GROUND_COL_UNRESOLVED 2  /* entries equal to ISG_GROUND_UNRESOLVED, over all facets */
#define ISG_GROUND_COL_BAD 3         /* bad entries, over all facets */
#define ISG_GROUND_COL_SETS 4        /* 4 + 2 s: |G_s|, the distinct valid indices of set s;  5 + 2 s: |P n G_s|.  Sets 0 .. 2 are the
                                      * facets (both 0 for s >= F), set 3 the union of all facets (distinct across facets). */
#define ISG_GROUND_SETS 4
#define ISG_GROUND_COLS 12

/* A row of `totals` (int64 [1 + G, ISG_GROUND_TOTALS]; row 0 every question, row 1 + g the questions of group g):
 *   head, ISG_GROUND_HEAD entries: [0] questions, [1] correct ones (pred == label; 0 without pred), [2] the sum of column 2,
 *     [3] the sum of column 3, [4 .. 8) reserved, never written;
 *   then 2 * ISG_GROUND_SETS blocks of ISG_GROUND_BLOCK entries, block 2 s + c at ISG_GROUND_HEAD + (2 s + c) * ISG_GROUND_BLOCK:
 *     set s over ALL questions (c = 0), then set s over the CORRECT questions (c = 1).  A block covers the questions with
 *     |G_s| > 0 and holds [0] those questions, [1] the sum of |P|, [2] of n_g, [3] of |G_s|, [4] of the hits |P n G_s|,
 *     [5] questions with hits > 0, [6] questions with hits == |G_s|, [7] reserved, never written;  then two histograms of
 *     ISG_GROUND_HIST entries indexed by m = |G_s|: at [8 + m] the questions, at [8 + ISG_GROUND_HIST + m] their hits.
 * The macro recall, the sum over the questions of hits / |G_s|, is the sum over m of hits[m] / m, formed on the host: no
 * floating-point sum runs on the device (the device isg_token_coo uses for its ratios).
 * A histogram has ISG_GROUND_FACETS * ISG_GROUND_GOLD_MAX + 1 entries, not ISG_GROUND_GOLD_MAX + 1: the union of three facets of
 * 64 distinct indices each holds up to 192, and a bin that took every larger m would make the macro recall of the union inexact.
 * Every block has the same shape, so the facets' histograms are never written beyond m = ISG_GROUND_GOLD_MAX. */
#define ISG_GROUND_HEAD 8
#define ISG_GROUND_HIST (ISG_GROUND_FACETS * ISG_GROUND_GOLD_MAX + 1)
#define ISG_GROUND_BLOCK (8 + 2 * ISG_GROUND_HIST)
#define ISG_GROUND_TOTALS (ISG_GROUND_HEAD + 2 * ISG_GROUND_SETS * ISG_GROUND_BLOCK)

/* kept(n) = node_mask[n] > threshold (fp32 [N]; a NaN is not kept, as in isg_token_coo); question g owns the nodes
 * [ptr[g], ptr[g + 1]) (int32 [B + 1]), n_g of them.  pred, label (int64 [B]) are given both or neither.
 * Launch 1: one wave per question, four questions per workgroup of 256 threads; lane j holds entry j of every facet, the
 * pairwise comparison runs on values read from the other lanes, |P| is a wave reduction over lanes striding the graph's nodes.
 * It writes every column of every row of `table`.
 * Launch 2 (skipped when totals == NULL): 1 + G workgroups (1 without groups); workgroup r walks all B rows and is the only writer
 * of row r of `totals`; workgroup 0 also advances `status` (optional).  The call ADDS to totals, which the caller zeroes once per
 * evaluation.
 * ISG_EINVAL: N < 0, B < 0, F outside [1, ISG_GROUND_FACETS], M outside [1, ISG_GROUND_GOLD_MAX], pred without label or the
 * reverse, groups with G outside [1, ISG_EVAL_GROUPS_MAX] or Fg outside [1, ISG_EVAL_FACETS_MAX], a null ptr / gold / table with
 * B > 0, a null node_mask with B > 0 and N > 0.  ISG_EUNSUPPORTED: N or B >= 2^31 - 1.  B == 0: ISG_OK, nothing is launched. */
int isg_grounding(const float *node_mask, float threshold, const int32_t *ptr, const int32_t *gold, int32_t F, int32_t M,
                  const int64_t *pred, const int64_t *label, const int32_t *groups, int32_t Fg, int32_t G, int32_t *table,
                  int64_t *totals, int32_t *status, int64_t N, int64_t B, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_GROUNDING_H */
