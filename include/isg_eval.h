/* Evaluation by question type on the device: the rank of the true answer with the K best classes of every row, running meters per
 * group of questions, and the token co-occurrence totals per group (csrc/isg_eval.hip); DESIGN.md 31.
 *
 * Sixteenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `ld*` = row
 * stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version
 * of its own: none of the other headers moves when an entry point here does.
 *
 * The rules of include/isg_optim.h hold: nothing here returns a device value to the host, no kernel uses an atomic in global
 * memory, and every floating-point sum runs in one fixed order (the rows of a workgroup ascending, then the workgroups ascending
 * inside ONE finishing workgroup, all in double), so two identical calls give the same bits.  Every argument is checked, and
 * ISG_EINVAL reported, before any HIP call.
 *
 * GROUPS.  `groups` is int32 [B, F], 1 <= F <= ISG_EVAL_FACETS_MAX: row b belongs to group groups[b, f] for every facet f.  The ids
 * of all facets are numbered in ONE space [0, G), 1 <= G <= ISG_EVAL_GROUPS_MAX (datasets.gqa.QuestionTypes numbers them so that
 * two facets never share an id); -1 means "no group in this facet".  A row that names one group in two facets is added to it
 * twice.  An id below -1 or at or above G is a BAD id: the row is skipped for that facet, and `status` (int32 [2], optional, zeroed
 * by the caller once per evaluation) is advanced: status[0] += the bad ids this call saw; status[1] = the lowest row of this call
 * that held one, written only while status[0] was still 0.  A bad input never faults.
 */
#ifndef ISG_EVAL_H
#define ISG_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_EVAL_ABI_VERSION 1

int isg_eval_abi_version(void);

#define ISG_EVAL_TOPK_MAX 8        /* classes per row isg_answer_rank lists */
#define ISG_EVAL_FACETS_MAX 4      /* F */
#define ISG_EVAL_GROUPS_MAX 256    /* G */

/* Slots of a group's row of isg_group_meters' `totals` (double [G, 8]). */
#define ISG_GRP_ROWS 0             /* rows counted (rank >= 0) */
#define ISG_GRP_LOSS_SUM 1         /* sum of row_loss over the counted rows whose loss is finite */
#define ISG_GRP_NONFINITE 2        /* counted rows whose loss is NaN or infinite */
#define ISG_GRP_HITS1 3            /* counted rows with rank == 0 */
#define ISG_GRP_HITSK 4            /* counted rows with rank < k */
#define ISG_GRP_SLOTS 8            /* 5 to 7: reserved, never written */

/* The rank of the true answer, and the K best classes, over fp32 logits [B, A] (row stride ld >= A, rows only 4-byte aligned, as
 * isg_xent_fwd takes them) and int64 labels [B].  One launch, a wave per row, lanes striding the row.
 *   rank[b] (int32) = #{a : x[a] > x[l] or (x[a] == x[l] and a < l)}, l = labels[b]: the classes that beat the label, a tie going
 *     to the lower index -- so rank == 0 exactly where isg_xent_fwd's pred (the lowest index among the maxima) equals the label;
 *     -1 for a row whose label == ignore_index;  A for any other label outside [0, A) and for a row that holds a NaN: such a row
 *     is never a hit at any k.
 *   top_ids int64 [B, K], top_prob fp32 [B, K] (each optional; 1 <= K <= ISG_EVAL_TOPK_MAX whenever one is given, K is not looked
 *     at otherwise): the K best classes of the row, value descending and index ascending among equals, found in K rounds of a
 *     wave-wide maximum and a wave-wide lowest index;  top_prob = expf((float)((double)x - row_lse[b])), with row_lse (double [B],
 *     what isg_xent_fwd wrote) required whenever top_prob is given.  Entries at and beyond A (K > A) get id -1 and probability 0,
 *     and so does every entry of a row that holds a NaN.  Ignored rows and rows with a bad label have their best classes listed
 *     like any other.
 * ISG_EINVAL: B < 0, A < 1, ld < A, K outside [1, ISG_EVAL_TOPK_MAX] with top_ids or top_prob given, top_prob without row_lse, a
 * null logits / labels / rank with B > 0.  ISG_EUNSUPPORTED: B >= 2^31.  B == 0: ISG_OK, nothing is launched. */
int isg_answer_rank(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, const double *row_lse,
                    int32_t *rank, int64_t *top_ids, float *top_prob, int32_t K, int64_t B, int32_t A, void *stream);

/* Doubles of isg_group_meters' workspace `parts` for B rows and G groups: one partial table per workgroup of the first launch.
 * Host only; 0 for B < 0 or G outside [1, ISG_EVAL_GROUPS_MAX]. */
int64_t isg_group_meters_parts(int64_t B, int32_t G);

/* Running meters per group: row_loss fp32 [B] and rank int32 [B] (isg_xent_fwd's and isg_answer_rank's) are added into
 * totals double [G, ISG_GRP_SLOTS] in place, slots ISG_GRP_* above; k >= 1 is a host scalar of THIS call.  A row with rank < 0 (an
 * ignored one) is counted nowhere.  Two launches.  The first: a workgroup takes 64 consecutive rows, thread g walks them in
 * ascending order for group g and writes that group's five sums (doubles; the counts are exact) into the workgroup's partial
 * table in `parts`.  The second, one finishing workgroup: every slot is summed over the workgroups ascending, in double, and
 * added to totals; `status` is advanced as the head of this file says.  overall (double [ISG_GRP_SLOTS], optional): the same five
 * slots over ALL rows of the call, each counted row once whatever its groups, summed in the same order.
 * ISG_EINVAL: B < 0, F or G out of range, k < 1, a null row_loss / rank / groups / totals / parts with B > 0.  ISG_EWORKSPACE:
 * parts_len < isg_group_meters_parts(B, G).  ISG_EUNSUPPORTED: B >= 2^31.  B == 0: ISG_OK, nothing is launched. */
int isg_group_meters(const float *row_loss, const int32_t *rank, const int32_t *groups, int32_t F, int32_t G, int32_t k,
                     double *totals, double *overall, double *parts, int64_t parts_len, int32_t *status, int64_t B, void *stream);

/* Token co-occurrence totals per group: isg_token_coo's `table` int32 [B, 8] and qflags int32 [B] (optional: NULL = all 0) are
 * added into totals int64 [G, ISG_COO_TOTALS] (include/isg.h) in place.  Row g of totals advances by exactly what isg_token_coo's
 * finishing kernel adds for the questions of group g alone: every slot and every histogram, the reserved slots 12 to 15 never
 * written.  All integer and exact.  ONE launch of G workgroups: workgroup g walks all B rows for its own group, sums in registers
 * and LDS, and is the only writer of totals' row g; workgroup 0 also advances `status`.
 * ISG_EINVAL: B < 0, F or G out of range, a null table / groups / totals with B > 0.  ISG_EUNSUPPORTED: B >= 2^31 - 1 (as
 * isg_token_coo).  B == 0: ISG_OK, nothing is launched. */
int isg_token_coo_groups(const int32_t *table, const int32_t *qflags, const int32_t *groups, int32_t F, int32_t G, int64_t *totals,
                         int32_t *status, int64_t B, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_EVAL_H */
