/* Training through shared scene encodings: the backward of isg_instance_rows (include/isg_instances.h), i.e. per DISTINCT row the
 * sum of the gradient rows of that row's copies in the instance batch (csrc/isg_instances_bwd.hip); DESIGN.md 33.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_instances_train.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative
 * ISG_E* status, nothing throws).  It has an ABI version of its own.
 *
 * THE FUNCTION.  With the names of isg_instances.h -- ptr[g] the node range of graph g, erange[g] its edge range (what
 * isg_instances_size leaves in its workspace), inst_ptr / inst_eptr the node / edge ranges of the Q instances -- and with
 * glist[gptr[g] .. gptr[g + 1]) the instances q of graph g in ASCENDING q (index[q] == g):
 *     d_x[n, :Cx] = sum over j in [gptr[g], gptr[g + 1]) of g_xo[inst_ptr[glist[j]] + (n - ptr[g]), :Cx]          ptr[g] <= n < ptr[g + 1]
 *     d_e[e, :Ce] = sum over j in [gptr[g], gptr[g + 1]) of g_eo[inst_eptr[glist[j]] + (e - erange[g]), :Ce]      erange[g] <= e < erange[g + 1]
 * The copies of a row sit at computable addresses, so there is no list of slots, only the [Q] list of instances per graph.
 *
 * The sum starts from the first copy and adds the others in the order of glist with plain fp32 adds, one rounding each (nothing
 * is contracted): a row's bits are those of a host loop over its copies.  No atomics; every output word has one writer; two calls
 * agree bit for bit.  EVERY row of d_x and d_e is written: a row whose graph has no instance, or that no graph's range holds, is +0.
 * A bad input never faults: a graph's range in glist is clamped to [0, Q]; an instance number outside [0, Q), an instance range
 * that is negative or too short for the row's offset, and a copy's row number outside [0, xo_rows) / [0, eo_rows) are compared
 * and that copy is skipped -- none of them is used as an address.  ptr and erange are read at [0, G] only (PRECONDITION for a
 * right answer: both non-decreasing, as every GraphPlan's and every size pass's are).
 */
#ifndef ISG_INSTANCES_TRAIN_H
#define ISG_INSTANCES_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_INSTANCES_TRAIN_ABI_VERSION 1

int isg_instances_train_abi_version(void);

/* ONE launch for both halves, the work mapping of isg_instance_rows: sixteen lanes per OUTPUT row, 16 bytes per lane and access,
 * rows independent.  g_xo fp32 [xo_rows, Cx] row stride ldgx (the gradient of isg_instance_rows' x_out), d_x fp32 [x_rows, Cx] row
 * stride lddx; g_eo [eo_rows, Ce] row stride ldge, d_e [e_rows, Ce] row stride ldde.  ptr / erange int32 [G + 1]; inst_ptr /
 * inst_eptr int32 [Q + 1]; gptr int32 [G + 1]; glist int32 [Q].  Either half may be empty (x_rows == 0 / e_rows == 0: its
 * pointers are not looked at); Q == 0 or xo_rows == 0 is no error: the half's rows are +0 (glist / g_xo are then not looked at).
 * ISG_EINVAL: a negative count; in a half that has rows: a width < 1, a stride below its width, G == 0, a missing d_x / ptr /
 * inst_ptr / gptr (d_e / erange / inst_eptr / gptr), a missing g_xo with xo_rows > 0 (g_eo, eo_rows), a missing glist with Q > 0.
 * ISG_EUNSUPPORTED: a width or stride that is no multiple of 4 or a row pointer that is not 16-byte aligned in a half that has
 * rows; a count (rows, G, Q) of 2^31 - 1024 or more.  x_rows == 0 and e_rows == 0: ISG_OK, nothing is written. */
int isg_instance_rows_bwd(const float *g_xo, int32_t ldgx, int64_t xo_rows, float *d_x, int32_t lddx, int64_t x_rows, int32_t Cx,
                          const float *g_eo, int32_t ldge, int64_t eo_rows, float *d_e, int32_t ldde, int64_t e_rows, int32_t Ce,
                          const int32_t *ptr, const int32_t *erange, const int32_t *inst_ptr, const int32_t *inst_eptr,
                          const int32_t *gptr, const int32_t *glist, int64_t G, int64_t Q, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_INSTANCES_TRAIN_H */
