/* Many questions per scene graph: a batch of G distinct graphs expanded on the device into the batch of Q graph INSTANCES that
 * Q questions would have brought along as copies (csrc/isg_instances.hip); DESIGN.md 30.
 *
 * Fifteenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: device pointers, `ld*` = row stride
 * in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its
 * own: none of the other headers moves when an entry point here does.
 *
 * THE FUNCTION.  index[q] in [0, G) names the graph of question q.  Instance q lists graph index[q]'s nodes in order and its edges
 * in their original order, renumbered; the instance batch is exactly what concatenating copies of the graphs would give:
 *     batch'[inst_ptr[q] + i]            = q                                   i < ptr[g + 1] - ptr[g],  g = index[q]
 *     node_src[inst_ptr[q] + i]          = ptr[g] + i
 *     edge_src[inst_eptr[q] + j]         = eb(g) + j                           j < ee(g) - eb(g)
 *     edge_index'[:, inst_eptr[q] + j]   = edge_index[:, eb(g) + j] - ptr[g] + inst_ptr[q]
 * where [eb(g), ee(g)) is the range of graph g's edges in edge_index.  PRECONDITION: the edges of one graph are contiguous in
 * edge_index and the graphs follow each other in order, as every collate produces; an edge's graph is batch[edge_index[1][e]].
 *
 * No kernel here uses an atomic: every output word has one writer, or (the two flags) takes a plain store of 1 from whoever sees
 * the fault.  A bad input never faults: every index read from memory is clamped or checked before it is used as an address.
 *
 * TWO CALLS, so that the caller can allocate between them (as isg_subgraph_cut's caller sizes its workspace first): the size pass
 * leaves N' and E' in `status`; a caller who knows the graphs' sizes on the host computes them there and never reads `status`.
 */
#ifndef ISG_INSTANCES_H
#define ISG_INSTANCES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_INSTANCES_ABI_VERSION 1

int isg_instances_abi_version(void);

/* Bytes of the workspace both passes share (the per-graph edge ranges, int32 [G + 1]); 0 for a negative G. */
size_t isg_instances_workspace_bytes(int64_t G);

/* The size pass, two launches behind a 16-byte clear of `status`: the per-graph edge ranges (one thread per edge), then ONE
 * workgroup's scan over the Q instances in blocks of 1024.
 * ptr int32 [G + 1]: node range of every graph (a GraphPlan's; clamped to [0, N] and to non-decreasing where it is not);
 * batch int64 [N]; edge_index int64 [2, E] (row stride E); index int32 [Q].
 * inst_ptr / inst_eptr int32 [Q + 1]: node / edge range of every instance.
 * status int32 [4] = (N', E', bad_index, bad_grouping):
 *   bad_index     1 when some index[q] lies outside [0, G); such an instance is empty.
 *   bad_grouping  1 when the graph ids decrease along the edge list, an edge's two ends lie in different graphs, or an end or its
 *                 graph id is out of range.  The ranges are then some ranges inside [0, E] -- the outputs are in bounds and
 *                 wrong, and where the ids decrease (a range then has several writers) two calls may disagree on them.
 * Sums run in 64 bits; a running total beyond 2^31 - 1 is stored as 2^31 - 1 (the fill pass writes nothing beyond its capacities).
 * ISG_EINVAL: a negative size, G == 0 with Q > 0, a missing ptr / index / inst_ptr / inst_eptr / status, a missing batch or
 * edge_index with E > 0 -- all checked before anything is dereferenced.  ISG_EUNSUPPORTED: N, E, G or Q of 2^31 - 1024 or more.
 * ISG_EWORKSPACE: a missing or short workspace.  Q == 0: ISG_OK, nothing is written (not even status). */
int isg_instances_size(const int32_t *ptr, const int64_t *batch, const int64_t *edge_index, const int32_t *index, int64_t N,
                       int64_t E, int64_t G, int64_t Q, int32_t *inst_ptr, int32_t *inst_eptr, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream);

/* The fill pass, one launch, one wave per instance: batch_out int64 [cap_nodes], node_src int64 [cap_nodes], edge_src int64
 * [cap_edges], edge_index_out int64 [2, cap_edges] (row stride cap_edges).  inst_ptr / inst_eptr / workspace: as the size pass left
 * them.  Entries at or beyond a capacity are not written; with cap_nodes = N' and cap_edges = E' every entry is.
 * ISG_EINVAL: a negative size or capacity, G == 0 with Q > 0, a missing ptr / index / inst_ptr / inst_eptr, a missing batch_out /
 * node_src with cap_nodes > 0, a missing edge_index / edge_index_out / edge_src with cap_edges > 0.  ISG_EUNSUPPORTED: a size or
 * capacity of 2^31 - 1024 or more.  ISG_EWORKSPACE as above.  Q == 0: ISG_OK, nothing is written. */
int isg_instances_fill(const int32_t *ptr, const int64_t *edge_index, const int32_t *index, int64_t N, int64_t E, int64_t G,
                       int64_t Q, const int32_t *inst_ptr, const int32_t *inst_eptr, const void *workspace, size_t workspace_bytes,
                       int64_t cap_nodes, int64_t cap_edges, int64_t *batch_out, int64_t *edge_index_out, int64_t *node_src,
                       int64_t *edge_src, void *stream);

/* x_out[i, :Cx] = x[node_src[i], :Cx] for i < n_out and e_out[j, :Ce] = e[edge_src[j], :Ce] for j < m_out, fp32 rows, ONE launch:
 * sixteen lanes per row, 16 bytes per lane and access.  x [x_rows, Cx] row stride ldx, e [e_rows, Ce] row stride lde; a source
 * row number outside [0, x_rows) / [0, e_rows) leaves its output row unwritten.  Either half may be empty (n_out == 0 / m_out == 0:
 * its pointers are not looked at).
 * ISG_EINVAL: a negative count, a width < 1 or a stride below its width in a half that has rows, a missing pointer there.
 * ISG_EUNSUPPORTED: a width or stride that is no multiple of 4 or a pointer that is not 16-byte aligned in a half that has rows;
 * a count of 2^31 - 1024 or more.  n_out == 0 and m_out == 0: ISG_OK, nothing is written. */
int isg_instance_rows(const float *x, int32_t ldx, int64_t x_rows, const int64_t *node_src, int64_t n_out, float *x_out,
                      int32_t ldxo, int32_t Cx, const float *e, int32_t lde, int64_t e_rows, const int64_t *edge_src, int64_t m_out,
                      float *e_out, int32_t ldeo, int32_t Ce, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_INSTANCES_H */
