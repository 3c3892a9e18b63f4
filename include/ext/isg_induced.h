/* Induced-subgraph instances: a batch of G distinct graphs and Q rows of keep bits become, in one pass, the batch of Q graph
 * INSTANCES in which instance q is graph index[q] minus the nodes its bits leave out (csrc/isg_induced.hip); DESIGN.md 34.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_induced.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing
 * throws).  It has an ABI version of its own.
 *
 * THE FUNCTION.  With the names of isg_instances.h -- ptr[g] the node range of graph g, [eb(g), ee(g)) the range of its edges in
 * edge_index, index[q] in [0, G) the graph of instance q -- and with
 *     keep uint32 [Q, W], row stride W: bit (i & 31) of word (i >> 5) of row q says whether LOCAL node i of graph index[q] is in
 *     instance q.  Bits at or beyond n_g = ptr[g + 1] - ptr[g] are ignored; nodes with a local index >= 32 W are dropped;
 *     keep == NULL keeps every node (W is then not looked at),
 * instance q lists the kept nodes of its graph in order and, in their original order, the edges whose two ends are both kept:
 *     batch'[inst_ptr[q] + r]            = q
 *     node_src[inst_ptr[q] + r]          = ptr[g] + i          i = the r-th kept local node of g = index[q]
 *     edge_src[inst_eptr[q] + s]         = the s-th edge of g with both ends kept
 *     edge_index'[:, inst_eptr[q] + s]   = inst_ptr[q] + rank_q(end - ptr[g])   for both ends
 * where rank_q(i) is the number of kept local nodes of instance q below i.  With every bit set (or keep == NULL) this is
 * isg_instances_size / isg_instances_fill; with Q = G, the identity index and the bits of a mask it is isg_subgraph_cut.
 * PRECONDITION, as in isg_instances.h: the edges of one graph are contiguous in edge_index and the graphs follow each other in
 * order; an edge's graph is batch[edge_index[1][e]].
 *
 * One wave per instance in both passes: the wave holds its row of keep one word per lane (hence W <= 64, 2048 nodes per graph),
 * a node's rank is the popcounts of the words below plus that of the bits below, and the graph's edge range is walked 64 edges at
 * a time with a ballot per chunk and a running base.  No kernel uses an atomic: every output word has one writer, or (the two
 * flags) takes a plain store of 1 from whoever sees the fault; two calls give the same bits.  A bad input never faults: every
 * index read from memory is clamped or compared before it becomes an address, and an edge of the range with an end outside its
 * graph's node range is not kept.
 *
 * TWO CALLS, so that the caller can allocate between them: the size pass leaves N' and E' in `status`.
 */
#ifndef ISG_INDUCED_H
#define ISG_INDUCED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_INDUCED_ABI_VERSION 1

int isg_induced_abi_version(void);

/* Bytes of the workspace both passes share: the per-graph edge ranges (int32 [G + 1], what the fill pass reads) and the size
 * pass's per-instance node and edge counts (int32 [2, Q]); 0 for a negative G or Q. */
size_t isg_induced_workspace_bytes(int64_t G, int64_t Q);

/* The size pass, three launches behind a 16-byte clear of `status`: the per-graph edge ranges (one thread per edge), the kept
 * nodes and edges of every instance (one wave per instance), then ONE workgroup's scan over the Q counts in blocks of 1024.
 * ptr int32 [G + 1] (clamped to [0, N] and to non-decreasing where it is not); batch int64 [N]; edge_index int64 [2, E] (row
 * stride E); index int32 [Q]; keep uint32 [Q, W] or NULL.
 * inst_ptr / inst_eptr int32 [Q + 1]: node / edge range of every instance.
 * status int32 [4] = (N', E', bad_index, bad_grouping), with the meanings of isg_instances.h: bad_index 1 when some index[q]
 * lies outside [0, G) (such an instance is empty); bad_grouping 1 when the graph ids decrease along the edge list, an edge's two
 * ends lie in different graphs, or an end or its graph id is out of range (the outputs are then in bounds and wrong).
 * Sums run in 64 bits; a running total beyond 2^31 - 1 is stored as 2^31 - 1.
 * ISG_EINVAL: a negative size, G == 0 with Q > 0, W < 1 with a keep, a missing ptr / index / inst_ptr / inst_eptr / status, a
 * missing batch or edge_index with E > 0 -- all checked before anything is dereferenced.  ISG_EUNSUPPORTED: N, E, G or Q of
 * 2^31 - 1024 or more; W > 64 with a keep.  ISG_EWORKSPACE: a missing or short workspace.  Q == 0: ISG_OK, nothing is written
 * (not even status). */
int isg_induced_size(const int32_t *ptr, const int64_t *batch, const int64_t *edge_index, const int32_t *index,
                     const uint32_t *keep, int64_t W, int64_t N, int64_t E, int64_t G, int64_t Q, int32_t *inst_ptr,
                     int32_t *inst_eptr, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* The fill pass, one launch, one wave per instance: batch_out int64 [cap_nodes], node_src int64 [cap_nodes], edge_src int64
 * [cap_edges], edge_index_out int64 [2, cap_edges] (row stride cap_edges).  keep / W / inst_ptr / inst_eptr / workspace: as the
 * size pass took and left them.  Entries at or beyond a capacity are not written; with cap_nodes = N' and cap_edges = E' every
 * entry is.
 * ISG_EINVAL: a negative size or capacity, G == 0 with Q > 0, W < 1 with a keep, a missing ptr / index / inst_ptr / inst_eptr,
 * a missing batch_out / node_src with cap_nodes > 0, a missing edge_index / edge_index_out / edge_src with cap_edges > 0.
 * ISG_EUNSUPPORTED: a size or capacity of 2^31 - 1024 or more; W > 64 with a keep.  ISG_EWORKSPACE as above.  Q == 0: ISG_OK,
 * nothing is written. */
int isg_induced_fill(const int32_t *ptr, const int64_t *edge_index, const int32_t *index, const uint32_t *keep, int64_t W,
                     int64_t N, int64_t E, int64_t G, int64_t Q, const int32_t *inst_ptr, const int32_t *inst_eptr,
                     const void *workspace, size_t workspace_bytes, int64_t cap_nodes, int64_t cap_edges, int64_t *batch_out,
                     int64_t *edge_index_out, int64_t *node_src, int64_t *edge_src, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_INDUCED_H */
