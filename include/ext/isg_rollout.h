/* Attention rollout: the read-out's pooling weights walked back through the layers' head-averaged attention weights, with a
 * residual share at every layer (Abnar & Zuidema 2020) -- a node attribution from ONE forward (csrc/isg_rollout.hip); DESIGN.md 35.
 *
 * An extension header of libisg_hip.so: it lies under include/ext/, outside the table of device headers that _lib.load() binds
 * (isubgvqa_amd/_lib.py, HEADERS), and is bound by isubgvqa_amd/_ext_rollout.py on the same handle.  The status codes and
 * conventions of isg.h hold (device pointers, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing
 * throws).  It has an ABI version of its own.
 *
 * THE FUNCTION.  Inputs:
 *     ptr int32 [B + 1]: the node range of graph g is [ptr[g], ptr[g + 1]);
 *     the CSR by source: rowptr_s int32 [N + 1], eid_s int32 [E], dst_s int32 [E] -- the out-slots of node s are
 *         rowptr_s[s] .. rowptr_s[s + 1] - 1, slot j names the edge eid_s[j] and its destination dst_s[j];
 *     for the layers l = 0 .. L - 1: alpha_l fp32 [E, H] by EDGE ID with row stride lda_l >= H, and optionally mask_l fp32 [N]
 *         (the layer's node mask; none = all ones);
 *     start fp32 [N];  residual = lambda in [0, 1].
 * With  a_l[e] = (sum over h of alpha_l[e, h]) / H  and  w_l[e] = a_l[e] * mask_l[src e] * mask_l[dst e]:
 *     r_L = start
 *     for l = L - 1 down to 0, for every node s of graph g:
 *         flow[l][e] = (1 - lambda) * w_l[e] * r_{l+1}[dst e]         for every out-slot e of s, in slot order
 *         r_l[s]     = lambda * r_{l+1}[s] + sum over e of flow[l][e]  (slots ascending, fp32)
 *     relevance = r_0
 * In fp32, every operation rounded once (nothing is contracted into an fma): the head sum runs h ascending from alpha_l[e, 0] and
 * is multiplied once by the fp32 value of 1 / H; w = (a * mask[src]) * mask[dst]; flow = ((1 - lambda) * w) * r[dst]; the node's
 * sum starts from lambda * r[s] and adds the flows slot by slot.  The result is a function of the inputs alone.
 *
 * RULES.
 *   - A slot whose eid lies outside [0, E) contributes nothing and is never used as an address.
 *   - A slot whose dst lies outside its source's graph range [ptr[g], ptr[g + 1]) contributes nothing and is never used as an
 *     address.
 *   - ptr is clamped to [0, N] and made non-decreasing (hi = max(lo, .)), as isg_induced_size does; rowptr_s is clamped to [0, E]
 *     in the same way.
 *   - The kernel is launched for graphs of up to `nmax` nodes (the plan's bound).  A graph with more nodes gets NaN in every one
 *     of its relevance rows and is otherwise skipped (its rows of edge_flow stay as the caller left them).
 *   - No atomics.  Every output word has one writer.  Two calls give the same bits.
 *
 * KNOWN ANSWER.  2 nodes; edges by id 0->0, 1->1, 0->1; H = 1, L = 1; alpha = [1, 0.25, 0.75], start = [0, 1], lambda = 0.5,
 * no mask: relevance = [0.375, 0.625] and flow[0] = [0, 0.125, 0.375].  With a true softmax per destination, no mask and every
 * node reachable from itself, each graph's sum of relevance equals its sum of start.
 *
 * One wave per graph (64-thread workgroups): the graph's two relevance vectors live in LDS, ping-pong; lane i owns the source
 * nodes i, i + 64, ...; all L layers run inside the one launch.
 */
#ifndef ISG_ROLLOUT_H
#define ISG_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_ROLLOUT_ABI_VERSION 1

int isg_rollout_abi_version(void);

/* Host only.  The most layers one call takes (8), and the most nodes per graph a launch can be made for (`nmax`; 4096: the two
 * relevance vectors of a graph, 2 * nmax floats of dynamic LDS, then take 32 KiB, half of what a workgroup gets without asking). */
int isg_rollout_max_layers(void);
int isg_rollout_max_nodes(void);

/* One launch behind no other work.  layers: a HOST int64 table [L][3] = (address of alpha_l, its row stride in floats, address
 * of mask_l or 0); it is read before the call returns.  relevance fp32 [N].  edge_flow fp32 [L, E] with row stride E, or NULL:
 * flow[l][e] is written at edge_flow[l * E + eid] for every valid slot of a graph within nmax; the caller hands in zeros.
 * ISG_EINVAL: a negative size; L < 1 or H < 1; lambda outside [0, 1] or NaN; a row stride below H; with N > 0 a missing ptr,
 * rowptr_s, start, relevance or layers, a missing alpha_l, and with E > 0 a missing eid_s or dst_s -- all checked before anything
 * is dereferenced on the device.  ISG_EUNSUPPORTED: L > isg_rollout_max_layers(), nmax > isg_rollout_max_nodes(); N, E, B, H, nmax
 * or a row stride of 2^31 - 1024 or more.  B == 0 or N == 0: ISG_OK, nothing is written. */
int isg_attention_rollout(const int32_t *ptr, const int32_t *rowptr_s, const int32_t *eid_s, const int32_t *dst_s,
                          const int64_t *layers, int64_t L, int64_t H, float residual, const float *start, int64_t N, int64_t E,
                          int64_t B, int64_t nmax, float *relevance, float *edge_flow, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_ROLLOUT_H */
