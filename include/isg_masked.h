/* The masked MaskingGATv2Conv layer with its live tables built ONCE per launch (csrc/isg_live_tables.hip, csrc/isg_layer_conv.hip).
 *
 * Eighth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `ld*` = row stride
 * in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its
 * own: none of the other headers moves when an entry point here does.
 *
 * A masked isg_gatv2_layer_conv on groups of tiles turns every tile's CSR slots and masks into a table set in
 * LDS before it computes anything, once per (tile, head).  The tables depend on neither the head nor the weights.  Here a
 * pre-pass writes every tile's table set to memory once per launch, in the byte layout the kernel keeps in LDS, and the kernel
 * copies them in.  out / alpha / rowmax / row_dead are isg_gatv2_layer_conv's bits: the same table values reach
 * the same code.
 *
 * One tile's image, ISG_LIVE_TABLES_TILE_BYTES = 4176 bytes; tile t of the list is at byte t * 4176 of the buffer.  With
 * {r0, nrows, e0, ne} the tile's entry, nr = min(nrows, 64), n = min(ne, 256), slot s = CSR slot e0 + s, mask(s) =
 * edge_mask[eid] if edge_mask else node_mask[src] * node_mask[dst], live(s) = s < n and (bits of mask(s) & 0x7fffffff) != 0:
 *      0  int32 [256][2]  {eid, bits of mask(s)}; {0, bits of 1.0f} for s >= n
 *   2048  float [256]     +0 for a dead slot, edge_inv_scale[e0 + s] for a live one
 *   3072  uint8 [256]     source row in the tile, min(max(src - r0, 0), max(nr - 1, 0)); 0 for s >= n
 *   3328  uint8 [256]     destination row in the tile, clamped alike
 *   3584  uint8 [256]     the live slots in CSR order; zeros behind them
 *   3840  int32 [68]      rowptr[r0 + i] - e0 for i <= nr; zeros behind them
 *   4112  int32 [4]       {r0, nr, e0, n}
 *   4128  uint64          bit r set: a live slot's source or destination is tile row r;  then 8 zero bytes
 *   4144  uint64 [4]      live-slot words: bit (s & 63) of word (s >> 6)
 */
#ifndef ISG_MASKED_H
#define ISG_MASKED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_MASKED_ABI_VERSION 1

int isg_masked_abi_version(void);

#define ISG_LIVE_TABLES_TILE_BYTES 4176

/* Bytes of the table buffer for a tile list of `capacity` entries (capacity * ISG_LIVE_TABLES_TILE_BYTES); negative capacity: 0. */
int64_t isg_layer_conv_live_tables_bytes(int64_t capacity);

/* The pre-pass: image t of `tables` from entry t of tile_info, for t < *ntiles (one 256-thread workgroup per entry, `capacity`
 * of them; entries at and behind *ntiles are left unwritten).  rowptr / eid / src / dst / tile_info / ntiles: the CSR and the
 * tile list that isg_gatv2_layer_conv_tables will be handed -- the SAME list in the same order, since the kernel finds an image
 * by its position.  edge_inv_scale fp32 [E] as isg_edge_planes wrote it.  Exactly one mask form is read: edge_mask fp32 [E] when
 * given, else node_mask fp32 [N]; ISG_EINVAL with neither.  tables: 16-byte aligned, isg_layer_conv_live_tables_bytes(capacity)
 * bytes, fully overwritten for t < *ntiles by plain vector stores. */
int isg_layer_conv_live_tables(const int32_t *rowptr, const int32_t *eid, const int32_t *src, const int32_t *dst,
                               const float *edge_inv_scale, const int32_t *tile_info, const int32_t *ntiles, int64_t capacity,
                               const float *node_mask, const float *edge_mask, uint8_t *tables, int64_t N, int64_t E, void *stream);

/* Tiles per group that isg_gatv2_layer_conv / isg_gatv2_layer_conv_tables pick for a masked launch of this shape on the current
 * device (ISG_LC_GROUP forces it): 1 = the per-tile kernel runs and no tables are read. */
int32_t isg_gatv2_layer_conv_group(int64_t N, int64_t E, int32_t H, int64_t max_tiles);

/* 0 when ISG_LC_TABLES=0 (read once per process) makes isg_gatv2_layer_conv_tables ignore its tables -- the A/B switch -- else 1. */
int32_t isg_layer_conv_live_tables_enabled(void);

/* isg_gatv2_layer_conv (include/isg.h) with its parameters in its order, and live_tables behind row_dead: the buffer
 * isg_layer_conv_live_tables filled on the same stream from the same CSR, tile list and masks.  NULL, an unmasked launch, a
 * group size of 1, ISG_LC_DENSE_MASK=1 or ISG_LC_TABLES=0: isg_gatv2_layer_conv itself.  ISG_EUNSUPPORTED for a buffer that is
 * not 16-byte aligned. */
int isg_gatv2_layer_conv_tables(const uint16_t *x_planes, const float *x_inv_scale, const uint16_t *wn_frag, const float *wn_inv_scale,
                                const float *bn, const uint16_t *edge_planes, const float *edge_inv_scale, const uint16_t *we_frag,
                                const float *we_inv_scale, const float *att, const float *bias, const int32_t *rowptr,
                                const int32_t *eid, const int32_t *src, const int32_t *dst, const int32_t *tile_info,
                                const int32_t *ntiles, int64_t max_tiles, const float *node_mask, const float *edge_mask,
                                float *out, int32_t ldo, float *alpha, float *rowmax, uint8_t *row_dead, const uint8_t *live_tables,
                                int64_t N, int64_t E, int32_t H, int32_t C, int32_t K_in, int32_t K_edge, float negative_slope,
                                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_MASKED_H */
