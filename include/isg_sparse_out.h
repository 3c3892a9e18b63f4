/* The masked MaskingGATv2Conv layer with `out` written only where it is read (csrc/isg_layer_conv.hip).
 *
 * Twelfth device header of libisg_hip.so (the status codes and conventions of isg.h hold: raw device pointers, `ld*` = row stride
 * in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its
 * own: isg.h and isg_masked.h did not move when it came, and neither moves when an entry point here does.
 *
 * It also relaxes one documented contract of the two older layer entry points without touching their signatures: `alpha` may be
 * NULL in isg_gatv2_layer_conv (include/isg.h), isg_gatv2_layer_conv_tables (include/isg_masked.h) and the entry point below.
 * The attention weights are then not stored; out / rowmax / row_dead keep their bits.
 */
#ifndef ISG_SPARSE_OUT_H
#define ISG_SPARSE_OUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_SPARSE_OUT_ABI_VERSION 1

int isg_sparse_out_abi_version(void);

/* Flag of isg_gatv2_layer_conv_sparse.  A masked launch on groups of tiles writes a row of `out` / `rowmax` that no live slot has
 * as destination -- `+0 + bias` and that vector's maxima, the same in every such row -- for ONE row per tile only: the tile's first
 * such row.  The tile's other such rows keep row_dead = 1 in every head (and their alpha entries) and are otherwise NOT WRITTEN:
 * what the buffers held before stays.  Every row with a live in-slot is written as always.  A reader takes a row whose H flags
 * are all set from the FIRST such row of its tile: that row is always written (it is the one row of its kind that the launch
 * stores, or a row before it that the aggregation wrote and found dead).  Launches that do not run on groups of tiles -- a group
 * size of 1, ISG_LC_DENSE_MASK=1, ISG_LC_AGG_ALL_ROWS=1, a group whose node list passes 64 rows -- write every row, and
 * ISG_LC_DENSE_OUT=1 (read once per process) makes every launch do so: the A/B switch.  The rows that are written hold the same
 * bits either way. */
#define ISG_LC_SPARSE_OUT 1

/* isg_gatv2_layer_conv_tables (include/isg_masked.h) with a flag word behind live_tables: 0 = that function, bit for bit;
 * ISG_LC_SPARSE_OUT as above, which needs row_dead and one of the masks (ISG_EINVAL without); any other bit: ISG_EINVAL.
 * live_tables may be NULL (ISG_LC_TABLES=0 scans the tiles in the kernel): the rule is the same. */
int isg_gatv2_layer_conv_sparse(const uint16_t *x_planes, const float *x_inv_scale, const uint16_t *wn_frag, const float *wn_inv_scale,
                                const float *bn, const uint16_t *edge_planes, const float *edge_inv_scale, const uint16_t *we_frag,
                                const float *we_inv_scale, const float *att, const float *bias, const int32_t *rowptr,
                                const int32_t *eid, const int32_t *src, const int32_t *dst, const int32_t *tile_info,
                                const int32_t *ntiles, int64_t max_tiles, const float *node_mask, const float *edge_mask,
                                float *out, int32_t ldo, float *alpha, float *rowmax, uint8_t *row_dead, const uint8_t *live_tables,
                                int32_t flags, int64_t N, int64_t E, int32_t H, int32_t C, int32_t K_in, int32_t K_edge,
                                float negative_slope, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_SPARSE_OUT_H */
