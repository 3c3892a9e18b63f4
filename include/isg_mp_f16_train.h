/* Training with fp16 feature rows: the backward of the GATv2 message-passing operator on saved rows stored as IEEE half
 * (csrc/isg_mp_bwd.hip).
 *
 * Thirteenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: device pointers, `ld*` = row stride
 * in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its
 * own: none of the other headers moves when an entry point here does.
 *
 * THE FUNCTION.  With MaskingGATv2Conv.feature_dtype = torch.float16 (BASELINE configs[4], "fp16 features / fp32 accumulate")
 * the projected rows x_l, x_r and e_proj are stored as IEEE half; isg_gatv2_mp_fwd_f16 reads them and every product and sum is
 * fp32.  The backward here reads the same half rows, converts four channels at a time at the point of use (the conversion is
 * exact) and then IS isg_gatv2_mp_bwd: the same two launches, the same fp32 operations in the same order, S in fp64, no atomic.
 * Its results equal, bit for bit, those of isg_gatv2_mp_bwd on the same rows converted to fp32.  Every gradient is fp32.
 */
#ifndef ISG_MP_F16_TRAIN_H
#define ISG_MP_F16_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_MP_F16_TRAIN_ABI_VERSION 1

int isg_mp_f16_train_abi_version(void);

/* isg_gatv2_mp_bwd (isg.h: the CSR by destination and by source, the masks, one partial row of d att per 16 destinations, the
 * limits and the ISG_EUNSUPPORTED cases -- 4 !| C, H outside {1, 2, 4, 8}, more than 8 channel passes -- are the same) with
 * x_l [N, H*C], x_r [N, H*C] and e_proj [E, H*C] as IEEE half.  att, alpha, grad_out, the masks and all five results are fp32.
 * Row strides: ld_l, ld_r, ld_e of x_l, x_r, e_proj in HALVES; ld_dl, ld_dr of d_x_l, d_x_r in FLOATS.  0 = dense (H*C);
 * otherwise a multiple of 4, at least H*C (so x_l | x_r may be the column halves of one [N, 2*H*C] half projection, and
 * d_x_l | d_x_r those of one [N, 2*H*C] fp32 buffer; the columns of a row a pointer does not own are neither read nor written).
 * d_e_proj, d_att_partial, d_edge_mask and grad_out are dense.  The half rows are 8-byte aligned, d_x_l and d_x_r 16-byte.
 * ISG_EINVAL: a stride that is negative, no multiple of 4 or below H*C; a misaligned row pointer; a required pointer missing.
 * N == 0: ISG_OK, nothing is written. */
int isg_gatv2_mp_bwd_f16(const uint16_t *x_l, const uint16_t *x_r, const uint16_t *e_proj, const float *att, const float *alpha,
                         const float *grad_out, const int32_t *rowptr, const int32_t *eid, const int32_t *src,
                         const int32_t *rowptr_s, const int32_t *eid_s, const int32_t *dst_s, const float *node_mask,
                         const float *edge_mask, float *d_x_l, float *d_x_r, float *d_e_proj, float *d_att_partial,
                         float *d_edge_mask, int64_t N, int64_t E, int32_t H, int32_t C, float negative_slope, int32_t ld_l,
                         int32_t ld_r, int32_t ld_e, int32_t ld_dl, int32_t ld_dr, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_MP_F16_TRAIN_H */
