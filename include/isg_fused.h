/* Launches that run several small operators of a step as one (csrc/isg_small_mlps.hip).
 *
 * Fourth device header of libisg_hip.so, beside include/isg.h, include/isg_train.h and include/isg_optim.h (the status codes and
 * conventions of isg.h hold: raw device pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a
 * negative ISG_E* status, nothing throws).  It has an ABI version of its own: none of the other headers moves when an entry
 * point here does.  Every entry point here is a drop-in for a sequence of isg.h's entry points and leaves that sequence's bits.
 */
#ifndef ISG_FUSED_H
#define ISG_FUSED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_FUSED_ABI_VERSION 1

int isg_fused_abi_version(void);

/* Up to four narrow MLPs over M rows each as ONE launch: chain = Linear(+GELU) or Linear, GELU, Linear(+GELU), every width a
 * multiple of 32 in [32, 128] -- the question side of a step (ISubGVQA/models/masking.py:152 of every masked layer,
 * att_pooling.py:66), whose Linears would each run alone on 32 workgroups of isg_linear_bf16x6.  A workgroup takes 32 rows of
 * one chain; a two-Linear chain keeps its intermediate in LDS.  Every output bit is isg_linear_bf16x6's, run Linear by Linear
 * (same split, MFMA shape, k order, product order, bias / GELU epilogue).
 * chains: HOST int64 [n_chains][ISG_SMALL_MLPS_FIELDS], read before the call returns:
 *   0 x (fp32 [M, K1], device address)   1 row stride of x   2 out (fp32 [M, last N])   3 row stride of out   4 Linears (1 or 2)
 *   5 w1 planes (isg_split_bf16x3 of [N1, K1])   6 bias1 fp32 [N1] or 0   7 N1   8 K1   9 act1 (0 none, 1 exact GELU)
 *   10 w2 planes ([N2, N1])   11 bias2 or 0   12 N2   13 K2 (= N1)   14 act2            (10..14 are not read with one Linear)
 * ISG_EUNSUPPORTED for a width outside the rule, an address that is not 16-byte aligned, a row stride that is no multiple
 * of 4, or when ISG_GEMM_KROT / ISG_GEMM_DUAL_K give isg_linear_bf16x6 another accumulation order. */
#define ISG_SMALL_MLPS_FIELDS 15
#define ISG_SMALL_MLPS_MAX_CHAINS 4
#define ISG_SMALL_MLPS_MAX_WIDTH 128
int isg_small_mlps(const int64_t *chains, int32_t n_chains, int64_t M, void *stream);

/* d[M,N] = act(cat(a, b, a * b) @ W[N,3C]^T + bias) without the concatenation in memory (csrc/isg_catmul_linear.hip): the answer
 * head's embedding Linear (isubgvqa.py:288-291) on 32-row x 128-column blocks.  Every output bit -- d and d_rowmax -- is that of
 * isg_cat_mul_rowmax followed by isg_linear_f16x3_tile (one K-chunk, its default 16x16x32 MFMA form).
 * a, b fp32 [M, C] contiguous; w_planes / w_inv_scale from isg_split_f16x2_rows of the [N, 3C] weight; bias fp32 [N] or NULL;
 * d fp32 (row stride ldd); d_rowmax NULL or fp32 [M, N / 32] (written); act 0 none, 1 exact GELU.
 * ISG_EUNSUPPORTED unless 32 | C, C <= ISG_CATMUL_MAX_C, 32 | N, a / b / w_planes 16-byte aligned, at most 65535 row blocks;
 * and when ISG_F16X3_MFMA=32 gives isg_linear_f16x3_tile another accumulation order. */
#define ISG_CATMUL_MAX_C 128
int isg_linear_f16x3_catmul(const float *a, const float *b, const uint16_t *w_planes, const float *w_inv_scale,
                            const float *bias, float *d, float *d_rowmax, int64_t M, int32_t N, int32_t C, int32_t ldd,
                            int32_t act, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_FUSED_H */
