/* --concat_instr models: a Linear whose bias is a ROW per segment (csrc/isg_gemm.hip) and that row's gradient (csrc/isg_concat.hip);
 * DESIGN.md 29.
 *
 * Fourteenth device header of libisg_hip.so (the status codes and conventions of isg.h hold: device pointers, `ld*` = row stride
 * in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its
 * own: none of the other headers moves when an entry point here does.
 *
 * THE FUNCTION.  With concat_instr a MaskingGATv2Conv projects cat(x, u[batch]), 2C wide (mgat_v2_conv.py:153-154).  The
 * concatenation is never formed:
 *     cat(x, u[batch]) . W^T + b  =  x . W[:, :C]^T  +  (u . W[:, C:]^T + b)[batch]
 * The first term is the N-row GEMM at K = C, the second a B-row GEMM whose result P is one bias row per graph.  The entry point
 * below is isg_linear_bf16x6_f16 (fp32 rows in) with `+ P[seg[m], :]` where that one adds `+ bias[:]`: the same kernel, the same
 * six bf16 products per pair of fp32 values, one fp32 add per element in the epilogue, then the activation.
 */
#ifndef ISG_CONCAT_H
#define ISG_CONCAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_CONCAT_ABI_VERSION 1

int isg_concat_abi_version(void);

/* D[m, :N] = act(A[m, :K] . W[:, :K]^T + P[seg[m], :N]), act: 0 none, 1 exact GELU, 2 ReLU (fp32 D only).
 * a [M, K] fp32, row stride lda; w_planes: isg_split_bf16x3 of W [N, K]; p [S, N] fp32, row stride ldp >= N (it may be a column
 * slice of a wider tensor); seg [M] int32, values in [0, S), trusted like every index the forward kernels take; d [M, N] fp32 or,
 * with d_is_f16, IEEE half (one round-to-nearest-even after the add and the activation), row stride ldd in elements of d.
 * With S = 1 and seg = 0 the result equals isg_linear_bf16x6(bias = p) bit for bit.
 * ISG_EINVAL: a missing pointer with M > 0, ldp < N, S < 1, and whatever isg_linear_bf16x6 calls invalid.  ISG_EUNSUPPORTED:
 * wherever isg_linear_bf16x6 says so (4 !| K, 4 !| lda, a misaligned a, more than 65535 row tiles), and ReLU with d_is_f16.
 * M == 0: ISG_OK, nothing is written. */
int isg_linear_bf16x6_rowbias(const float *a, const uint16_t *w_planes, const float *p, int32_t ldp, const int32_t *seg, int32_t S,
                              void *d, int32_t d_is_f16, int64_t M, int32_t N, int32_t K, int32_t lda, int32_t ldd, int32_t act,
                              void *stream);

/* The gradient of p: out[s, :C] = the sum of g[m, :C] over the rows m in [rowptr[s], rowptr[s + 1]), added in row order (no atomics:
 * two calls agree bit for bit); a segment without rows is written as zeros.  rowptr [S + 1] int32, non-decreasing, rowptr[0] >= 0,
 * rowptr[S] <= M (a batch's node ranges; trusted, clamped to [0, M]); g [M, C] fp32, row stride ldg; out [S, C] fp32, row stride
 * ldo (column slices of wider tensors are fine; 16-byte aligned pointers with 4 | C, ldg, ldo take the vector path).
 * ISG_EINVAL: a negative count, C < 1, ldg < C, ldo < C, a missing pointer with S > 0.  ISG_EUNSUPPORTED: M >= 2^31, or more than
 * 65535 column blocks.  S == 0: ISG_OK, nothing is written. */
int isg_segment_range_sum(const int32_t *rowptr, const float *g, int32_t ldg, float *out, int32_t ldo, int32_t S, int64_t M,
                          int32_t C, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISG_CONCAT_H */
