/* A Linear's backward on the device: the activation's derivative and the bias gradient in one pass over the upstream gradient,
 * and the weight gradient on the bf16 matrix cores (csrc/isg_linear_bwd.hip).
 *
 * Seventh device header of libisg_hip.so (the status codes and conventions of include/isg.h hold: raw device pointers, `stream` =
 * hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws; every refusal below is returned before any launch).  It
 * has an ABI version of its own: no other header moves when an entry point here does.
 *
 * Buffers are the caller's.  No kernel here uses an atomic in global memory and every sum runs in a fixed order: two identical
 * calls give the same bits.
 */
#ifndef ISG_LINEAR_TRAIN_H
#define ISG_LINEAR_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_LINEAR_TRAIN_ABI_VERSION 1

int isg_linear_train_abi_version(void);

/* Host only: the number P of partial rows (1 <= P <= 1024, P <= max(M, 1)) that isg_linear_bwd_prep writes into db_part for an
 * [M, N] gradient.  Workgroup p owns the rows [p R, min(M, (p + 1) R)), R = ceil(M / P); it takes them at most 256 at a time. */
int64_t isg_linear_bwd_prep_parts(int64_t M, int32_t N);

/* One pass over g [M, N] (fp32, row pitch ldg):
 *   mode 0 (identity)  dz = g.  dz may be null: then only db_part is written and g is not copied.
 *   mode 1 (GELU)      saved = the pre-activation z;  dz = g * (Phi(z) + z phi(z)), the exact (erf) form.
 *   mode 2 (ReLU)      saved = the forward's result y;  dz = g * (y > 0 ? 1.0f : 0.0f) -- a multiply, not a select: a nonfinite
 *                      g at a masked position gives NaN.
 * dz [M, N] (row pitch lddz) and db_part [P, N] (contiguous, P = isg_linear_bwd_prep_parts(M, N)) are both optional, not both
 * null.  db_part[p][n] = the sum of dz[m][n] over the rows m that workgroup p owns: a workgroup takes its rows in blocks of T
 * consecutive rows (T a power of two <= 256 that depends on N and the tensors' alignment alone), the i-th row it owns adds to
 * chain i mod T in row order, and the T chains are added in chain order.  A workgroup that owns no rows writes zeros.  The caller adds the P rows.
 * Rows need 4-byte alignment only.  Where g, saved and dz share their offset from a 16-byte boundary and every pitch is a multiple
 * of 4 the columns between 16-byte boundaries move as float4, the rest (and everything otherwise) as scalars.
 * M == 0: ISG_OK, no launch, nothing written.
 * ISG_EINVAL: a null g; a null saved with mode != 0; dz and db_part both null; a pitch below N; a mode outside 0..2; M < 0; N <= 0.
 * ISG_EUNSUPPORTED: M >= 2^31. */
int isg_linear_bwd_prep(const float *g, int32_t ldg, const float *saved, int32_t lds, int32_t mode, float *dz, int32_t lddz,
                        float *db_part, int64_t M, int32_t N, void *stream);

/* Host only: the number of row splits isg_linear_wgrad_bf16x6 is best launched with (1 <= splits <= 65535, at most ceil(M / 256);
 * 0 for an empty shape), like isg_linear_wgrad_splits. */
int64_t isg_linear_wgrad_bf16x6_splits(int64_t M, int32_t N, int32_t K);

/* dW = g^T x for y = x W^T on the bf16 matrix cores: g [M, N] (row pitch ldg) and x [M, K] (row pitch ldx) fp32, each value split
 * exactly into three bf16 terms and the six products of isg_linear_bf16x6 (hi lo, lo hi, mid mid, hi mid, mid hi, hi hi) summed
 * in fp32, small terms first, 16 rows at a time.  partial [splits][N][K] fp32: split z holds the sum over the rows
 * [z R, min(M, (z + 1) R)), R = ceil(M / splits) rounded up to 16; a split with no rows writes zeros.  The caller adds the splits
 * in order.  The domain is isg_linear_bf16x6's: a value that rounds to a bf16 infinity, and any nonfinite value, gives a nonfinite
 * row (g) or column (x) of dW; nothing is clamped.  Rows need 4-byte alignment only.
 * ISG_EINVAL: a null pointer; M < 0, N <= 0 or K <= 0; ldg < N; ldx < K; splits <= 0.
 * ISG_EUNSUPPORTED: M >= 2^31, splits > 65535, more than 65535 tiles of 128 columns in N or in K. */
int isg_linear_wgrad_bf16x6(const float *g, const float *x, float *partial, int64_t M, int32_t N, int32_t K, int32_t ldg,
                            int32_t ldx, int64_t splits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_LINEAR_TRAIN_H */
