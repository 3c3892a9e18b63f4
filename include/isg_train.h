/* Training of the question side: the backward kernels of the short-sequence attention and of add + LayerNorm, and dropout that
 * a backward regenerates instead of reading a stored mask (csrc/isg_text_bwd.hip).
 *
 * Second device header of libisg_hip.so, beside include/isg.h (whose status codes and conventions hold here: fp32 device
 * pointers, `ld*` = row stride in elements, `stream` = hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).
 * It has an ABI version of its own, so the inference ABI of isg.h does not move when a training entry point does.
 *
 * THE KEEP RULE, one convention for every entry point below.  Under a 64-bit `seed` and a drop probability 0 <= p < 1
 * (ISG_EINVAL otherwise), element (i, j) of an [M, D] operand is KEPT iff
 *     uniform24(word[j & 3] of philox4x32_10((i, j >> 2, 0x1571, 0x9E37), (seed & 0xffffffff, seed >> 32))) >= p
 * compared in fp32, uniform24(w) = (float)(w >> 8) * 2^-24 (csrc/isg_common.hpp::Philox, oracle/philox.py); a survivor is
 * multiplied by 1.0f / (1.0f - p), a dropped element is 0.  For the attention probabilities i = (b * H + h) * Tq + t and j = s
 * (the key).  At p == 0 nothing is drawn and the call is the inference kernel's arithmetic bit for bit.
 * No kernel here uses an atomic in global memory: two identical calls give the same bits.
 */
#ifndef ISG_TRAIN_H
#define ISG_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_TRAIN_ABI_VERSION 1

int isg_train_abi_version(void);

/* out = x * keep / (1 - p) on [M, D] rows.  The backward is the same call on the gradient.  x may alias out.
 * ISG_EUNSUPPORTED unless 4 | D, 4 | ld*, 16-byte aligned rows, M < 2^31. */
int isg_dropout(const float *x, int32_t ldx, float *out, int32_t ldo, int64_t M, int32_t D, float p, uint64_t seed, void *stream);

/* isg_mha_small's heads form with dropout on the attention probabilities, as nn.MultiheadAttention has it in training:
 * out = (P * keep / (1 - p)) V with P = softmax(Q K^T / sqrt(hd) + key_bias).  Operands and limits of isg_mha_small (hd <= 64,
 * 4 | hd, Tk <= 128, 16-byte aligned rows, 64 KB of LDS); at p == 0 it IS isg_mha_small. */
int isg_mha_small_train(const float *q, int32_t ldq, const float *k, int32_t ldk, const float *v, int32_t ldv, const float *key_bias,
                        float *out, int32_t ldo, int64_t B, int32_t H, int32_t hd, int32_t Tq, int32_t Tk, float p, uint64_t seed,
                        void *stream);

/* The backward of both: P is recomputed with the forward's arithmetic (same order, same expf and divide), then with
 * P~ = P * keep / (1 - p):  dV[s] = sum_t P~[t,s] dO[t];  dP~[t,s] = <dO[t], V[s]>;  dP = dP~ * keep / (1 - p);
 * dS = P * (dP - sum_s P dP);  dQ[t] = scale * sum_s dS[t,s] K[s];  dK[s] = scale * sum_t dS[t,s] Q[t], the sums over t in
 * ascending order inside one workgroup per (batch item, head).  d_q / d_k / d_v may be column slices of one [T*B, 3D] gradient
 * (their strides are ldq / ldk / ldv of their own: lddq / lddk / lddv).  key_bias (optional) gets no gradient.
 * Q, K, V, dO and the [Tq][Tk] strips of P~ and dS live in LDS: 4 * (2 Tk (hd + 4) + 2 Tq hd + 2 Tq Tk) bytes, at most 160 KB
 * (CLIP's 77 x 77 keys at hd = 64: 126 KB); beyond that, and outside isg_mha_small's limits, ISG_EUNSUPPORTED. */
int isg_mha_small_bwd(const float *q, int32_t ldq, const float *k, int32_t ldk, const float *v, int32_t ldv, const float *key_bias,
                      const float *d_out, int32_t lddo, float *d_q, int32_t lddq, float *d_k, int32_t lddk, float *d_v, int32_t lddv,
                      int64_t B, int32_t H, int32_t hd, int32_t Tq, int32_t Tk, float p, uint64_t seed, void *stream);
/* The LDS bytes isg_mha_small_bwd asks for (what the 160 KB bound is held against). */
int64_t isg_mha_small_bwd_lds_bytes(int32_t hd, int32_t Tq, int32_t Tk);

/* out = LayerNorm(r + dropout(x)), the post-norm step of nn.TransformerEncoderLayer / DecoderLayer in training, with
 * isg_add_layernorm's arithmetic (mean, the residue pass, biased variance).  r and beta optional.  At p == 0 it IS
 * isg_add_layernorm.  4 | D, D <= 2048, 16-byte aligned rows, M < 2^31 (ISG_EUNSUPPORTED otherwise). */
int isg_dropout_add_layernorm(const float *x, int32_t ldx, const float *r, int32_t ldr, const float *gamma, const float *beta,
                              float eps, float *out, int32_t ldo, int64_t M, int32_t D, float p, uint64_t seed, void *stream);

/* Its backward.  Nothing is saved by the forward but its inputs: a wave per row recomputes v = r + dropout(x) and the row's
 * statistics, then d_v = rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = d_out * gamma;  d_r = d_v (d_r optional),
 * d_x = d_v * keep / (1 - p).  d_gamma / d_beta leave as ONE PARTIAL ROW PER WORKGROUP, fp32 [isg_add_layernorm_bwd_parts(M), D]
 * each (d_beta_part optional), which the caller sums over the parts in fixed order.  Limits of the forward. */
int isg_add_layernorm_bwd(const float *x, int32_t ldx, const float *r, int32_t ldr, const float *gamma, float eps, const float *d_out,
                          int32_t lddo, float *d_x, int32_t lddx, float *d_r, int32_t lddr, float *d_gamma_part, float *d_beta_part,
                          int64_t M, int32_t D, float p, uint64_t seed, void *stream);
int32_t isg_add_layernorm_bwd_parts(int64_t M);

#ifdef __cplusplus
}
#endif

#endif /* ISG_TRAIN_H */
