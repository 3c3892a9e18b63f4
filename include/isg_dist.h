/* Data-parallel training on the device: every gradient packed, scaled, into one flat fp32 bucket (csrc/isg_dist.hip).
 *
 * Sixth device header of libisg_hip.so (the status codes and conventions of include/isg.h hold: raw device pointers, `stream` =
 * hipStream_t or NULL, ISG_OK or a negative ISG_E* status, nothing throws).  It has an ABI version of its own: no other header
 * moves when an entry point here does.
 *
 * The bucket is what one all-reduce sums across the ranks; isg_mt_sqnorm and isg_mt_adam (include/isg_optim.h) then read the
 * reduced gradients in place, through the gradient column of their own table -- there is no unpack pass.
 */
#ifndef ISG_DIST_H
#define ISG_DIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_DIST_ABI_VERSION 1

int isg_dist_abi_version(void);

/* dst[t][i] = scale * src[t][i] (accumulate == 0: one fp32 multiply) or fmaf(scale, src[t][i], dst[t][i]) (accumulate != 0: one
 * rounding) for the T tensors of a table.  `src` and `dst` are device int64 [T]: the address of tensor t's gradient and of its
 * slot in the bucket, fp32, contiguous, 4-byte aligned (a scalar head up to the first 16-byte boundary, a float4 body where source
 * and slot share their offset from one, a scalar tail; scalars throughout where they do not).  `numel` (device int64 [T]),
 * `chunk_prefix` (device int64 [T + 1]) and `total_chunks` are include/isg_optim.h's: chunks of isg_mt_chunk_elems() elements, a
 * workgroup per chunk, the grid capped and striding over the rest.
 * src[t] == 0: tensor t has no gradient on this rank.  Its slot is zeroed, or with `accumulate` left as it is.
 * One launch, no atomic, nothing written outside [dst[t], dst[t] + numel[t]); two identical calls give the same bits.
 * T = 0 and tensors of numel 0 are allowed.  ISG_EINVAL: T < 0, total_chunks < 0, chunks without tensors, a null array with T > 0. */
int isg_mt_pack(const int64_t *src, const int64_t *dst, const int64_t *numel, const int64_t *chunk_prefix, int32_t T,
                int64_t total_chunks, float scale, int32_t accumulate, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ISG_DIST_H */
