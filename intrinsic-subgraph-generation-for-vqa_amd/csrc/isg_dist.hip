// The gradient bucket's pack (include/isg_dist.h): T gradients, each scaled into its slot of one flat fp32 buffer, in one launch.
//
// A copy with a multiply: 4 B read and 4 B written per element (8 B read when it accumulates), so all there is to do is to keep
// every access 16 bytes wide and every lane busy.  The table's geometry is isg_optim.hip's (isg_mt.hpp): chunks of MT_CHUNK
// elements, a workgroup per chunk found by bisection, a capped grid that strides over the rest.  A gradient is read exactly once
// and never again before the next backward overwrites it: its loads are non-temporal, which leaves the cache to the bucket that
// the all-reduce, the norm and Adam read next.  -DISG_PACK_PLAIN_LOADS builds the kernel with ordinary loads instead, for
// tools/time_train_ddp.py's comparison of the two.
#include "isg_common.hpp"
#include "isg_mt.hpp"
#include "../../include/isg_dist.h"

namespace isg {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#ifdef ISG_PACK_PLAIN_LOADS
#define PACK_LOAD(p) (*(p))
#else
#define PACK_LOAD(p) __builtin_nontemporal_load(p)
#endif
constexpr int PACK_VECS = MT_CHUNK / (4 * MT_THREADS);          // float4 per lane of one chunk
static_assert(PACK_VECS * 4 * MT_THREADS == MT_CHUNK, "a chunk is a whole number of float4 per lane");

struct PackArgs {
  const int64_t *src;        // [T] gradient addresses; an entry 0 = no gradient on this rank
  const int64_t *dst;        // [T] slot addresses
  const int64_t *numel;      // [T]
  const int64_t *prefix;     // [T + 1]
  int T;
  int64_t chunks;
  float scale;
  int accumulate;
};

template <bool ACC>
__device__ __forceinline__ float pack_one(float s, float d, float scale) {
  // the accumulation is an explicit fmaf: one rounding, whatever the compiler would make of `*` and `+`
  return ACC ? fmaf(scale, s, d) : mul_rn(scale, s);
}

template <bool ACC>
__device__ __forceinline__ void pack_chunk(const float *s, float *d, int n, float scale, int tid) {
  // the float4 body needs ONE head for both: the same offset from a 16-byte boundary (chunks are whole multiples of 16 B, so a
  // tensor's chunks all agree).  Slots start on 256 B; a gradient that torch allocated does too, a view at an odd offset may not.
  const int hs = head_elems(s);
  const bool vec = hs == head_elems(d);
  const int head = vec ? min(n, hs) : n, nv = (n - head) >> 2, tail0 = head + 4 * nv;
  for (int i = tid; i < head; i += MT_THREADS) d[i] = pack_one<ACC>(PACK_LOAD(s + i), ACC ? d[i] : 0.f, scale);
  const f32x4 *sv = reinterpret_cast<const f32x4 *>(s + head);
  f32x4 *dv = reinterpret_cast<f32x4 *>(d + head);
  // a chunk is at most PACK_VECS float4 per lane: every load is issued before the first store (the compiler cannot move a load
  // over a store through pointers that may alias, and one 16-byte load in flight per lane does not cover the memory's latency)
  f32x4 s4[PACK_VECS], d4[PACK_VECS];
#pragma unroll
  for (int k = 0; k < PACK_VECS; ++k) {
    const int i = tid + k * MT_THREADS;
    s4[k] = d4[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < nv) {
      s4[k] = PACK_LOAD(sv + i);
      if (ACC) d4[k] = dv[i];
    }
  }
#pragma unroll
  for (int k = 0; k < PACK_VECS; ++k) {
    const int i = tid + k * MT_THREADS;
    if (i < nv) {
      d4[k].x = pack_one<ACC>(s4[k].x, d4[k].x, scale);
      d4[k].y = pack_one<ACC>(s4[k].y, d4[k].y, scale);
      d4[k].z = pack_one<ACC>(s4[k].z, d4[k].z, scale);
      d4[k].w = pack_one<ACC>(s4[k].w, d4[k].w, scale);
      dv[i] = d4[k];
    }
  }
  if (tid < n - tail0) {
    const int i = tail0 + tid;
    d[i] = pack_one<ACC>(PACK_LOAD(s + i), ACC ? d[i] : 0.f, scale);
  }
}

__device__ __forceinline__ void zero_chunk(float *d, int n, int tid) {
  const int head = min(n, head_elems(d)), nv = (n - head) >> 2, tail0 = head + 4 * nv;
  if (tid < head) d[tid] = 0.f;
  f32x4 *dv = reinterpret_cast<f32x4 *>(d + head);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < nv; i += MT_THREADS) dv[i] = z;
  if (tid < n - tail0) d[tail0 + tid] = 0.f;
}

__global__ __launch_bounds__(MT_THREADS) void mt_pack_kernel(PackArgs a) {
  const int tid = threadIdx.x;
  const int64_t base = a.prefix[0];
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    const int t = chunk_tensor(a.prefix, a.T, c + base);
    const int64_t start = (c + base - a.prefix[t]) * MT_CHUNK;
    const int n = (int)max((int64_t)0, min((int64_t)MT_CHUNK, a.numel[t] - start));
    const int64_t src = a.src[t];
    float *d = reinterpret_cast<float *>(a.dst[t]) + start;
    if (src == 0) {                                   // no gradient on this rank: zeros, or nothing to add
      if (!a.accumulate) zero_chunk(d, n, tid);
      continue;
    }
    const float *s = reinterpret_cast<const float *>(src) + start;
    if (a.accumulate) pack_chunk<true>(s, d, n, a.scale, tid);
    else pack_chunk<false>(s, d, n, a.scale, tid);
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_dist_abi_version(void) { return ISG_DIST_ABI_VERSION; }

extern "C" int isg_mt_pack(const int64_t *src, const int64_t *dst, const int64_t *numel, const int64_t *chunk_prefix, int32_t T,
                           int64_t total_chunks, float scale, int32_t accumulate, void *stream) {
  if (T < 0 || total_chunks < 0 || (T == 0 && total_chunks != 0)) return ISG_EINVAL;
  PackArgs a = {.src = src, .dst = dst, .numel = numel, .prefix = chunk_prefix, .T = T, .chunks = total_chunks, .scale = scale,
                .accumulate = accumulate};
  if (a.T > 0 && (!a.src || !a.dst || !a.numel || !a.prefix)) return ISG_EINVAL;
  if (a.chunks == 0) return ISG_OK;
  mt_pack_kernel<<<mt_grid(a.chunks), MT_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
