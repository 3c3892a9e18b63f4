// The tensor table's geometry, shared by the kernels that walk one (csrc/isg_optim.hip: the gradient norm and Adam;
// csrc/isg_dist.hip: the gradient bucket's pack).  include/isg_optim.h describes the table; isg_mt_chunk_elems() reports MT_CHUNK.
#pragma once
#include "isg_common.hpp"

namespace isg {

constexpr int MT_CHUNK = 4096;        // elements of one chunk: 4 float4 per lane of a 256-thread workgroup, 112 KB of Adam traffic
constexpr int MT_THREADS = 256;
constexpr int MT_GRID_MAX = 2048;     // 8 workgroups per CU resident at once; the rest of the chunks are strided over

// The tensor of absolute chunk c (prefix[0] <= c < prefix[T]): the largest t with prefix[t] <= c.  Tensors of numel 0 own no
// chunk (prefix[t] == prefix[t + 1]) and are stepped over.  Uniform across the workgroup: the compiler keeps it on the scalar unit.
__device__ __forceinline__ int chunk_tensor(const int64_t *prefix, int T, int64_t c) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// elements in front of the first 16-byte boundary of a 4-byte aligned address
__device__ __forceinline__ int head_elems(const void *p) { return (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2); }

static inline unsigned mt_grid(int64_t chunks) { return (unsigned)(chunks < MT_GRID_MAX ? chunks : MT_GRID_MAX); }

}  // namespace isg
