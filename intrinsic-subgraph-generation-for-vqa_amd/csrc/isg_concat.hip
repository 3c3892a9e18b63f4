// concat_instr training (include/isg_concat.h): the gradient of the per-graph bias rows of isg_linear_bf16x6_rowbias.
//
// dP[s, :] = sum of dz[m, :] over the rows m of segment s.  A batch vector is sorted, so a segment is a RANGE of rows
// [rowptr[s], rowptr[s + 1]): one workgroup per (segment, block of columns), one thread per float4 column, the rows added in row
// order -- no atomics, the order of every sum a function of rowptr alone, so two calls agree bit for bit.  Every row of dz is
// read once, in full 16-byte lanes along the row.  (isg_segment_rows_sum walks 256-slot pieces with sixteen lanes each, which suits
// the scene-graph encoder's index lists; on 82 286 rows of 1024 columns it leaves most of the chip idle and takes 1014 us, which
// made a concat layer's training step slower than the literal concatenation: DESIGN.md 29.)
#include "isg_common.hpp"

#include <type_traits>

#include "../../include/isg_concat.h"

namespace isg {

constexpr int SRS_U = 4;   // rows in flight per thread

template <bool V4>
__global__ __launch_bounds__(256) void segment_range_sum_kernel(const int *__restrict__ rowptr, const float *__restrict__ G,
                                                                int64_t ldg, float *__restrict__ out, int64_t ldo, int M, int C) {
  typedef typename std::conditional<V4, float4, float>::type T;
  constexpr int W = V4 ? 4 : 1;
  const int s = blockIdx.x;
  const int c = (blockIdx.y * blockDim.x + threadIdx.x) * W;
  if (c >= C) return;
  // rowptr is trusted to be non-decreasing; the clamps keep a bad one inside G
  const int rb = max(0, min(rowptr[s], M)), re = max(rb, min(rowptr[s + 1], M));
  float acc[W];
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.f;
  for (int r0 = rb; r0 < re; r0 += SRS_U) {
    T g[SRS_U];
#pragma unroll
    for (int u = 0; u < SRS_U; ++u) g[u] = *reinterpret_cast<const T *>(G + (int64_t)min(r0 + u, re - 1) * ldg + c);
#pragma unroll
    for (int u = 0; u < SRS_U; ++u) {
      if (r0 + u < re) {   // row order: row u is added before row u + 1
        const float *v = reinterpret_cast<const float *>(&g[u]);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] += v[i];
      }
    }
  }
  *reinterpret_cast<T *>(out + (int64_t)s * ldo + c) = *reinterpret_cast<const T *>(acc);
}

}  // namespace isg

using namespace isg;

extern "C" int isg_segment_range_sum(const int32_t *rowptr, const float *g, int32_t ldg, float *out, int32_t ldo, int32_t S,
                                     int64_t M, int32_t C, void *stream) {
  if (S < 0 || M < 0 || C <= 0 || ldg < C || ldo < C) return ISG_EINVAL;
  if (S == 0) return ISG_OK;
  if (!rowptr || !out || (M > 0 && !g)) return ISG_EINVAL;
  if (M >= (1ll << 31)) return ISG_EUNSUPPORTED;
  const bool v4 = (C & 3) == 0 && (ldg & 3) == 0 && (ldo & 3) == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int cols = v4 ? C / 4 : C;                       // columns of threads
  const int threads = cols <= 64 ? 64 : cols <= 128 ? 128 : 256;
  const long long by = (cols + threads - 1) / threads;
  if (by > 65535) return ISG_EUNSUPPORTED;
  dim3 grid((unsigned)S, (unsigned)by);
  if (v4) segment_range_sum_kernel<true><<<grid, threads, 0, as_stream(stream)>>>(rowptr, g, ldg, out, ldo, (int)M, C);
  else segment_range_sum_kernel<false><<<grid, threads, 0, as_stream(stream)>>>(rowptr, g, ldg, out, ldo, (int)M, C);
  return check_launch();
}
