// Backward of the instance-row gather (include/ext/isg_instances_train.h): per distinct node / edge row, the sum of the gradient
// rows of its copies in the instance batch, in ascending instance number.
//
// Bandwidth-bound, no LDS, no matrix work; the work mapping of instance_rows_kernel (csrc/isg_instances.hip): sixteen lanes per
// OUTPUT row, 16 bytes per lane and access, one launch for both halves.  The copies of row r of graph g sit at
// inst_ptr[q] + (r - ptr[g]) for the instances q of g, so the inverse needs the [Q] list of instances per graph and no slot
// list; a row finds its graph by a binary search over the G + 1 range starts (the same words for all sixteen lanes).  A long
// chain (one graph asked a thousand times) is one lane group's serial loop: its loads are issued BWD_K copies at a time, the
// adds stay in the order of the list.  No atomics, one writer per output word, one rounding per add.
// Every number read from memory that becomes an address is compared first; a copy that fails is skipped.
#include "isg_common.hpp"

#include "../../include/ext/isg_instances_train.h"

namespace isg {

constexpr int BWD_THREADS = 256, BWD_LANES = 16, BWD_ROWS_PER_BLOCK = BWD_THREADS / BWD_LANES;
constexpr int BWD_U = 5;         // float4 per lane and pass: 300 channels are 75 float4, five per lane
constexpr int BWD_K = 4;         // copies whose loads are in flight together

struct RowsBwdArgs {
  const float *g_xo;             // [xo_rows, 4 Cx4] row stride ldgx; may be NULL when x_rows == 0 or xo_rows == 0
  int64_t ldgx;
  int64_t xo_rows;
  float *d_x;                    // [x_rows, 4 Cx4] row stride lddx; may be NULL when x_rows == 0
  int64_t lddx;
  int64_t x_rows;
  int Cx4;                       // float4 per row
  const float *g_eo;             // may be NULL when e_rows == 0 or eo_rows == 0
  int64_t ldge;
  int64_t eo_rows;
  float *d_e;                    // may be NULL when e_rows == 0
  int64_t ldde;
  int64_t e_rows;
  int Ce4;
  const int *ptr;                // int32 [G + 1]: node range of every graph; may be NULL when x_rows == 0
  const int *erange;             // int32 [G + 1]: edge range of every graph; may be NULL when e_rows == 0
  const int *inst_ptr;           // int32 [Q + 1]; may be NULL when x_rows == 0
  const int *inst_eptr;          // int32 [Q + 1]; may be NULL when e_rows == 0
  const int *gptr;               // int32 [G + 1]: range of every graph in glist
  const int *glist;              // int32 [Q]: the instances of every graph, ascending; may be NULL when Q == 0
  int G, Q;
};

__device__ __forceinline__ float4 add4_rn(const float4 &a, const float4 &b) {
  return make_float4(add_rn(a.x, b.x), add_rn(a.y, b.y), add_rn(a.z, b.z), add_rn(a.w, b.w));
}

__global__ __launch_bounds__(BWD_THREADS) void instance_rows_bwd_kernel(RowsBwdArgs a) {
  const int lane = threadIdx.x & (BWD_LANES - 1);
  int64_t r = (int64_t)blockIdx.x * BWD_ROWS_PER_BLOCK + threadIdx.x / BWD_LANES;
  const bool nodes = r < a.x_rows;
  if (!nodes) r -= a.x_rows;
  if (!nodes && r >= a.e_rows) return;
  const int *range = nodes ? a.ptr : a.erange;
  const int *iptr = nodes ? a.inst_ptr : a.inst_eptr;
  const int64_t rows_in = nodes ? a.xo_rows : a.eo_rows;
  const int C4 = nodes ? a.Cx4 : a.Ce4;
  const float4 *src = reinterpret_cast<const float4 *>(nodes ? a.g_xo : a.g_eo);
  const int64_t ld4 = (nodes ? a.ldgx : a.ldge) >> 2;
  float4 *dst = reinterpret_cast<float4 *>(nodes ? a.d_x + r * a.lddx : a.d_e + r * a.ldde);
  // the first graph whose range ends behind row r (graphs without rows are passed over); indices stay in [0, G]
  int lo = 0, hi = a.G - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)range[mid + 1] > r) hi = mid;
    else lo = mid + 1;
  }
  const int64_t r0 = range[lo], r1 = range[lo + 1];
  int j0 = 0, j1 = 0;
  if (r0 <= r && r < r1 && rows_in > 0) {                        // else: no graph holds this row, or there is nothing to read
    j0 = max(0, min(a.gptr[lo], a.Q));
    j1 = max(j0, min(a.gptr[lo + 1], a.Q));
  }
  const int64_t off = r - r0;
  for (int cb = 0; cb < C4; cb += BWD_LANES * BWD_U) {
    float4 acc[BWD_U];
#pragma unroll
    for (int u = 0; u < BWD_U; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have = false;                                           // (the same in all sixteen lanes of a row)
    for (int j = j0; j < j1; j += BWD_K) {
      int64_t row[BWD_K];
      bool ok[BWD_K];
#pragma unroll
      for (int k = 0; k < BWD_K; ++k) {
        ok[k] = false;
        row[k] = 0;
        if (j + k < j1) {
          const int q = a.glist[j + k];
          if (q >= 0 && q < a.Q) {
            const int64_t b = iptr[q], e = iptr[q + 1];
            row[k] = b + off;
            ok[k] = b >= 0 && row[k] < e && row[k] < rows_in;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < BWD_U; ++u) {
        const int c = cb + lane + u * BWD_LANES;
        if (c < C4) {
          float4 v[BWD_K];
#pragma unroll
          for (int k = 0; k < BWD_K; ++k)
            if (ok[k]) v[k] = src[row[k] * ld4 + c];
          bool h = have;
#pragma unroll
          for (int k = 0; k < BWD_K; ++k)
            if (ok[k]) {
              acc[u] = h ? add4_rn(acc[u], v[k]) : v[k];         // the sum starts from the first copy
              h = true;
            }
        }
      }
#pragma unroll
      for (int k = 0; k < BWD_K; ++k) have = have || ok[k];
    }
#pragma unroll
    for (int u = 0; u < BWD_U; ++u) {
      const int c = cb + lane + u * BWD_LANES;
      if (c < C4) dst[c] = acc[u];
    }
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_instances_train_abi_version(void) { return ISG_INSTANCES_TRAIN_ABI_VERSION; }

static inline bool bwd_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }
static inline bool bwd_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

extern "C" int isg_instance_rows_bwd(const float *g_xo, int32_t ldgx, int64_t xo_rows, float *d_x, int32_t lddx, int64_t x_rows,
                                     int32_t Cx, const float *g_eo, int32_t ldge, int64_t eo_rows, float *d_e, int32_t ldde,
                                     int64_t e_rows, int32_t Ce, const int32_t *ptr, const int32_t *erange, const int32_t *inst_ptr,
                                     const int32_t *inst_eptr, const int32_t *gptr, const int32_t *glist, int64_t G, int64_t Q,
                                     void *stream) {
  if (xo_rows < 0 || x_rows < 0 || eo_rows < 0 || e_rows < 0 || G < 0 || Q < 0) return ISG_EINVAL;
  RowsBwdArgs a = {.g_xo = g_xo, .ldgx = ldgx, .xo_rows = xo_rows, .d_x = d_x, .lddx = lddx, .x_rows = x_rows, .Cx4 = Cx / 4,
                   .g_eo = g_eo, .ldge = ldge, .eo_rows = eo_rows, .d_e = d_e, .ldde = ldde, .e_rows = e_rows, .Ce4 = Ce / 4,
                   .ptr = ptr, .erange = erange, .inst_ptr = inst_ptr, .inst_eptr = inst_eptr, .gptr = gptr, .glist = glist,
                   .G = (int)G, .Q = (int)Q};
  if ((a.x_rows > 0 || a.e_rows > 0) && (G == 0 || !a.gptr || (Q > 0 && !a.glist))) return ISG_EINVAL;
  if (a.x_rows > 0 && (Cx < 1 || ldgx < Cx || lddx < Cx || !a.d_x || !a.ptr || !a.inst_ptr || (a.xo_rows > 0 && !a.g_xo)))
    return ISG_EINVAL;
  if (a.e_rows > 0 && (Ce < 1 || ldge < Ce || ldde < Ce || !a.d_e || !a.erange || !a.inst_eptr || (a.eo_rows > 0 && !a.g_eo)))
    return ISG_EINVAL;
  if (bwd_too_large(xo_rows) || bwd_too_large(x_rows) || bwd_too_large(eo_rows) || bwd_too_large(e_rows) || bwd_too_large(G) ||
      bwd_too_large(Q))
    return ISG_EUNSUPPORTED;
  if (a.x_rows > 0 && (((Cx | ldgx | lddx) & 3) || bwd_misaligned(a.d_x) || (a.xo_rows > 0 && bwd_misaligned(a.g_xo))))
    return ISG_EUNSUPPORTED;
  if (a.e_rows > 0 && (((Ce | ldge | ldde) & 3) || bwd_misaligned(a.d_e) || (a.eo_rows > 0 && bwd_misaligned(a.g_eo))))
    return ISG_EUNSUPPORTED;
  if (a.x_rows == 0 && a.e_rows == 0) return ISG_OK;
  const int64_t blocks = (x_rows + e_rows + BWD_ROWS_PER_BLOCK - 1) / BWD_ROWS_PER_BLOCK;
  instance_rows_bwd_kernel<<<(unsigned)blocks, BWD_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
