// Integrated gradients on a batch of graph instances (include/ext/isg_ig.h, where both functions are stated word for word): the
// rows of the path's points as one instance batch, and the gradient rows of that batch reduced to one attribution per parent row.
//
// Both kernels are bandwidth-bound, use no LDS and no matrix work, and share the work mapping of instance_rows_kernel
// (csrc/isg_instances.hip) and instance_rows_bwd_kernel (csrc/isg_instances_bwd.hip): sixteen lanes per OUTPUT row, 16 bytes per
// lane and access, one launch for the node half and the edge half.  The attribution finds a row's graph by a binary search over
// the G + 1 range starts, walks the row's copies IG_K at a time (their loads in flight together, the fma chain in the order of
// the list), and combines the sixteen lanes' partial sums by a fixed xor-butterfly inside the lane group.  No atomics, one
// writer per output word.  Every number read from memory that becomes an address is compared first.
#include "isg_common.hpp"

#include "../../include/ext/isg_ig.h"

namespace isg {

constexpr int IG_THREADS = 256, IG_LANES = 16, IG_ROWS_PER_BLOCK = IG_THREADS / IG_LANES;
constexpr int IG_U = 5;          // float4 per lane and pass of the path rows: 300 channels are 75 float4, five per lane
constexpr int IG_K = 4;          // copies whose loads are in flight together

__device__ __forceinline__ float fma_1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

struct IgPathArgs {
  const float *x;                // [x_rows, 4 Cx4] row stride ldx; may be NULL when n_out == 0
  int64_t ldx;
  int64_t x_rows;
  const float *b_x;              // optional baseline: NULL = zeros; ldbx == 0: one row
  int64_t ldbx;
  const int64_t *node_src;       // may be NULL when n_out == 0
  const int64_t *inst_of;        // may be NULL when n_out == 0
  int64_t n_out;
  float *x_out;                  // may be NULL when n_out == 0
  int64_t ldxo;
  int Cx4;                       // float4 per row
  const float *e;                // may be NULL when m_out == 0
  int64_t lde;
  int64_t e_rows;
  const float *b_e;              // optional baseline, as b_x
  int64_t ldbe;
  const int64_t *edge_src;       // may be NULL when m_out == 0
  const int64_t *einst_of;       // may be NULL when m_out == 0 or path_e == 0
  int64_t m_out;
  float *e_out;                  // may be NULL when m_out == 0
  int64_t ldeo;
  int Ce4;
  const float *t;                // [Q]; may be NULL when no interpolated half has rows
  int Q;
  int path_e;
};

__global__ __launch_bounds__(IG_THREADS) void ig_path_rows_kernel(IgPathArgs a) {
  const int lane = threadIdx.x & (IG_LANES - 1);
  int64_t r = (int64_t)blockIdx.x * IG_ROWS_PER_BLOCK + threadIdx.x / IG_LANES;
  const bool nodes = r < a.n_out;
  if (!nodes) r -= a.n_out;
  if (!nodes && r >= a.m_out) return;
  const int64_t s = nodes ? a.node_src[r] : a.edge_src[r];
  if (s < 0 || s >= (nodes ? a.x_rows : a.e_rows)) return;
  const bool path = nodes || a.path_e != 0;
  float tq = 1.f, omt = 0.f;
  if (path) {
    const int64_t q = nodes ? a.inst_of[r] : a.einst_of[r];
    if (q < 0 || q >= a.Q) return;
    tq = a.t[q];
    omt = sub_rn(1.f, tq);
  }
  const float4 *src = reinterpret_cast<const float4 *>(nodes ? a.x + s * a.ldx : a.e + s * a.lde);
  const float *bp = nodes ? a.b_x : a.b_e;
  const float4 *base = (path && bp) ? reinterpret_cast<const float4 *>(bp + s * (nodes ? a.ldbx : a.ldbe)) : nullptr;
  float4 *dst = reinterpret_cast<float4 *>(nodes ? a.x_out + r * a.ldxo : a.e_out + r * a.ldeo);
  const int C4 = nodes ? a.Cx4 : a.Ce4;
  for (int c0 = lane; c0 < C4; c0 += IG_LANES * IG_U) {
    float4 v[IG_U], b[IG_U];
#pragma unroll
    for (int u = 0; u < IG_U; ++u)
      if (c0 + u * IG_LANES < C4) {
        v[u] = src[c0 + u * IG_LANES];
        if (base) b[u] = base[c0 + u * IG_LANES];
      }
#pragma unroll
    for (int u = 0; u < IG_U; ++u)
      if (c0 + u * IG_LANES < C4) {
        float4 o = v[u];
        if (base)
          o = make_float4(fma_1(tq, v[u].x, mul_rn(omt, b[u].x)), fma_1(tq, v[u].y, mul_rn(omt, b[u].y)),
                          fma_1(tq, v[u].z, mul_rn(omt, b[u].z)), fma_1(tq, v[u].w, mul_rn(omt, b[u].w)));
        else if (path)
          o = make_float4(mul_rn(tq, v[u].x), mul_rn(tq, v[u].y), mul_rn(tq, v[u].z), mul_rn(tq, v[u].w));
        dst[c0 + u * IG_LANES] = o;
      }
  }
}

struct IgAttrArgs {
  const float *g_xo;             // [xo_rows, 4 Cx4] row stride ldgx; may be NULL when x_rows == 0 or xo_rows == 0
  int64_t ldgx;
  int64_t xo_rows;
  const float *x;                // [x_rows, 4 Cx4] row stride ldx; may be NULL when x_rows == 0
  int64_t ldx;
  const float *b_x;              // optional baseline: NULL = zeros; ldbx == 0: one row
  int64_t ldbx;
  float *attr_x;                 // [x_rows]; may be NULL when x_rows == 0
  float *avg_x;                  // optional [x_rows, 4 Cx4] row stride ldax
  int64_t ldax;
  int64_t x_rows;
  int Cx4;                       // float4 per row
  const float *g_eo;             // may be NULL when e_rows == 0 or eo_rows == 0
  int64_t ldge;
  int64_t eo_rows;
  const float *e;                // may be NULL when e_rows == 0
  int64_t lde;
  const float *b_e;              // optional baseline, as b_x
  int64_t ldbe;
  float *attr_e;                 // may be NULL when e_rows == 0
  float *avg_e;                  // optional
  int64_t ldae;
  int64_t e_rows;
  int Ce4;
  const float *w;                // [Q]; may be NULL when Q == 0
  const int *ptr;                // int32 [G + 1]: node range of every graph; may be NULL when x_rows == 0
  const int *erange;             // int32 [G + 1]: edge range of every graph; may be NULL when e_rows == 0
  const int *inst_ptr;           // int32 [Q + 1]; may be NULL when x_rows == 0
  const int *inst_eptr;          // int32 [Q + 1]; may be NULL when e_rows == 0
  const int *gptr;               // int32 [G + 1]: range of every graph in glist; may be NULL when there are no rows
  const int *glist;              // int32 [Q]: the instances of every graph, ascending; may be NULL when Q == 0
  int G, Q;
  int accumulate;
};

// one copy of the row: its address (in float4 rows) and weight, or ok == false where a rule of the header skips it
struct IgCopy {
  int64_t row;
  float w;
  bool ok;
};

__device__ __forceinline__ IgCopy ig_copy(const IgAttrArgs &a, const int *iptr, int64_t off, int64_t rows_in, int j) {
  IgCopy c = {0, 0.f, false};
  const int q = a.glist[j];
  if (q >= 0 && q < a.Q) {
    const int64_t b = iptr[q], e = iptr[q + 1];
    c.row = b + off;
    c.ok = b >= 0 && c.row < e && c.row < rows_in;
    if (c.ok) c.w = a.w[q];
  }
  return c;
}

__device__ __forceinline__ float4 fma4_1(float w, const float4 &v, const float4 &acc) {
  return make_float4(fma_1(w, v.x, acc.x), fma_1(w, v.y, acc.y), fma_1(w, v.z, acc.z), fma_1(w, v.w, acc.w));
}

__global__ __launch_bounds__(IG_THREADS) void ig_attribution_kernel(IgAttrArgs a) {
  const int lane = threadIdx.x & (IG_LANES - 1);
  int64_t r = (int64_t)blockIdx.x * IG_ROWS_PER_BLOCK + threadIdx.x / IG_LANES;
  const bool nodes = r < a.x_rows;
  if (!nodes) r -= a.x_rows;
  if (!nodes && r >= a.e_rows) return;                           // (all sixteen lanes of a row leave together)
  const int *range = nodes ? a.ptr : a.erange;
  const int *iptr = nodes ? a.inst_ptr : a.inst_eptr;
  const int64_t rows_in = nodes ? a.xo_rows : a.eo_rows;
  const int C4 = nodes ? a.Cx4 : a.Ce4;
  const float4 *src = reinterpret_cast<const float4 *>(nodes ? a.g_xo : a.g_eo);
  const int64_t ld4 = (nodes ? a.ldgx : a.ldge) >> 2;
  const float4 *xin = reinterpret_cast<const float4 *>(nodes ? a.x + r * a.ldx : a.e + r * a.lde);
  const float *bp = nodes ? a.b_x : a.b_e;
  const float4 *base = bp ? reinterpret_cast<const float4 *>(bp + r * (nodes ? a.ldbx : a.ldbe)) : nullptr;
  float *attr = nodes ? a.attr_x + r : a.attr_e + r;
  float *avgp = nodes ? a.avg_x : a.avg_e;
  float4 *avg = avgp ? reinterpret_cast<float4 *>(avgp + r * (nodes ? a.ldax : a.ldae)) : nullptr;
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
  bool have = false;                                             // some copy passed the rules (the same in all sixteen lanes)
  for (int j = j0; j < j1 && !have; ++j) have = ig_copy(a, iptr, off, rows_in, j).ok;
  float s = 0.f;
  if (have) {
    for (int c = lane; c < C4; c += IG_LANES) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int j = j0;
      for (; j + IG_K <= j1; j += IG_K) {
        IgCopy cp[IG_K];
        float4 v[IG_K];
#pragma unroll
        for (int k = 0; k < IG_K; ++k) cp[k] = ig_copy(a, iptr, off, rows_in, j + k);
#pragma unroll
        for (int k = 0; k < IG_K; ++k)
          if (cp[k].ok) v[k] = src[cp[k].row * ld4 + c];
#pragma unroll
        for (int k = 0; k < IG_K; ++k)
          if (cp[k].ok) acc = fma4_1(cp[k].w, v[k], acc);
      }
      for (; j < j1; ++j) {
        const IgCopy cp = ig_copy(a, iptr, off, rows_in, j);
        if (cp.ok) acc = fma4_1(cp.w, src[cp.row * ld4 + c], acc);
      }
      float4 d = xin[c];
      if (base) {
        const float4 b = base[c];
        d = make_float4(sub_rn(d.x, b.x), sub_rn(d.y, b.y), sub_rn(d.z, b.z), sub_rn(d.w, b.w));
      }
      s = add_rn(s, add_rn(add_rn(add_rn(mul_rn(d.x, acc.x), mul_rn(d.y, acc.y)), mul_rn(d.z, acc.z)), mul_rn(d.w, acc.w)));
      if (avg) {
        if (a.accumulate) {
          const float4 o = avg[c];
          acc = make_float4(add_rn(o.x, acc.x), add_rn(o.y, acc.y), add_rn(o.z, acc.z), add_rn(o.w, acc.w));
        }
        avg[c] = acc;
      }
    }
  } else if (!a.accumulate && avg) {
    for (int c = lane; c < C4; c += IG_LANES) avg[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // the fixed butterfly inside the row's sixteen lanes; every lane of the group is here (`have` and the loop bounds above differ
  // between rows, never inside one)
#pragma unroll
  for (int m = IG_LANES / 2; m > 0; m >>= 1) s = add_rn(s, __shfl_xor(s, m, IG_LANES));
  if (lane == 0) {
    if (!a.accumulate) *attr = have ? s : 0.f;
    else if (have) *attr = add_rn(*attr, s);
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_ig_abi_version(void) { return ISG_IG_ABI_VERSION; }

static inline bool ig_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }
static inline bool ig_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static inline bool ig_bad_base_stride(int32_t ldb, int32_t C) { return ldb < 0 || (ldb != 0 && ldb < C); }

extern "C" int isg_ig_path_rows(const float *x, int32_t ldx, int64_t x_rows, const float *b_x, int32_t ldbx, const int64_t *node_src,
                                const int64_t *inst_of, int64_t n_out, float *x_out, int32_t ldxo, int32_t Cx, const float *e,
                                int32_t lde, int64_t e_rows, const float *b_e, int32_t ldbe, const int64_t *edge_src,
                                const int64_t *einst_of, int64_t m_out, float *e_out, int32_t ldeo, int32_t Ce, const float *t,
                                int64_t Q, int32_t path_e, void *stream) {
  if (n_out < 0 || m_out < 0 || x_rows < 0 || e_rows < 0 || Q < 0) return ISG_EINVAL;
  IgPathArgs a = {.x = x, .ldx = ldx, .x_rows = x_rows, .b_x = b_x, .ldbx = ldbx, .node_src = node_src, .inst_of = inst_of,
                  .n_out = n_out, .x_out = x_out, .ldxo = ldxo, .Cx4 = Cx / 4, .e = e, .lde = lde, .e_rows = e_rows, .b_e = b_e,
                  .ldbe = ldbe, .edge_src = edge_src, .einst_of = einst_of, .m_out = m_out, .e_out = e_out, .ldeo = ldeo,
                  .Ce4 = Ce / 4, .t = t, .Q = (int)Q, .path_e = path_e};
  if (a.n_out > 0 && (Cx < 1 || ldx < Cx || ldxo < Cx || !a.x || !a.node_src || !a.x_out || !a.inst_of || !a.t ||
                      (a.b_x && ig_bad_base_stride(ldbx, Cx))))
    return ISG_EINVAL;
  if (a.m_out > 0 && (Ce < 1 || lde < Ce || ldeo < Ce || !a.e || !a.edge_src || !a.e_out)) return ISG_EINVAL;
  if (a.m_out > 0 && a.path_e && (!a.einst_of || !a.t || (a.b_e && ig_bad_base_stride(ldbe, Ce)))) return ISG_EINVAL;
  if (ig_too_large(n_out) || ig_too_large(m_out) || ig_too_large(Q)) return ISG_EUNSUPPORTED;
  if (a.n_out > 0 && (((Cx | ldx | ldxo) & 3) || ig_misaligned(a.x) || ig_misaligned(a.x_out) ||
                      (a.b_x && ((ldbx & 3) || ig_misaligned(a.b_x)))))
    return ISG_EUNSUPPORTED;
  if (a.m_out > 0 && (((Ce | lde | ldeo) & 3) || ig_misaligned(a.e) || ig_misaligned(a.e_out) ||
                      (a.path_e && a.b_e && ((ldbe & 3) || ig_misaligned(a.b_e)))))
    return ISG_EUNSUPPORTED;
  if (a.n_out == 0 && a.m_out == 0) return ISG_OK;
  const int64_t blocks = (n_out + m_out + IG_ROWS_PER_BLOCK - 1) / IG_ROWS_PER_BLOCK;
  ig_path_rows_kernel<<<(unsigned)blocks, IG_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}

extern "C" int isg_ig_attribution(const float *g_xo, int32_t ldgx, int64_t xo_rows, const float *x, int32_t ldx, const float *b_x,
                                  int32_t ldbx, float *attr_x, float *avg_x, int32_t ldax, int64_t x_rows, int32_t Cx,
                                  const float *g_eo, int32_t ldge, int64_t eo_rows, const float *e, int32_t lde, const float *b_e,
                                  int32_t ldbe, float *attr_e, float *avg_e, int32_t ldae, int64_t e_rows, int32_t Ce, const float *w,
                                  const int32_t *ptr, const int32_t *erange, const int32_t *inst_ptr, const int32_t *inst_eptr,
                                  const int32_t *gptr, const int32_t *glist, int64_t G, int64_t Q, int32_t accumulate, void *stream) {
  if (xo_rows < 0 || x_rows < 0 || eo_rows < 0 || e_rows < 0 || G < 0 || Q < 0) return ISG_EINVAL;
  IgAttrArgs a = {.g_xo = g_xo, .ldgx = ldgx, .xo_rows = xo_rows, .x = x, .ldx = ldx, .b_x = b_x, .ldbx = ldbx, .attr_x = attr_x,
                  .avg_x = avg_x, .ldax = ldax, .x_rows = x_rows, .Cx4 = Cx / 4, .g_eo = g_eo, .ldge = ldge, .eo_rows = eo_rows,
                  .e = e, .lde = lde, .b_e = b_e, .ldbe = ldbe, .attr_e = attr_e, .avg_e = avg_e, .ldae = ldae, .e_rows = e_rows,
                  .Ce4 = Ce / 4, .w = w, .ptr = ptr, .erange = erange, .inst_ptr = inst_ptr, .inst_eptr = inst_eptr, .gptr = gptr,
                  .glist = glist, .G = (int)G, .Q = (int)Q, .accumulate = accumulate};
  if ((a.x_rows > 0 || a.e_rows > 0) && (G == 0 || !a.gptr || (Q > 0 && (!a.glist || !a.w)))) return ISG_EINVAL;
  if (a.x_rows > 0 && (Cx < 1 || ldgx < Cx || ldx < Cx || !a.attr_x || !a.x || !a.ptr || !a.inst_ptr || (a.xo_rows > 0 && !a.g_xo) ||
                       (a.b_x && ig_bad_base_stride(ldbx, Cx)) || (a.avg_x && ldax < Cx)))
    return ISG_EINVAL;
  if (a.e_rows > 0 && (Ce < 1 || ldge < Ce || lde < Ce || !a.attr_e || !a.e || !a.erange || !a.inst_eptr || (a.eo_rows > 0 && !a.g_eo) ||
                       (a.b_e && ig_bad_base_stride(ldbe, Ce)) || (a.avg_e && ldae < Ce)))
    return ISG_EINVAL;
  if (ig_too_large(xo_rows) || ig_too_large(x_rows) || ig_too_large(eo_rows) || ig_too_large(e_rows) || ig_too_large(G) ||
      ig_too_large(Q))
    return ISG_EUNSUPPORTED;
  if (a.x_rows > 0 && (((Cx | ldgx | ldx) & 3) || ig_misaligned(a.x) || (a.xo_rows > 0 && ig_misaligned(a.g_xo)) ||
                       (a.b_x && ((ldbx & 3) || ig_misaligned(a.b_x))) || (a.avg_x && ((ldax & 3) || ig_misaligned(a.avg_x)))))
    return ISG_EUNSUPPORTED;
  if (a.e_rows > 0 && (((Ce | ldge | lde) & 3) || ig_misaligned(a.e) || (a.eo_rows > 0 && ig_misaligned(a.g_eo)) ||
                       (a.b_e && ((ldbe & 3) || ig_misaligned(a.b_e))) || (a.avg_e && ((ldae & 3) || ig_misaligned(a.avg_e)))))
    return ISG_EUNSUPPORTED;
  if (a.x_rows == 0 && a.e_rows == 0) return ISG_OK;
  const int64_t blocks = (x_rows + e_rows + IG_ROWS_PER_BLOCK - 1) / IG_ROWS_PER_BLOCK;
  ig_attribution_kernel<<<(unsigned)blocks, IG_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
