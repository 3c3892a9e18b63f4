// Many questions per scene graph (include/isg_instances.h): G distinct graphs and an index over Q questions become the batch of Q
// graph instances that Q copies would have made -- maps and renumbered index tensors only; the rows follow in isg_instance_rows.
//
// All integer and exact.  Size pass: (1) one thread per edge position finds where the graph id of the edge list changes and stores
// the per-graph edge ranges -- every entry of eptr[0 .. G] is written by the thread that sees the id pass it, whatever the list
// looks like; (2) ONE workgroup scans the Q instances' node and edge counts in blocks of INST_SCAN_BLOCK.  Fill pass: one wave per
// instance walks its nodes and edges 64 at a time.  No atomics: an output word has one writer, a flag takes a plain store of 1.
// Every number read from memory that becomes an address is clamped first (inst_node_range / inst_edge_range / inst_edge_graph), by
// the same rule in both passes, so a bad ptr, batch, edge_index or index gives wrong rows and never a fault.
#include "isg_common.hpp"

#include "../../include/isg_instances.h"

namespace isg {

constexpr int INST_THREADS = 256, INST_PER = 4, INST_SCAN_BLOCK = INST_THREADS * INST_PER;   // instances one scan step takes
constexpr int INST_WAVES = INST_THREADS / ISG_WAVE;
constexpr long long INST_I32_MAX = 2147483647ll;

struct InstArgs {
  const int *ptr;                // int32 [G + 1]
  const int64_t *batch;          // int64 [N]; NULL in the fill pass, may be NULL when E == 0
  const int64_t *edge_index;     // int64 [2, E]; may be NULL when E == 0
  const int *index;              // int32 [Q]
  int N, E, G, Q;
  int *inst_ptr, *inst_eptr;     // int32 [Q + 1]
  int *status;                   // int32 [4] = {N', E', bad_index, bad_grouping}; NULL in the fill pass
  int *eptr;                     // workspace int32 [G + 1]: edge range of every graph
  int cap_nodes, cap_edges;      // fill pass only
  int64_t *batch_out, *edge_index_out, *node_src, *edge_src;   // NULL in the size pass; may be NULL where the capacity is 0
};

__device__ __forceinline__ void inst_node_range(const InstArgs &a, int g, int &lo, int &hi) {
  lo = max(0, min(a.ptr[g], a.N));
  hi = max(lo, min(a.ptr[g + 1], a.N));
}
__device__ __forceinline__ void inst_edge_range(const InstArgs &a, int g, int &lo, int &hi) {
  lo = max(0, min(a.eptr[g], a.E));
  hi = max(lo, min(a.eptr[g + 1], a.E));
}

// graph of edge e in [0, G); `bad`: an end or its graph id is out of range, or the two ends disagree (the edge then counts as the
// last graph's, which keeps every range inside the list)
__device__ __forceinline__ int inst_edge_graph(const InstArgs &a, int e, bool &bad) {
  const int64_t s = a.edge_index[e], d = a.edge_index[(int64_t)a.E + e];
  if (s < 0 || s >= a.N || d < 0 || d >= a.N) {
    bad = true;
    return a.G - 1;
  }
  const int64_t gs = a.batch[s], gd = a.batch[d];
  if (gd < 0 || gd >= a.G) {
    bad = true;
    return a.G - 1;
  }
  if (gs != gd) bad = true;
  return (int)gd;
}

// thread e of E + 1: the graph ids before and at position e (-1 before the list, G behind it); the ids in (before, at] begin here
__global__ __launch_bounds__(INST_THREADS) void instances_edge_ranges_kernel(InstArgs a) {
  const long long e = (long long)blockIdx.x * INST_THREADS + threadIdx.x;
  if (e > a.E) return;
  bool bad = false;
  const int before = e == 0 ? -1 : inst_edge_graph(a, (int)e - 1, bad);
  bool bad_here = false;
  const int at = e == a.E ? a.G : inst_edge_graph(a, (int)e, bad_here);
  for (int g = before + 1; g <= at; ++g) a.eptr[g] = (int)e;
  if (bad_here || at < before) a.status[3] = 1;       // (`bad` belongs to thread e - 1)
}

__device__ __forceinline__ long long inst_wave_scan(long long v, int lane) {      // inclusive
#pragma unroll
  for (int off = 1; off < ISG_WAVE; off <<= 1) {
    const long long o = __shfl_up(v, off, ISG_WAVE);
    if (lane >= off) v += o;
  }
  return v;
}
__device__ __forceinline__ int inst_sat(long long v) { return (int)(v < INST_I32_MAX ? v : INST_I32_MAX); }

__global__ __launch_bounds__(INST_THREADS) void instances_scan_kernel(InstArgs a) {
  __shared__ long long s_n[INST_WAVES], s_e[INST_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry_n = 0, carry_e = 0;
  bool bad = false;
  for (int base = 0; base < a.Q; base += INST_SCAN_BLOCK) {     // (Q < 2^31 - INST_SCAN_BLOCK: checked on the host)
    int cn[INST_PER], ce[INST_PER];
    long long tn = 0, te = 0;
#pragma unroll
    for (int u = 0; u < INST_PER; ++u) {
      const int q = base + tid * INST_PER + u;
      cn[u] = ce[u] = 0;
      if (q < a.Q) {
        const int g = a.index[q];
        if (g < 0 || g >= a.G) {
          bad = true;
        } else {
          int lo, hi;
          inst_node_range(a, g, lo, hi);
          cn[u] = hi - lo;
          inst_edge_range(a, g, lo, hi);
          ce[u] = hi - lo;
        }
      }
      tn += cn[u];
      te += ce[u];
    }
    const long long in_n = inst_wave_scan(tn, lane), in_e = inst_wave_scan(te, lane);
    if (lane == ISG_WAVE - 1) {
      s_n[wave] = in_n;
      s_e[wave] = in_e;
    }
    __syncthreads();
    long long before_n = carry_n + in_n - tn, before_e = carry_e + in_e - te;
#pragma unroll
    for (int w = 0; w < INST_WAVES; ++w) {
      if (w < wave) {
        before_n += s_n[w];
        before_e += s_e[w];
      }
      carry_n += s_n[w];
      carry_e += s_e[w];
    }
#pragma unroll
    for (int u = 0; u < INST_PER; ++u) {
      const int q = base + tid * INST_PER + u;
      if (q < a.Q) {
        a.inst_ptr[q] = inst_sat(before_n);
        a.inst_eptr[q] = inst_sat(before_e);
      }
      before_n += cn[u];
      before_e += ce[u];
    }
    __syncthreads();                                            // s_n / s_e are rewritten by the next block
  }
  if (tid == 0) {
    a.inst_ptr[a.Q] = a.status[0] = inst_sat(carry_n);
    a.inst_eptr[a.Q] = a.status[1] = inst_sat(carry_e);
  }
  if (bad) a.status[2] = 1;
}

// one wave per instance
__global__ __launch_bounds__(INST_THREADS) void instances_fill_kernel(InstArgs a) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * INST_WAVES + (threadIdx.x >> 6);
  if (q >= a.Q) return;
  const int g = a.index[q];
  if (g < 0 || g >= a.G) return;                                // an empty instance
  int nlo, nhi, elo, ehi;
  inst_node_range(a, g, nlo, nhi);
  inst_edge_range(a, g, elo, ehi);
  const long long n0 = a.inst_ptr[q], e0 = a.inst_eptr[q];
  for (int i = lane; i < nhi - nlo; i += ISG_WAVE) {
    const long long o = n0 + i;
    if (o < 0 || o >= a.cap_nodes) break;
    a.batch_out[o] = q;
    a.node_src[o] = nlo + i;
  }
  const int64_t shift = n0 - nlo;
  for (int j = lane; j < ehi - elo; j += ISG_WAVE) {
    const long long o = e0 + j;
    if (o < 0 || o >= a.cap_edges) break;
    a.edge_src[o] = elo + j;
    a.edge_index_out[o] = a.edge_index[elo + j] + shift;
    a.edge_index_out[(int64_t)a.cap_edges + o] = a.edge_index[(int64_t)a.E + elo + j] + shift;
  }
}

constexpr int ROWS_LANES = 16, ROWS_PER_BLOCK = INST_THREADS / ROWS_LANES, ROWS_U = 5;   // 300 channels: 75 float4, five per lane

struct RowsArgs {
  const float *x;
  int64_t ldx;
  int64_t x_rows;
  const int64_t *node_src;
  int64_t n_out;
  float *x_out;
  int64_t ldxo;
  int Cx4;                       // float4 per row
  const float *e;
  int64_t lde;
  int64_t e_rows;
  const int64_t *edge_src;
  int64_t m_out;
  float *e_out;
  int64_t ldeo;
  int Ce4;
};

__global__ __launch_bounds__(INST_THREADS) void instance_rows_kernel(RowsArgs a) {
  const int lane = threadIdx.x & (ROWS_LANES - 1);
  int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / ROWS_LANES;
  const bool nodes = r < a.n_out;
  if (!nodes) r -= a.n_out;
  if (!nodes && r >= a.m_out) return;
  const int64_t s = nodes ? a.node_src[r] : a.edge_src[r];
  if (s < 0 || s >= (nodes ? a.x_rows : a.e_rows)) return;
  const float4 *src = reinterpret_cast<const float4 *>(nodes ? a.x + s * a.ldx : a.e + s * a.lde);
  float4 *dst = reinterpret_cast<float4 *>(nodes ? a.x_out + r * a.ldxo : a.e_out + r * a.ldeo);
  const int C4 = nodes ? a.Cx4 : a.Ce4;
  for (int c0 = lane; c0 < C4; c0 += ROWS_LANES * ROWS_U) {
    float4 v[ROWS_U];
#pragma unroll
    for (int u = 0; u < ROWS_U; ++u)
      if (c0 + u * ROWS_LANES < C4) v[u] = src[c0 + u * ROWS_LANES];
#pragma unroll
    for (int u = 0; u < ROWS_U; ++u)
      if (c0 + u * ROWS_LANES < C4) dst[c0 + u * ROWS_LANES] = v[u];
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_instances_abi_version(void) { return ISG_INSTANCES_ABI_VERSION; }

extern "C" size_t isg_instances_workspace_bytes(int64_t G) { return G < 0 ? 0 : (size_t)(G + 1) * sizeof(int32_t); }

static inline bool inst_too_large(int64_t v) { return v >= (1ll << 31) - INST_SCAN_BLOCK; }

extern "C" int isg_instances_size(const int32_t *ptr, const int64_t *batch, const int64_t *edge_index, const int32_t *index,
                                  int64_t N, int64_t E, int64_t G, int64_t Q, int32_t *inst_ptr, int32_t *inst_eptr,
                                  int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  if (N < 0 || E < 0 || G < 0 || Q < 0) return ISG_EINVAL;
  if (inst_too_large(N) || inst_too_large(E) || inst_too_large(G) || inst_too_large(Q)) return ISG_EUNSUPPORTED;
  if (Q == 0) return ISG_OK;
  if (G == 0) return ISG_EINVAL;
  InstArgs a = {.ptr = ptr, .batch = batch, .edge_index = edge_index, .index = index, .N = (int)N, .E = (int)E, .G = (int)G,
                .Q = (int)Q, .inst_ptr = inst_ptr, .inst_eptr = inst_eptr, .status = status, .eptr = (int *)workspace,
                .cap_nodes = 0, .cap_edges = 0, .batch_out = nullptr, .edge_index_out = nullptr, .node_src = nullptr,
                .edge_src = nullptr};
  if (!a.ptr || !a.index || !a.inst_ptr || !a.inst_eptr || !a.status || (a.E > 0 && (!a.batch || !a.edge_index))) return ISG_EINVAL;
  if (!a.eptr || workspace_bytes < isg_instances_workspace_bytes(G)) return ISG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(a.status, 0, 4 * sizeof(int32_t), st) != hipSuccess) return check_launch();
  instances_edge_ranges_kernel<<<(unsigned)((E + 1 + INST_THREADS - 1) / INST_THREADS), INST_THREADS, 0, st>>>(a);
  instances_scan_kernel<<<1, INST_THREADS, 0, st>>>(a);
  return check_launch();
}

extern "C" int isg_instances_fill(const int32_t *ptr, const int64_t *edge_index, const int32_t *index, int64_t N, int64_t E,
                                  int64_t G, int64_t Q, const int32_t *inst_ptr, const int32_t *inst_eptr, const void *workspace,
                                  size_t workspace_bytes, int64_t cap_nodes, int64_t cap_edges, int64_t *batch_out,
                                  int64_t *edge_index_out, int64_t *node_src, int64_t *edge_src, void *stream) {
  if (N < 0 || E < 0 || G < 0 || Q < 0 || cap_nodes < 0 || cap_edges < 0) return ISG_EINVAL;
  if (inst_too_large(N) || inst_too_large(E) || inst_too_large(G) || inst_too_large(Q) || inst_too_large(cap_nodes) ||
      inst_too_large(cap_edges))
    return ISG_EUNSUPPORTED;
  if (Q == 0) return ISG_OK;
  if (G == 0) return ISG_EINVAL;
  InstArgs a = {.ptr = ptr, .batch = nullptr, .edge_index = edge_index, .index = index, .N = (int)N, .E = (int)E, .G = (int)G,
                .Q = (int)Q, .inst_ptr = const_cast<int *>(inst_ptr), .inst_eptr = const_cast<int *>(inst_eptr), .status = nullptr,
                .eptr = (int *)const_cast<void *>(workspace), .cap_nodes = (int)cap_nodes, .cap_edges = (int)cap_edges,
                .batch_out = batch_out, .edge_index_out = edge_index_out, .node_src = node_src, .edge_src = edge_src};
  if (!a.ptr || !a.index || !a.inst_ptr || !a.inst_eptr || (a.cap_nodes > 0 && (!a.batch_out || !a.node_src)) ||
      (a.cap_edges > 0 && (!a.edge_index || !a.edge_index_out || !a.edge_src)))
    return ISG_EINVAL;
  if (!a.eptr || workspace_bytes < isg_instances_workspace_bytes(G)) return ISG_EWORKSPACE;
  if (a.cap_nodes == 0 && a.cap_edges == 0) return ISG_OK;
  instances_fill_kernel<<<(unsigned)((Q + INST_WAVES - 1) / INST_WAVES), INST_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}

extern "C" int isg_instance_rows(const float *x, int32_t ldx, int64_t x_rows, const int64_t *node_src, int64_t n_out, float *x_out,
                                 int32_t ldxo, int32_t Cx, const float *e, int32_t lde, int64_t e_rows, const int64_t *edge_src,
                                 int64_t m_out, float *e_out, int32_t ldeo, int32_t Ce, void *stream) {
  if (n_out < 0 || m_out < 0 || x_rows < 0 || e_rows < 0) return ISG_EINVAL;
  RowsArgs a = {.x = x, .ldx = ldx, .x_rows = x_rows, .node_src = node_src, .n_out = n_out, .x_out = x_out, .ldxo = ldxo,
                .Cx4 = Cx / 4, .e = e, .lde = lde, .e_rows = e_rows, .edge_src = edge_src, .m_out = m_out, .e_out = e_out,
                .ldeo = ldeo, .Ce4 = Ce / 4};
  if (a.n_out > 0 && (Cx < 1 || ldx < Cx || ldxo < Cx || !a.x || !a.node_src || !a.x_out)) return ISG_EINVAL;
  if (a.m_out > 0 && (Ce < 1 || lde < Ce || ldeo < Ce || !a.e || !a.edge_src || !a.e_out)) return ISG_EINVAL;
  if (inst_too_large(n_out) || inst_too_large(m_out)) return ISG_EUNSUPPORTED;
  if (a.n_out > 0 && (((Cx | ldx | ldxo) & 3) || ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.x_out)) & 15)))
    return ISG_EUNSUPPORTED;
  if (a.m_out > 0 && (((Ce | lde | ldeo) & 3) || ((reinterpret_cast<uintptr_t>(a.e) | reinterpret_cast<uintptr_t>(a.e_out)) & 15)))
    return ISG_EUNSUPPORTED;
  if (a.n_out == 0 && a.m_out == 0) return ISG_OK;
  const int64_t blocks = (n_out + m_out + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  instance_rows_kernel<<<(unsigned)blocks, INST_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
