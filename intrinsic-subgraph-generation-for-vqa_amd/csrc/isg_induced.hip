// Induced-subgraph instances (include/ext/isg_induced.h): G distinct graphs, an index over Q instances and a row of keep bits per
// instance become the batch of Q graphs in which instance q is graph index[q] minus the nodes its bits leave out -- maps and
// renumbered index tensors only, as in isg_instances.hip; the rows follow through node_src / edge_src.
//
// All integer and exact.  Size pass: (1) one thread per edge position stores the per-graph edge ranges (the kernel of
// isg_instances.hip, repeated here so that no existing entry point moves); (2) one wave per instance counts its kept nodes and
// kept edges; (3) ONE workgroup scans the Q counts in blocks of IND_SCAN_BLOCK.  Fill pass: one wave per instance does the walk of
// (2) again and writes.  A wave holds its row of keep one word per lane; the rank of a node is the popcounts of the words below
// plus that of the bits below (a shuffle each); the edge range is walked 64 at a time with a ballot per chunk and a running base.
// Every loop bound is uniform over the wave, so every lane takes part in every shuffle and ballot.  No atomics: an output word has
// one writer, a flag takes a plain store of 1.  Every number read from memory that becomes an address or a lane number is clamped
// or compared first, by the same rule in both passes, so a bad ptr, batch, edge_index, index or keep gives wrong rows and never a
// fault.
#include "isg_common.hpp"

#include "../../include/ext/isg_induced.h"

namespace isg {

constexpr int IND_THREADS = 256, IND_PER = 4, IND_SCAN_BLOCK = IND_THREADS * IND_PER;   // instances one scan step takes
constexpr int IND_WAVES = IND_THREADS / ISG_WAVE;
constexpr int IND_WORDS_MAX = ISG_WAVE;                                                 // one word of keep per lane
constexpr long long IND_I32_MAX = 2147483647ll;

struct IndArgs {
  const int *ptr;                // int32 [G + 1]
  const int64_t *batch;          // int64 [N]; NULL in the fill pass, may be NULL when E == 0
  const int64_t *edge_index;     // int64 [2, E]; may be NULL when E == 0
  const int *index;              // int32 [Q]
  const uint32_t *keep;          // uint32 [Q, W]; NULL: every node is kept
  int W;
  int N, E, G, Q;
  int *inst_ptr, *inst_eptr;     // int32 [Q + 1]
  int *status;                   // int32 [4] = {N', E', bad_index, bad_grouping}; NULL in the fill pass
  int *eptr;                     // workspace int32 [G + 1]: edge range of every graph
  int *cnt;                      // workspace int32 [2, Q]: kept nodes, kept edges of every instance; NULL in the fill pass
  int cap_nodes, cap_edges;      // fill pass only
  int64_t *batch_out, *edge_index_out, *node_src, *edge_src;   // NULL in the size pass; may be NULL where the capacity is 0
};

__device__ __forceinline__ void ind_node_range(const IndArgs &a, int g, int &lo, int &hi) {
  lo = max(0, min(a.ptr[g], a.N));
  hi = max(lo, min(a.ptr[g + 1], a.N));
}
__device__ __forceinline__ void ind_edge_range(const IndArgs &a, int g, int &lo, int &hi) {
  lo = max(0, min(a.eptr[g], a.E));
  hi = max(lo, min(a.eptr[g + 1], a.E));
}

// graph of edge e in [0, G); `bad`: an end or its graph id is out of range, or the two ends disagree (the edge then counts as the
// last graph's, which keeps every range inside the list)
__device__ __forceinline__ int ind_edge_graph(const IndArgs &a, int e, bool &bad) {
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
__global__ __launch_bounds__(IND_THREADS) void induced_edge_ranges_kernel(IndArgs a) {
  const long long e = (long long)blockIdx.x * IND_THREADS + threadIdx.x;
  if (e > a.E) return;
  bool bad = false;
  const int before = e == 0 ? -1 : ind_edge_graph(a, (int)e - 1, bad);
  bool bad_here = false;
  const int at = e == a.E ? a.G : ind_edge_graph(a, (int)e, bad_here);
  for (int g = before + 1; g <= at; ++g) a.eptr[g] = (int)e;
  if (bad_here || at < before) a.status[3] = 1;       // (`bad` belongs to thread e - 1)
}

// The kept nodes of one instance as its wave holds them: `word` = this lane's 32 bits (bits beyond the graph already cleared),
// `below` = kept nodes in the words of the lanes below, `n` = local nodes that can be kept at all (min(n_g, 32 W)).
struct IndRow {
  uint32_t word;
  int below, n, kept;
  bool all;                      // keep == NULL: node i is kept and its rank is i
};

__device__ __forceinline__ IndRow ind_row(const IndArgs &a, long long q, int n_g, int lane) {
  IndRow r = {.word = 0u, .below = 0, .n = n_g, .kept = n_g, .all = a.keep == nullptr};
  if (r.all) return r;
  r.n = min(n_g, 32 * a.W);
  const int bits = min(max(r.n - 32 * lane, 0), 32);                     // bits of this lane's word that name a node
  if (bits > 0) r.word = a.keep[q * a.W + lane] & (bits >= 32 ? 0xffffffffu : (1u << bits) - 1u);      // (bits > 0: lane < W)
  int incl = __popc(r.word);
#pragma unroll
  for (int off = 1; off < ISG_WAVE; off <<= 1) {
    const int o = __shfl_up(incl, off, ISG_WAVE);
    if (lane >= off) incl += o;
  }
  r.below = incl - __popc(r.word);
  r.kept = __shfl(incl, ISG_WAVE - 1, ISG_WAVE);
  return r;
}

// local node i of the instance (any int; every lane of the wave calls this): is it kept, and its rank if it is
__device__ __forceinline__ bool ind_lookup(const IndRow &r, long long i, int &rank) {
  const bool inside = i >= 0 && i < r.n;
  const int ii = inside ? (int)i : 0;
  if (r.all) {
    rank = ii;
    return inside;
  }
  const int src = min(ii >> 5, ISG_WAVE - 1);                            // (r.n <= 32 * 64: already below 64)
  const uint32_t w = (uint32_t)__shfl((int)r.word, src, ISG_WAVE);
  const int below = __shfl(r.below, src, ISG_WAVE);
  rank = below + __popc(w & ((1u << (ii & 31)) - 1u));
  return inside && ((w >> (ii & 31)) & 1u);
}

// One wave walks instance q.  FILL false: the counts into a.cnt; FILL true: the outputs, nothing at or beyond a capacity.
template <bool FILL>
__global__ __launch_bounds__(IND_THREADS) void induced_walk_kernel(IndArgs a) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * IND_WAVES + (threadIdx.x >> 6);
  if (q >= a.Q) return;                                          // (uniform over the wave, as every branch and bound below)
  const int g = a.index[q];
  if (g < 0 || g >= a.G) {                                       // an empty instance; the scan sets the flag
    if (!FILL && lane == 0) a.cnt[q] = a.cnt[(long long)a.Q + q] = 0;
    return;
  }
  int nlo, nhi, elo, ehi;
  ind_node_range(a, g, nlo, nhi);
  ind_edge_range(a, g, elo, ehi);
  if (FILL && a.cap_edges == 0) ehi = elo;                       // no edge is written: edge_index may be missing
  const IndRow row = ind_row(a, q, nhi - nlo, lane);
  const long long n0 = FILL ? a.inst_ptr[q] : 0, e0 = FILL ? a.inst_eptr[q] : 0;
  if (FILL) {
    for (int base = 0; base < row.n; base += ISG_WAVE) {
      const int i = base + lane;
      int r;
      const bool kept = ind_lookup(row, i, r);
      const long long o = n0 + r;
      if (kept && o >= 0 && o < a.cap_nodes) {
        a.batch_out[o] = q;
        a.node_src[o] = nlo + i;
      }
    }
  }
  long long ebase = 0;                                           // kept edges of the chunks before this one
  for (int c = elo; c < ehi; c += ISG_WAVE) {
    const int e = c + lane;
    long long ls = -1, ld = -1;
    if (e < ehi) {
      ls = a.edge_index[e] - nlo;
      ld = a.edge_index[(int64_t)a.E + e] - nlo;
    }
    int rs, rd;
    const bool ks = ind_lookup(row, ls, rs), kd = ind_lookup(row, ld, rd);
    const bool kept = ks && kd;
    const unsigned long long m = __ballot(kept);
    if (FILL) {
      const long long o = e0 + ebase + __popcll(m & ((1ull << lane) - 1ull));
      if (kept && o >= 0 && o < a.cap_edges) {
        a.edge_src[o] = e;
        a.edge_index_out[o] = n0 + rs;
        a.edge_index_out[(int64_t)a.cap_edges + o] = n0 + rd;
      }
    }
    ebase += __popcll(m);
  }
  if (!FILL && lane == 0) {
    a.cnt[q] = row.kept;
    a.cnt[(long long)a.Q + q] = (int)ebase;
  }
}

__device__ __forceinline__ long long ind_wave_scan(long long v, int lane) {      // inclusive
#pragma unroll
  for (int off = 1; off < ISG_WAVE; off <<= 1) {
    const long long o = __shfl_up(v, off, ISG_WAVE);
    if (lane >= off) v += o;
  }
  return v;
}
__device__ __forceinline__ int ind_sat(long long v) { return (int)(v < IND_I32_MAX ? v : IND_I32_MAX); }

__global__ __launch_bounds__(IND_THREADS) void induced_scan_kernel(IndArgs a) {
  __shared__ long long s_n[IND_WAVES], s_e[IND_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry_n = 0, carry_e = 0;
  bool bad = false;
  for (int base = 0; base < a.Q; base += IND_SCAN_BLOCK) {      // (Q < 2^31 - IND_SCAN_BLOCK: checked on the host)
    int cn[IND_PER], ce[IND_PER];
    long long tn = 0, te = 0;
#pragma unroll
    for (int u = 0; u < IND_PER; ++u) {
      const int q = base + tid * IND_PER + u;
      cn[u] = ce[u] = 0;
      if (q < a.Q) {
        const int g = a.index[q];
        if (g < 0 || g >= a.G) {
          bad = true;
        } else {
          cn[u] = max(a.cnt[q], 0);
          ce[u] = max(a.cnt[(long long)a.Q + q], 0);
        }
      }
      tn += cn[u];
      te += ce[u];
    }
    const long long in_n = ind_wave_scan(tn, lane), in_e = ind_wave_scan(te, lane);
    if (lane == ISG_WAVE - 1) {
      s_n[wave] = in_n;
      s_e[wave] = in_e;
    }
    __syncthreads();
    long long before_n = carry_n + in_n - tn, before_e = carry_e + in_e - te;
#pragma unroll
    for (int w = 0; w < IND_WAVES; ++w) {
      if (w < wave) {
        before_n += s_n[w];
        before_e += s_e[w];
      }
      carry_n += s_n[w];
      carry_e += s_e[w];
    }
#pragma unroll
    for (int u = 0; u < IND_PER; ++u) {
      const int q = base + tid * IND_PER + u;
      if (q < a.Q) {
        a.inst_ptr[q] = ind_sat(before_n);
        a.inst_eptr[q] = ind_sat(before_e);
      }
      before_n += cn[u];
      before_e += ce[u];
    }
    __syncthreads();                                            // s_n / s_e are rewritten by the next block
  }
  if (tid == 0) {
    a.inst_ptr[a.Q] = a.status[0] = ind_sat(carry_n);
    a.inst_eptr[a.Q] = a.status[1] = ind_sat(carry_e);
  }
  if (bad) a.status[2] = 1;
}

}  // namespace isg

using namespace isg;

extern "C" int isg_induced_abi_version(void) { return ISG_INDUCED_ABI_VERSION; }

extern "C" size_t isg_induced_workspace_bytes(int64_t G, int64_t Q) {
  return G < 0 || Q < 0 ? 0 : (size_t)(G + 1 + 2 * Q) * sizeof(int32_t);
}

static inline bool ind_too_large(int64_t v) { return v >= (1ll << 31) - IND_SCAN_BLOCK; }

extern "C" int isg_induced_size(const int32_t *ptr, const int64_t *batch, const int64_t *edge_index, const int32_t *index,
                                const uint32_t *keep, int64_t W, int64_t N, int64_t E, int64_t G, int64_t Q, int32_t *inst_ptr,
                                int32_t *inst_eptr, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  if (N < 0 || E < 0 || G < 0 || Q < 0 || (keep && W < 1)) return ISG_EINVAL;
  if (ind_too_large(N) || ind_too_large(E) || ind_too_large(G) || ind_too_large(Q) || (keep && W > IND_WORDS_MAX))
    return ISG_EUNSUPPORTED;
  if (Q == 0) return ISG_OK;
  if (G == 0) return ISG_EINVAL;
  int *ws = (int *)workspace;
  IndArgs a = {.ptr = ptr, .batch = batch, .edge_index = edge_index, .index = index, .keep = keep, .W = keep ? (int)W : 0,
               .N = (int)N, .E = (int)E, .G = (int)G, .Q = (int)Q, .inst_ptr = inst_ptr, .inst_eptr = inst_eptr, .status = status,
               .eptr = ws, .cnt = ws ? ws + (G + 1) : nullptr, .cap_nodes = 0, .cap_edges = 0, .batch_out = nullptr,
               .edge_index_out = nullptr, .node_src = nullptr, .edge_src = nullptr};
  if (!a.ptr || !a.index || !a.inst_ptr || !a.inst_eptr || !a.status || (a.E > 0 && (!a.batch || !a.edge_index))) return ISG_EINVAL;
  if (!a.eptr || !a.cnt || workspace_bytes < isg_induced_workspace_bytes(G, Q)) return ISG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(a.status, 0, 4 * sizeof(int32_t), st) != hipSuccess) return check_launch();
  induced_edge_ranges_kernel<<<(unsigned)((E + 1 + IND_THREADS - 1) / IND_THREADS), IND_THREADS, 0, st>>>(a);
  induced_walk_kernel<false><<<(unsigned)((Q + IND_WAVES - 1) / IND_WAVES), IND_THREADS, 0, st>>>(a);
  induced_scan_kernel<<<1, IND_THREADS, 0, st>>>(a);
  return check_launch();
}

extern "C" int isg_induced_fill(const int32_t *ptr, const int64_t *edge_index, const int32_t *index, const uint32_t *keep,
                                int64_t W, int64_t N, int64_t E, int64_t G, int64_t Q, const int32_t *inst_ptr,
                                const int32_t *inst_eptr, const void *workspace, size_t workspace_bytes, int64_t cap_nodes,
                                int64_t cap_edges, int64_t *batch_out, int64_t *edge_index_out, int64_t *node_src,
                                int64_t *edge_src, void *stream) {
  if (N < 0 || E < 0 || G < 0 || Q < 0 || cap_nodes < 0 || cap_edges < 0 || (keep && W < 1)) return ISG_EINVAL;
  if (ind_too_large(N) || ind_too_large(E) || ind_too_large(G) || ind_too_large(Q) || ind_too_large(cap_nodes) ||
      ind_too_large(cap_edges) || (keep && W > IND_WORDS_MAX))
    return ISG_EUNSUPPORTED;
  if (Q == 0) return ISG_OK;
  if (G == 0) return ISG_EINVAL;
  IndArgs a = {.ptr = ptr, .batch = nullptr, .edge_index = edge_index, .index = index, .keep = keep, .W = keep ? (int)W : 0,
               .N = (int)N, .E = (int)E, .G = (int)G, .Q = (int)Q, .inst_ptr = const_cast<int *>(inst_ptr),
               .inst_eptr = const_cast<int *>(inst_eptr), .status = nullptr, .eptr = (int *)const_cast<void *>(workspace),
               .cnt = nullptr, .cap_nodes = (int)cap_nodes, .cap_edges = (int)cap_edges, .batch_out = batch_out,
               .edge_index_out = edge_index_out, .node_src = node_src, .edge_src = edge_src};
  if (!a.ptr || !a.index || !a.inst_ptr || !a.inst_eptr || (a.cap_nodes > 0 && (!a.batch_out || !a.node_src)) ||
      (a.cap_edges > 0 && (!a.edge_index || !a.edge_index_out || !a.edge_src)))
    return ISG_EINVAL;
  if (!a.eptr || workspace_bytes < isg_induced_workspace_bytes(G, Q)) return ISG_EWORKSPACE;
  if (a.cap_nodes == 0 && a.cap_edges == 0) return ISG_OK;
  induced_walk_kernel<true><<<(unsigned)((Q + IND_WAVES - 1) / IND_WAVES), IND_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
