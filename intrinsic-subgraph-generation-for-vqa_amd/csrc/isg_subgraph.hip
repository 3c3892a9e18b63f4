// Induced-subgraph cut: the nodes a mask keeps, the edges among them, and everything renumbered -- on the device, in three launches.
//
// All integer and exact.  Launch 1 counts the kept nodes / kept edges of every block of SG_BLOCK consecutive elements.  Launch 2:
// every workgroup adds up the counts of the blocks before its own (they are final: the kernel boundary is the only hand-off between
// workgroups), ranks its own elements with wave ballots + popcounts and scatters the ids.  Launch 3 needs every node's rank: the
// kept edges' endpoints in the new numbering, the per-graph node ranges, the per-graph table of kept nodes, the two counts.
// The grid depends on N, E, B and table_k alone -- never on the device -- and nothing is accumulated atomically, so the outputs are a
// function of the inputs.
#include "isg_common.hpp"

#include <algorithm>

namespace isg {

constexpr int SG_THREADS = 256, SG_PER = 4, SG_BLOCK = SG_THREADS * SG_PER;      // elements one workgroup ranks
constexpr int SG_CHUNKS = SG_BLOCK / ISG_WAVE;                                   // ballots per workgroup

struct SubgraphArgs {
  const float *node_mask;        // fp32 [N]; may be NULL when N == 0
  float threshold;
  int complement;
  const int64_t *edge_index;     // int64 [2, E]; may be NULL when E == 0
  const int64_t *batch;          // int64 [N]; may be NULL when N == 0
  const int *ptr;                // int32 [B + 1]
  int N, E, B;
  int *node_new, *edge_new;      // int32 [N] / [E]: new id or -1
  int64_t *node_id, *edge_id;    // int64 [N] / [E]: kept ids, ascending
  int64_t *edge_index_out;       // int64 [2, E], row stride E
  int64_t *batch_out;            // int64 [N]
  int *ptr_out;                  // int32 [B + 1]
  int *sel;                      // int32 [B, table_k]; may be NULL when table_k == 0
  int table_k;
  int *counts;                   // int32 [2] = {N', E'}
  int *block_counts;             // workspace: kept elements per block, node blocks first, then edge blocks
  int *excl;                     // workspace int32 [N + 1]: kept nodes before n
  int *etotal;                   // workspace int32 [1]: E'
  int nbn, nbe;                  // node blocks, edge blocks
};

__device__ __forceinline__ bool sg_keep_node(const SubgraphArgs &a, int n) {
  return (a.node_mask[n] > a.threshold) != (a.complement != 0);      // a NaN compares false
}
// element i of block `blk` (blk < nbn: node i, else edge i) is kept
__device__ __forceinline__ bool sg_keep(const SubgraphArgs &a, bool nodes, int i) {
  if (nodes) return i < a.N && sg_keep_node(a, i);
  if (i >= a.E) return false;
  const int64_t s = a.edge_index[i], d = a.edge_index[(int64_t)a.E + i];
  if (s < 0 || s >= a.N || d < 0 || d >= a.N) return false;
  return sg_keep_node(a, (int)s) && sg_keep_node(a, (int)d);
}

__global__ __launch_bounds__(SG_THREADS) void subgraph_count_kernel(SubgraphArgs a) {
  __shared__ int s_cnt[SG_CHUNKS];
  const int tid = threadIdx.x, blk = blockIdx.x;
  const bool nodes = blk < a.nbn;
  const int base = (nodes ? blk : blk - a.nbn) * SG_BLOCK;
#pragma unroll
  for (int u = 0; u < SG_PER; ++u) {
    const unsigned long long m = __ballot(sg_keep(a, nodes, base + u * SG_THREADS + tid));
    if ((tid & 63) == 0) s_cnt[u * (SG_THREADS / ISG_WAVE) + (tid >> 6)] = __popcll(m);
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int c = 0; c < SG_CHUNKS; ++c) t += s_cnt[c];
    a.block_counts[blk] = t;
  }
}

__global__ __launch_bounds__(SG_THREADS) void subgraph_rank_kernel(SubgraphArgs a) {
  __shared__ int s_cnt[SG_CHUNKS];
  __shared__ int s_part[SG_THREADS / ISG_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  const bool nodes = blk < a.nbn;
  const int first = nodes ? 0 : a.nbn, local = blk - first;
  // kept elements of the blocks before this one
  int part = 0;
  for (int c = tid; c < local; c += SG_THREADS) part += a.block_counts[first + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if (lane == 0) s_part[wave] = part;
  const int base = local * SG_BLOCK;
  bool keep[SG_PER];
  unsigned long long m[SG_PER];
#pragma unroll
  for (int u = 0; u < SG_PER; ++u) {
    keep[u] = sg_keep(a, nodes, base + u * SG_THREADS + tid);
    m[u] = __ballot(keep[u]);
    if (lane == 0) s_cnt[u * (SG_THREADS / ISG_WAVE) + wave] = __popcll(m[u]);
  }
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int w = 0; w < SG_THREADS / ISG_WAVE; ++w) before += s_part[w];
  const int n_el = nodes ? a.N : a.E;
  int run = before;
#pragma unroll
  for (int u = 0; u < SG_PER; ++u) {
    int chunk = run;                         // kept elements before this wave's 64 of round u
    for (int w = 0; w < SG_THREADS / ISG_WAVE; ++w) {
      const int c = s_cnt[u * (SG_THREADS / ISG_WAVE) + w];
      if (w < wave) chunk += c;
      run += c;
    }
    const int i = base + u * SG_THREADS + tid;
    if (i >= n_el) continue;
    const int r = chunk + __popcll(m[u] & ((1ull << lane) - 1ull));
    if (nodes) {
      a.excl[i] = r;
      a.node_new[i] = keep[u] ? r : -1;
      if (keep[u]) {
        a.node_id[r] = i;
        a.batch_out[r] = a.batch[i];
      }
    } else {
      a.edge_new[i] = keep[u] ? r : -1;
      if (keep[u]) a.edge_id[r] = i;
    }
  }
  if (tid == 0) {                            // run = kept elements up to and including this block
    if (nodes && blk == a.nbn - 1) a.excl[a.N] = run;
    if (!nodes && local == a.nbe - 1) a.etotal[0] = run;
  }
}

__device__ __forceinline__ int sg_excl_at(const SubgraphArgs &a, int p) {      // kept nodes before position p of the node list
  return a.N > 0 ? a.excl[min(max(p, 0), a.N)] : 0;
}

__global__ __launch_bounds__(SG_THREADS) void subgraph_finish_kernel(SubgraphArgs a) {
  const long long i = (long long)blockIdx.x * SG_THREADS + threadIdx.x;
  if (i == 0) {
    a.counts[0] = sg_excl_at(a, a.N);
    a.counts[1] = a.E > 0 ? a.etotal[0] : 0;
  }
  if (i <= a.B) a.ptr_out[i] = sg_excl_at(a, a.ptr[i]);
  if (i < a.E) {
    const int r = a.edge_new[i];
    if (r >= 0) {                            // both endpoints are in range and kept
      a.edge_index_out[r] = a.node_new[a.edge_index[i]];
      a.edge_index_out[(int64_t)a.E + r] = a.node_new[a.edge_index[(int64_t)a.E + i]];
    }
  }
  if (a.table_k > 0) {
    if (i < a.N && a.node_new[i] >= 0) {     // a kept node: its place among its graph's kept nodes
      const int64_t g = a.batch[i];
      if (g >= 0 && g < a.B) {
        const int lo = a.ptr[g], hi = a.ptr[g + 1];
        if (lo >= 0 && lo <= i && i < hi) {
          const int j = a.node_new[i] - a.excl[lo];
          if (j >= 0 && j < a.table_k) a.sel[g * a.table_k + j] = (int)i - lo;
        }
      }
    }
    if (i < (long long)a.B * a.table_k) {    // the slots behind a graph's kept nodes
      const int g = (int)(i / a.table_k), j = (int)(i % a.table_k);
      const int kept = sg_excl_at(a, a.ptr[g + 1]) - sg_excl_at(a, a.ptr[g]);
      if (j >= kept) a.sel[i] = -1;
    }
  }
}

}  // namespace isg

using namespace isg;

static inline int64_t sg_blocks(int64_t n) { return (n + SG_BLOCK - 1) / SG_BLOCK; }

extern "C" size_t isg_subgraph_workspace_bytes(int64_t N, int64_t E) {
  if (N < 0 || E < 0) return 0;
  return (size_t)(sg_blocks(N) + sg_blocks(E) + (N + 1) + 1) * sizeof(int32_t);
}

extern "C" int isg_subgraph_cut(const float *node_mask, float threshold, int32_t complement, const int64_t *edge_index,
                                const int64_t *batch, const int32_t *ptr, int64_t N, int64_t E, int64_t B, int32_t *node_new,
                                int32_t *edge_new, int64_t *node_id, int64_t *edge_id, int64_t *edge_index_out, int64_t *batch_out,
                                int32_t *ptr_out, int32_t *sel, int32_t table_k, int32_t *counts, void *workspace,
                                size_t workspace_bytes, void *stream) {
  if (N < 0 || E < 0 || B < 0 || table_k < 0) return ISG_EINVAL;
  const int64_t lim = (1ll << 31) - SG_BLOCK;
  if (N >= lim || E >= lim || B >= lim || B * (int64_t)table_k >= lim) return ISG_EUNSUPPORTED;
  const int nbn = (int)sg_blocks(N), nbe = (int)sg_blocks(E);
  int *ws = (int *)workspace;
  SubgraphArgs a = {.node_mask = node_mask, .threshold = threshold, .complement = complement, .edge_index = edge_index,
                    .batch = batch, .ptr = ptr, .N = (int)N, .E = (int)E, .B = (int)B, .node_new = node_new, .edge_new = edge_new,
                    .node_id = node_id, .edge_id = edge_id, .edge_index_out = edge_index_out, .batch_out = batch_out,
                    .ptr_out = ptr_out, .sel = sel, .table_k = table_k, .counts = counts, .block_counts = ws,
                    .excl = ws ? ws + nbn + nbe : nullptr, .etotal = ws ? ws + nbn + nbe + (N + 1) : nullptr, .nbn = nbn, .nbe = nbe};
  if (!a.ptr || !a.node_new || !a.edge_new || !a.node_id || !a.edge_id || !a.edge_index_out || !a.batch_out || !a.ptr_out ||
      !a.counts || (a.N > 0 && (!a.node_mask || !a.batch)) || (a.E > 0 && !a.edge_index) || (a.table_k > 0 && !a.sel))
    return ISG_EINVAL;
  if (!a.block_counts || !a.excl || !a.etotal || workspace_bytes < isg_subgraph_workspace_bytes(N, E)) return ISG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  if (nbn + nbe > 0) {
    subgraph_count_kernel<<<nbn + nbe, SG_THREADS, 0, st>>>(a);
    subgraph_rank_kernel<<<nbn + nbe, SG_THREADS, 0, st>>>(a);
  }
  const int64_t span = std::max<int64_t>(std::max<int64_t>(N, E), std::max<int64_t>(B + 1, B * (int64_t)table_k));
  subgraph_finish_kernel<<<(unsigned)((span + SG_THREADS - 1) / SG_THREADS), SG_THREADS, 0, st>>>(a);
  return check_launch();
}
