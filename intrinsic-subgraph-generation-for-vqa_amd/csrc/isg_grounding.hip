// Grounding of the sampled subgraph in GQA's object annotations (include/isg_grounding.h): per question, how many of the objects
// its annotations refer to are among the kept nodes; per evaluation, running totals overall and per group of questions.
//
// Nothing here is compute-bound and nothing is on the timed path.  Launch 1 reads a graph's mask once and F * M <= 192 gold
// entries per question: lane j holds entry j of every facet, an entry is compared with the entries before it by reading the other
// lanes' registers (a uniform lane index: no LDS, no barrier), and ballots + popcounts turn the lanes' flags into the row of the
// table.  Launch 2 is the fold of isg_token_coo_groups: workgroup r walks the table for its own row of the totals, sums in
// registers and LDS (integer atomics, whose order cannot change an integer sum; the sums every question adds to are reduced over
// the wave first, so that only the histogram bins take an atomic per question) and adds the result with plain loads and stores.
// No atomic in global memory, no floating point beyond the comparison with the threshold.
#include "isg_common.hpp"
#include "../../include/isg_eval.h"
#include "../../include/isg_grounding.h"

#include <limits.h>

namespace isg {

constexpr int GR_ROWS = 4;            // questions (waves) per workgroup of the first launch
constexpr int GR_THREADS = 256;       // threads of the second launch
constexpr int GR_HEAD_SUMS = 4;       // written entries of a totals row's head
constexpr int GR_BLOCK_SUMS = 7;      // written entries in front of a block's histograms
constexpr int GR_SUMS = GR_HEAD_SUMS + 2 * ISG_GROUND_SETS * GR_BLOCK_SUMS;      // sums a thread keeps in registers; the histograms take LDS atomics
static_assert(ISG_GROUND_GOLD_MAX == ISG_WAVE && ISG_GROUND_FACETS + 1 == ISG_GROUND_SETS &&
              ISG_GROUND_COLS == ISG_GROUND_COL_SETS + 2 * ISG_GROUND_SETS &&
              ISG_GROUND_HIST == ISG_GROUND_FACETS * ISG_GROUND_GOLD_MAX + 1 && ISG_GROUND_BLOCK == 8 + 2 * ISG_GROUND_HIST &&
              ISG_GROUND_TOTALS == ISG_GROUND_HEAD + 2 * ISG_GROUND_SETS * ISG_GROUND_BLOCK,
              "header and kernel disagree");

struct GroundingArgs {
  const float *node_mask;    // fp32 [N]; may be NULL when N == 0
  float threshold;
  const int *ptr;            // int32 [B + 1]
  const int *gold;           // int32 [B, F, M]
  const int64_t *pred;       // int64 [B]; optional (NULL: no question counts as correct)
  const int64_t *label;      // int64 [B]; optional, given with pred
  const int *groups;         // int32 [B, Fg]; optional (NULL: G == 0)
  int *table;                // int32 [B, ISG_GROUND_COLS]
  int64_t *totals;           // int64 [1 + G, ISG_GROUND_TOTALS]; optional (NULL: the table only)
  int32_t *status;           // int32 [2]; optional
  int N, B, F, M, Fg, G;
};

__device__ __forceinline__ int popc64(unsigned long long b) { return __popcll(b); }

__global__ __launch_bounds__(ISG_WAVE * GR_ROWS) void grounding_rows_kernel(GroundingArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * GR_ROWS + (threadIdx.x >> 6);
  if (g >= a.B) return;                                  // the wave's: every lane of a wave that stays takes every ballot
  const int lo = min(max(a.ptr[g], 0), a.N), hi = min(max(a.ptr[g + 1], lo), a.N);
  const int n = hi - lo;
  int kept_nodes = 0;
  for (int base = lo; base < hi; base += ISG_WAVE) {     // lo, hi are the wave's
    const int i = base + lane;
    kept_nodes += popc64(__ballot(i < hi && a.node_mask[i] > a.threshold));      // a NaN compares false
  }
  int cols[ISG_GROUND_COLS];
#pragma unroll
  for (int c = 0; c < ISG_GROUND_COLS; ++c) cols[c] = 0;
  cols[ISG_GROUND_COL_KEPT] = kept_nodes;
  cols[ISG_GROUND_COL_NODES] = n;
  const int *row = a.gold + g * a.F * a.M;
  int val[ISG_GROUND_FACETS];                            // this lane's entry of every facet: a valid index, or -1
#pragma unroll
  for (int s = 0; s < ISG_GROUND_FACETS; ++s) {
    const int e = s < a.F && lane < a.M ? row[s * a.M + lane] : ISG_GROUND_PAD;
    const bool valid = e >= 0 && e < n;                  // checked against the graph before it becomes an address
    cols[ISG_GROUND_COL_UNRESOLVED] += popc64(__ballot(e == ISG_GROUND_UNRESOLVED));
    cols[ISG_GROUND_COL_BAD] += popc64(__ballot(!valid && e != ISG_GROUND_PAD && e != ISG_GROUND_UNRESOLVED));
    val[s] = valid ? e : -1;
  }
#pragma unroll
  for (int s = 0; s < ISG_GROUND_FACETS; ++s) {
    const int v = val[s];
    bool first = v >= 0;                                 // no earlier entry of this facet holds the index
    for (int j = 0; j < a.M; ++j) {                      // j is the wave's: every lane takes every read
      const int other = __shfl(val[s], j, ISG_WAVE);
      first = first & !(j < lane & other == v);
    }
    bool first_any = first;                              // ... and no entry of an earlier facet
#pragma unroll
    for (int t = 0; t < s; ++t)
      for (int j = 0; j < a.M; ++j) {
        const int other = __shfl(val[t], j, ISG_WAVE);
        first_any = first_any & (other != v);
      }
    bool hit = false;
    if (first) hit = a.node_mask[lo + v] > a.threshold;  // 0 <= v < n: lo + v < hi <= N
    const int size = popc64(__ballot(first)), hits = popc64(__ballot(hit));
    cols[ISG_GROUND_COL_SETS + 2 * s] = size;
    cols[ISG_GROUND_COL_SETS + 2 * s + 1] = hits;
    cols[ISG_GROUND_COL_SETS + 2 * ISG_GROUND_FACETS] += popc64(__ballot(first_any));
    cols[ISG_GROUND_COL_SETS + 2 * ISG_GROUND_FACETS + 1] += popc64(__ballot(first_any && hit));
  }
  int out = 0;
#pragma unroll
  for (int c = 0; c < ISG_GROUND_COLS; ++c) out = lane == c ? cols[c] : out;
  if (lane < ISG_GROUND_COLS) a.table[g * ISG_GROUND_COLS + lane] = out;
}

// workgroup r adds the questions of row r of the totals: every question (r == 0), or those of group r - 1, each as often as its
// facets name the group (the rule of isg_token_coo_groups)
__global__ __launch_bounds__(GR_THREADS) void grounding_totals_kernel(GroundingArgs a) {
  __shared__ unsigned long long s_tot[ISG_GROUND_TOTALS];
  __shared__ int s_bad, s_first;
  const int tid = threadIdx.x, r = blockIdx.x;
  for (int i = tid; i < ISG_GROUND_TOTALS; i += GR_THREADS) s_tot[i] = 0ull;
  if (tid == 0) { s_bad = 0; s_first = INT_MAX; }
  __syncthreads();
  long long acc[GR_SUMS];                                // this thread's share of the head and of every block's seven sums
#pragma unroll
  for (int j = 0; j < GR_SUMS; ++j) acc[j] = 0;
  for (int g = tid; g < a.B; g += GR_THREADS) {
    int times = r == 0 ? 1 : 0;
    if (a.groups) {
      for (int f = 0; f < a.Fg; ++f) {
        const int id = a.groups[(int64_t)g * a.Fg + f];
        if (r > 0) times += id == r - 1 ? 1 : 0;
        else if (id < -1 || id >= a.G) {                 // workgroup 0 sees every id once: it keeps the status
          atomicAdd(&s_bad, 1);
          atomicMin(&s_first, g);
        }
      }
    }
    if (times == 0) continue;
    const long long t = times;
    const int *row = a.table + (int64_t)g * ISG_GROUND_COLS;
    const bool correct = a.pred && a.pred[g] == a.label[g];
    acc[0] += t;
    acc[1] += correct ? t : 0;
    acc[2] += t * row[ISG_GROUND_COL_UNRESOLVED];
    acc[3] += t * row[ISG_GROUND_COL_BAD];
    const long long kept = row[ISG_GROUND_COL_KEPT], nodes = row[ISG_GROUND_COL_NODES];
#pragma unroll
    for (int s = 0; s < ISG_GROUND_SETS; ++s) {
      const int size = row[ISG_GROUND_COL_SETS + 2 * s], hits = row[ISG_GROUND_COL_SETS + 2 * s + 1];
      if (size <= 0) continue;
      const int m = min(size, ISG_GROUND_HIST - 1);       // what launch 1 wrote never exceeds it
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (c == 1 && !correct) continue;
        long long *sum = acc + GR_HEAD_SUMS + (2 * s + c) * GR_BLOCK_SUMS;       // static indices: registers
        sum[0] += t;
        sum[1] += t * kept;
        sum[2] += t * nodes;
        sum[3] += t * size;
        sum[4] += t * hits;
        sum[5] += hits > 0 ? t : 0;
        sum[6] += hits == size ? t : 0;
        unsigned long long *hist = s_tot + ISG_GROUND_HEAD + (2 * s + c) * ISG_GROUND_BLOCK + 8;      // LDS
        atomicAdd(&hist[m], (unsigned long long)t);
        atomicAdd(&hist[ISG_GROUND_HIST + m], (unsigned long long)(t * hits));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < GR_SUMS; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
    const int slot = j < GR_HEAD_SUMS ? j : ISG_GROUND_HEAD + ((j - GR_HEAD_SUMS) / GR_BLOCK_SUMS) * ISG_GROUND_BLOCK + (j - GR_HEAD_SUMS) % GR_BLOCK_SUMS;
    if ((tid & 63) == 0) atomicAdd(&s_tot[slot], (unsigned long long)acc[j]);
  }
  __syncthreads();
  int64_t *out = a.totals + (size_t)r * ISG_GROUND_TOTALS;
  for (int i = tid; i < ISG_GROUND_TOTALS; i += GR_THREADS) {
    const bool reserved = i < ISG_GROUND_HEAD ? i >= 4 : (i - ISG_GROUND_HEAD) % ISG_GROUND_BLOCK == 7;
    if (!reserved) out[i] += (int64_t)s_tot[i];
  }
  if (r == 0 && tid == 0 && a.status && s_bad > 0) {
    const int seen = a.status[0];
    if (seen == 0) a.status[1] = s_first;
    a.status[0] = (int)min((long long)INT_MAX, (long long)seen + s_bad);
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_grounding_abi_version(void) { return ISG_GROUNDING_ABI_VERSION; }

extern "C" int isg_grounding(const float *node_mask, float threshold, const int32_t *ptr, const int32_t *gold, int32_t F, int32_t M,
                             const int64_t *pred, const int64_t *label, const int32_t *groups, int32_t Fg, int32_t G, int32_t *table,
                             int64_t *totals, int32_t *status, int64_t N, int64_t B, void *stream) {
  if (N < 0 || B < 0 || F < 1 || F > ISG_GROUND_FACETS || M < 1 || M > ISG_GROUND_GOLD_MAX || (pred == nullptr) != (label == nullptr))
    return ISG_EINVAL;
  if (groups && (G < 1 || G > ISG_EVAL_GROUPS_MAX || Fg < 1 || Fg > ISG_EVAL_FACETS_MAX)) return ISG_EINVAL;
  const int64_t lim = (1ll << 31) - 1;
  if (N >= lim || B >= lim) return ISG_EUNSUPPORTED;
  GroundingArgs a = {.node_mask = node_mask, .threshold = threshold, .ptr = ptr, .gold = gold, .pred = pred, .label = label,
                     .groups = groups, .table = table, .totals = totals, .status = status,
                     .N = (int)N, .B = (int)B, .F = F, .M = M, .Fg = groups ? Fg : 0, .G = groups ? G : 0};
  if (a.B > 0 && (!a.ptr || !a.gold || !a.table || (a.N > 0 && !a.node_mask))) return ISG_EINVAL;
  if (a.B == 0) return ISG_OK;
  hipStream_t st = as_stream(stream);
  grounding_rows_kernel<<<(unsigned)((a.B + GR_ROWS - 1) / GR_ROWS), ISG_WAVE * GR_ROWS, 0, st>>>(a);
  if (a.totals) grounding_totals_kernel<<<1 + a.G, GR_THREADS, 0, st>>>(a);
  return check_launch();
}
