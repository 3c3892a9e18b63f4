// Evaluation by question type (include/isg_eval.h): the rank of the true answer with the K best classes of a row, running meters
// per group of questions, and the token co-occurrence totals per group.
//
// Nothing here is compute-bound.  The rank kernel reads [B, 1842] logits (30 MB at B = 4096) a wave per row, as the cross-entropy
// does: one pass counts the classes that beat the label; the K selection rounds read the 7 KB row again from the cache.  The two
// grouped kernels read a few words per row.  No atomic in global memory, no floating-point atomic anywhere: a double sum runs
// over the rows of a workgroup ascending, then over the workgroups ascending in ONE finishing workgroup; the integer tables of the
// co-occurrence totals take integer LDS atomics, whose order cannot change an integer sum.
#include "isg_common.hpp"
#include "../../include/isg_eval.h"

#include <limits.h>
#include <math.h>

namespace isg {

constexpr int RANK_ROWS = 4;          // rows (waves) per workgroup of the rank kernel
constexpr int GM_THREADS = 256;       // threads of the grouped kernels: one per group of the partial table (G <= 256)
constexpr int GM_ROWS = 64;           // rows one workgroup of isg_group_meters' first launch takes: thread g walks them one by one
constexpr int GM_USED = 5;            // slots of a group that are written (ISG_GRP_ROWS .. ISG_GRP_HITSK)
constexpr int GM_TAIL = 2 + GM_USED;  // behind a partial table: the bad ids the workgroup saw, its first bad row (or -1), then the
                                      // five sums over ALL counted rows of the workgroup, whatever their groups
constexpr int COOG_HIST = ISG_COO_TOKENS_MAX + 1;
constexpr int COOG_SUMS = 12;         // totals[0 .. 12) of isg_token_coo; [12, 16) reserved
static_assert(ISG_EVAL_GROUPS_MAX <= GM_THREADS && GM_ROWS <= GM_THREADS && ISG_GRP_SLOTS >= GM_USED && ISG_COO_TOTALS == 16 + 4 * COOG_HIST,
              "header and kernel disagree");

// ---- rank and the K best classes ------------------------------------------------------------------------------------------------
struct RankArgs {
  const float *logits;       // [B, A], row stride ld, rows 4-byte aligned
  const int64_t *labels;     // [B]
  const double *row_lse;     // [B]; may be NULL without top_prob
  int32_t *rank;             // [B]
  int64_t *top_ids;          // [B, K]; optional
  float *top_prob;           // [B, K]; optional
  int64_t ignore_index;
  int B, A, ld, K;           // K = 0 when neither top_ids nor top_prob is given
};

__global__ __launch_bounds__(64 * RANK_ROWS) void answer_rank_kernel(RankArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * RANK_ROWS + (threadIdx.x >> 6);
  if (row >= a.B) return;                               // the wave's: every lane of a wave that stays takes every shuffle
  const float *x = a.logits + (size_t)row * a.ld;
  const int64_t lab = a.labels[row];
  const bool valid = lab >= 0 && lab < a.A;
  const int l = valid ? (int)lab : 0;
  const float xl = x[l];                                // a NaN here makes the row a NaN row below
  int beat = 0;
  bool nan = false;
  for (int j = lane; j < a.A; j += 64) {
    const float v = x[j];
    nan |= v != v;
    beat += (v > xl || (v == xl && j < l)) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) beat += __shfl_xor(beat, off, 64);
  const bool row_nan = __ballot(nan) != 0ull;
  if (lane == 0) a.rank[row] = lab == a.ignore_index ? -1 : (!valid || row_nan) ? a.A : beat;
  if (a.K == 0) return;
  const double lse = a.top_prob ? a.row_lse[row] : 0.0;
  float pv = 0.f;                                       // the class picked in the round before: value and index
  int pi = -1;
  bool open = !row_nan;                                 // classes are left to pick
  for (int r = 0; r < a.K; ++r) {
    float best = -INFINITY;
    int arg = INT_MAX;                                  // no candidate seen yet
    if (open) {
      for (int j = lane; j < a.A; j += 64) {            // the row comes from the cache from the second read on
        const float v = x[j];
        const bool cand = pi < 0 || v < pv || (v == pv && j > pi);
        if (cand && (arg == INT_MAX || v > best)) { best = v; arg = j; }      // ascending j: a tie keeps the lower index
      }
    }
    const float m = wave_max(best);                     // -inf from a lane without a candidate never hides a real -inf: the
    const int idx = wave_min_i(arg != INT_MAX && best == m ? arg : INT_MAX);  // index says whether anything was there
    open = idx != INT_MAX;
    if (open) { pv = m; pi = idx; }
    if (lane == 0) {
      if (a.top_ids) a.top_ids[row * a.K + r] = open ? (int64_t)idx : -1;
      if (a.top_prob) a.top_prob[row * a.K + r] = open ? expf((float)((double)m - lse)) : 0.f;
    }
  }
}

// ---- a bad id, seen by whoever stages the row: integer LDS atomics ----------------------------------------------------------------
__device__ __forceinline__ void note_bad(int *s_bad, int *s_first, int id, int G, int row) {
  if (id < -1 || id >= G) {
    atomicAdd(s_bad, 1);
    atomicMin(s_first, row);
  }
}

__device__ __forceinline__ void advance_status(int32_t *status, long long bad, int first) {
  if (!status || bad <= 0) return;
  const int seen = status[0];
  if (seen == 0) status[1] = first;
  status[0] = (int)min((long long)INT_MAX, (long long)seen + bad);
}

// ---- grouped meters -------------------------------------------------------------------------------------------------------------
struct GroupMetersArgs {
  const float *row_loss;     // [B]
  const int32_t *rank;       // [B]
  const int32_t *groups;     // [B, F]
  double *totals;            // [G, ISG_GRP_SLOTS]
  double *overall;           // [ISG_GRP_SLOTS]; optional
  double *parts;             // [workgroups, G * GM_USED + GM_TAIL]
  int32_t *status;           // [2]; optional
  int B, F, G, k, nwg;
};

__global__ __launch_bounds__(GM_THREADS) void group_meters_parts_kernel(GroupMetersArgs a) {
  __shared__ float s_loss[GM_ROWS];
  __shared__ int s_rank[GM_ROWS];
  __shared__ int s_id[GM_ROWS * ISG_EVAL_FACETS_MAX];
  __shared__ int s_bad, s_first;
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * GM_ROWS;
  const int cnt = (int)min((int64_t)GM_ROWS, (int64_t)a.B - r0);
  if (tid == 0) { s_bad = 0; s_first = INT_MAX; }
  __syncthreads();
  if (tid < cnt) {
    const int64_t r = r0 + tid;
    s_loss[tid] = a.row_loss[r];
    s_rank[tid] = a.rank[r];
    for (int f = 0; f < a.F; ++f) {
      const int id = a.groups[r * a.F + f];
      s_id[tid * a.F + f] = id;
      note_bad(&s_bad, &s_first, id, a.G, (int)r);
    }
  }
  __syncthreads();
  double *part = a.parts + (size_t)blockIdx.x * (a.G * GM_USED + GM_TAIL);
  if (tid < a.G) {                                       // thread g: the rows ascending, for group g alone
    double rows = 0.0, loss = 0.0, bad_loss = 0.0, hit1 = 0.0, hitk = 0.0;
    for (int i = 0; i < cnt; ++i) {                      // one address for the wave: LDS broadcasts
      const int rk = s_rank[i];
      if (rk < 0) continue;
      const float v = s_loss[i];
      const bool fin = isfinite(v);
      for (int f = 0; f < a.F; ++f) {
        if (s_id[i * a.F + f] != tid) continue;
        rows += 1.0;
        if (fin) loss += (double)v; else bad_loss += 1.0;
        hit1 += rk == 0 ? 1.0 : 0.0;
        hitk += rk < a.k ? 1.0 : 0.0;
      }
    }
    double *p = part + tid * GM_USED;
    p[0] = rows;
    p[1] = loss;
    p[2] = bad_loss;
    p[3] = hit1;
    p[4] = hitk;
  }
  if (tid == GM_THREADS - 1) {                           // the last wave: idle up to 192 groups, so this walk runs beside theirs
    double rows = 0.0, loss = 0.0, bad_loss = 0.0, hit1 = 0.0, hitk = 0.0;      // every counted row once, ascending
    for (int i = 0; i < cnt; ++i) {
      const int rk = s_rank[i];
      if (rk < 0) continue;
      const float v = s_loss[i];
      rows += 1.0;
      if (isfinite(v)) loss += (double)v; else bad_loss += 1.0;
      hit1 += rk == 0 ? 1.0 : 0.0;
      hitk += rk < a.k ? 1.0 : 0.0;
    }
    double *t = part + a.G * GM_USED;
    t[0] = (double)s_bad;
    t[1] = s_bad > 0 ? (double)s_first : -1.0;
    t[2] = rows;
    t[3] = loss;
    t[4] = bad_loss;
    t[5] = hit1;
    t[6] = hitk;
  }
}

__global__ __launch_bounds__(GM_THREADS) void group_meters_finish_kernel(GroupMetersArgs a) {
  const int tid = threadIdx.x, stride = a.G * GM_USED + GM_TAIL;
  for (int e = tid; e < a.G * GM_USED; e += GM_THREADS) {
    double s = 0.0;
    for (int p = 0; p < a.nwg; ++p) s += a.parts[(size_t)p * stride + e];      // workgroups ascending
    a.totals[(e / GM_USED) * ISG_GRP_SLOTS + e % GM_USED] += s;
  }
  if (a.overall && tid >= GM_THREADS - GM_USED) {        // the last five threads: the first ones may hold several group slots
    const int e = tid - (GM_THREADS - GM_USED);
    double s = 0.0;
    for (int p = 0; p < a.nwg; ++p) s += a.parts[(size_t)p * stride + a.G * GM_USED + 2 + e];
    a.overall[e] += s;
  }
  if (tid == 0 && a.status) {
    long long bad = 0;
    int first = -1;
    for (int p = 0; p < a.nwg; ++p) {
      const double *t = a.parts + (size_t)p * stride + a.G * GM_USED;
      bad += (long long)t[0];
      if (first < 0 && t[0] > 0.0) first = (int)t[1];    // rows ascend with the workgroups
    }
    advance_status(a.status, bad, first);
  }
}

// ---- grouped co-occurrence totals -----------------------------------------------------------------------------------------------
struct CooGroupsArgs {
  const int32_t *table;      // [B, 8]
  const int32_t *qflags;     // [B]; optional
  const int32_t *groups;     // [B, F]
  int64_t *totals;           // [G, ISG_COO_TOTALS]
  int32_t *status;           // [2]; optional
  int B, F, G;
};

__device__ __forceinline__ void coog_hist_add(unsigned long long *hist, int m, int hits) {
  m = min(max(m, 0), COOG_HIST - 1);
  atomicAdd(&hist[m], 1ull);                             // LDS
  atomicAdd(&hist[COOG_HIST + m], (unsigned long long)hits);
}

// Workgroup g adds the rows of group g, each as often as its facets name g: the arithmetic of isg_token_coo's finishing kernel.
__global__ __launch_bounds__(GM_THREADS) void token_coo_groups_kernel(CooGroupsArgs a) {
  __shared__ unsigned long long s_tot[ISG_COO_TOTALS];
  __shared__ int s_bad, s_first;
  const int tid = threadIdx.x, grp = blockIdx.x;
  for (int i = tid; i < ISG_COO_TOTALS; i += GM_THREADS) s_tot[i] = 0ull;
  if (tid == 0) { s_bad = 0; s_first = INT_MAX; }
  __syncthreads();
  long long acc[COOG_SUMS];
#pragma unroll
  for (int j = 0; j < COOG_SUMS; ++j) acc[j] = 0;
  for (int g = tid; g < a.B; g += GM_THREADS) {
    int times = 0;
    for (int f = 0; f < a.F; ++f) {
      const int id = a.groups[(int64_t)g * a.F + f];
      times += id == grp ? 1 : 0;
      if (grp == 0) note_bad(&s_bad, &s_first, id, a.G, g);
    }
    if (times == 0) continue;
    const int *row = a.table + (int64_t)g * 8;
    const bool correct = row[0] != 0, color = a.qflags && (a.qflags[g] & 1);
    const bool pred_in = row[1] != 0, ans_valid = correct && row[2] != 0 && !color;
    const int words = row[4], words_kept = row[5], text = row[6], text_kept = row[7];
    for (int t = 0; t < times; ++t) {
      acc[0] += 1;
      acc[1] += correct;
      acc[2] += pred_in;
      acc[3] += correct && pred_in;
      acc[4] += ans_valid;
      acc[5] += ans_valid && row[3] != 0;
      if (correct && words > 0) {
        acc[6] += 1;
        acc[7] += words;
        acc[8] += words_kept;
        coog_hist_add(s_tot + 16, words, words_kept);
      }
      if (correct && text > 0) {
        acc[9] += 1;
        acc[10] += text;
        acc[11] += text_kept;
        coog_hist_add(s_tot + 16 + 2 * COOG_HIST, text, text_kept);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < COOG_SUMS; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
    if ((tid & 63) == 0) atomicAdd(&s_tot[j], (unsigned long long)acc[j]);
  }
  __syncthreads();
  int64_t *out = a.totals + (size_t)grp * ISG_COO_TOTALS;
  for (int i = tid; i < ISG_COO_TOTALS; i += GM_THREADS)
    if (i < COOG_SUMS || i >= 16) out[i] += (int64_t)s_tot[i];
  if (grp == 0 && tid == 0) advance_status(a.status, s_bad, s_first);
}

}  // namespace isg

using namespace isg;

extern "C" int isg_eval_abi_version(void) { return ISG_EVAL_ABI_VERSION; }

extern "C" int isg_answer_rank(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, const double *row_lse,
                               int32_t *rank, int64_t *top_ids, float *top_prob, int32_t K, int64_t B, int32_t A, void *stream) {
  const bool top = top_ids || top_prob;
  if (B < 0 || A < 1 || ld < A || (top && (K < 1 || K > ISG_EVAL_TOPK_MAX)) || (top_prob && !row_lse)) return ISG_EINVAL;
  if (B >= (1ll << 31)) return !logits || !labels || !rank ? ISG_EINVAL : ISG_EUNSUPPORTED;
  RankArgs a = {.logits = logits, .labels = labels, .row_lse = row_lse, .rank = rank, .top_ids = top_ids, .top_prob = top_prob,
                .ignore_index = ignore_index, .B = (int)B, .A = A, .ld = ld, .K = top ? K : 0};
  if (a.B > 0 && (!a.logits || !a.labels || !a.rank)) return ISG_EINVAL;
  if (a.B == 0) return ISG_OK;
  answer_rank_kernel<<<(unsigned)((B + RANK_ROWS - 1) / RANK_ROWS), 64 * RANK_ROWS, 0, as_stream(stream)>>>(a);
  return check_launch();
}

static int64_t group_meters_workgroups(int64_t B) { return B > 0 ? (B + GM_ROWS - 1) / GM_ROWS : 1; }

extern "C" int64_t isg_group_meters_parts(int64_t B, int32_t G) {
  if (B < 0 || G < 1 || G > ISG_EVAL_GROUPS_MAX) return 0;
  return group_meters_workgroups(B) * ((int64_t)G * GM_USED + GM_TAIL);
}

extern "C" int isg_group_meters(const float *row_loss, const int32_t *rank, const int32_t *groups, int32_t F, int32_t G, int32_t k,
                                double *totals, double *overall, double *parts, int64_t parts_len, int32_t *status, int64_t B,
                                void *stream) {
  if (B < 0 || F < 1 || F > ISG_EVAL_FACETS_MAX || G < 1 || G > ISG_EVAL_GROUPS_MAX || k < 1) return ISG_EINVAL;
  if (B >= (1ll << 31)) return !row_loss || !rank || !groups || !totals || !parts ? ISG_EINVAL : ISG_EUNSUPPORTED;
  GroupMetersArgs a = {.row_loss = row_loss, .rank = rank, .groups = groups, .totals = totals, .overall = overall,
                       .parts = parts, .status = status,
                       .B = (int)B, .F = F, .G = G, .k = k, .nwg = (int)group_meters_workgroups(B)};
  if (a.B > 0 && (!a.row_loss || !a.rank || !a.groups || !a.totals || !a.parts)) return ISG_EINVAL;
  if (a.B == 0) return ISG_OK;
  if (parts_len < isg_group_meters_parts(B, G)) return ISG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  group_meters_parts_kernel<<<a.nwg, GM_THREADS, 0, st>>>(a);
  group_meters_finish_kernel<<<1, GM_THREADS, 0, st>>>(a);
  return check_launch();
}

extern "C" int isg_token_coo_groups(const int32_t *table, const int32_t *qflags, const int32_t *groups, int32_t F, int32_t G,
                                    int64_t *totals, int32_t *status, int64_t B, void *stream) {
  if (B < 0 || F < 1 || F > ISG_EVAL_FACETS_MAX || G < 1 || G > ISG_EVAL_GROUPS_MAX) return ISG_EINVAL;
  if (B >= (1ll << 31) - 1) return !table || !groups || !totals ? ISG_EINVAL : ISG_EUNSUPPORTED;
  CooGroupsArgs a = {.table = table, .qflags = qflags, .groups = groups, .totals = totals, .status = status, .B = (int)B, .F = F,
                     .G = G};
  if (a.B > 0 && (!a.table || !a.groups || !a.totals)) return ISG_EINVAL;
  if (a.B == 0) return ISG_OK;
  token_coo_groups_kernel<<<G, GM_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch();
}
