// Token co-occurrence of a whole batch: is the answer's name among the picked nodes, how many question words (and kept text
// tokens) name an object of the graph, how many of those objects were picked -- per question, and as running totals.
//
// All integer and exact.  Launch 1: one wave per question.  The lanes hold the question's tokens (two per lane per table; lanes
// 0 and 1 also hold the predicted and the true answer's vocabulary id); the graph's names go through LDS COO_NODE_CHUNK at a
// time, once as they are and once with the un-kept nodes blanked, and every lane compares its values with every staged name.
// Ballots + popcounts turn the lanes' flags into the row of the table.  Launch 2 (only when the caller keeps totals): ONE
// workgroup walks the table, sums in registers and LDS, and adds the result to `totals` with plain loads and stores -- stream
// order is the only hand-off, nothing is accumulated atomically in global memory, so the outputs are a function of the inputs.
#include "isg_common.hpp"

namespace isg {

constexpr int COO_NODE_CHUNK = 256;                                  // nodes of a graph staged in LDS per pass
constexpr int COO_PER_LANE = ISG_COO_TOKENS_MAX / ISG_WAVE;          // tokens of one table a lane holds
constexpr int COO_VALUES = 2 * COO_PER_LANE + 1;                     // question words, text tokens, one answer id
constexpr int COO_HIST = ISG_COO_TOKENS_MAX + 1;                     // match counts 0 .. ISG_COO_TOKENS_MAX
constexpr int COO_SUMS = 12;                                         // totals[0 .. 12); [12, 16) reserved
constexpr int COO_TOT_THREADS = 256;
constexpr int COO_NO_NAME = -1, COO_NO_TOKEN = -2;                   // a blanked name never equals a blanked token
static_assert(COO_PER_LANE * ISG_WAVE == ISG_COO_TOKENS_MAX && ISG_COO_TOTALS == 16 + 4 * COO_HIST, "header and kernel disagree");

struct TokenCooArgs {
  const int64_t *names;          // int64, node n at names[n * name_stride]; may be NULL when N == 0
  int name_stride;
  const float *node_mask;        // fp32 [N]; may be NULL when N == 0
  float threshold;
  const int *ptr;                // int32 [B + 1]
  const int64_t *pred, *label;   // int64 [B]; may be NULL when B == 0
  const int *ans_sg;             // int32 [A]; may be NULL when A == 0
  const int *qtok;               // int32 [B, T]; may be NULL when T == 0
  const int *qflags;             // int32 [B]; optional (NULL: all 0)
  const int *ttok;               // int32 [B, T2]; may be NULL when T2 == 0
  const float *tkeep;            // fp32 [B, T2]; may be NULL when T2 == 0
  int N, B, A, T, T2;
  int *table;                    // int32 [B, 8]; may be NULL when B == 0
  int64_t *totals;               // int64 [ISG_COO_TOTALS]; optional (NULL: the table only)
};

__device__ __forceinline__ int coo_answer(const TokenCooArgs &a, int64_t cls) {
  return cls >= 0 && cls < a.A ? a.ans_sg[cls] : -1;
}

__global__ __launch_bounds__(ISG_WAVE) void token_coo_rows_kernel(TokenCooArgs a) {
  __shared__ int s_name[COO_NODE_CHUNK];       // name of every staged node (COO_NO_NAME: not an int32 >= 0)
  __shared__ int s_kept[COO_NODE_CHUNK];       // the same, COO_NO_NAME where the node is not kept
  const int lane = threadIdx.x, g = blockIdx.x;
  const int64_t pr = a.pred[g], lb = a.label[g];
  int v[COO_VALUES];
#pragma unroll
  for (int u = 0; u < COO_PER_LANE; ++u) {
    const int t = u * ISG_WAVE + lane;
    const int q = t < a.T ? a.qtok[(int64_t)g * a.T + t] : -1;
    const int x = t < a.T2 && a.tkeep[(int64_t)g * a.T2 + t] == 1.0f ? a.ttok[(int64_t)g * a.T2 + t] : -1;      // a NaN is not 1
    v[u] = q >= 0 ? q : COO_NO_TOKEN;
    v[COO_PER_LANE + u] = x >= 0 ? x : COO_NO_TOKEN;
  }
  const int ans = lane == 0 ? coo_answer(a, pr) : lane == 1 ? coo_answer(a, lb) : -1;
  v[COO_VALUES - 1] = ans >= 0 ? ans : COO_NO_TOKEN;
  unsigned in_graph = 0, in_kept = 0;          // bit j: value j names a node / a kept node
  const int lo = min(max(a.ptr[g], 0), a.N), hi = min(max(a.ptr[g + 1], lo), a.N);
  for (int base = lo; base < hi; base += COO_NODE_CHUNK) {      // lo, hi are the wave's: every lane takes every barrier
    const int cnt = min(COO_NODE_CHUNK, hi - base);
    __syncthreads();                           // the chunk before this one has been read
    for (int i = lane; i < cnt; i += ISG_WAVE) {
      const int n = base + i;
      const int64_t nm = a.names[(int64_t)n * a.name_stride];
      const int nm32 = nm >= 0 && nm <= INT32_MAX ? (int)nm : COO_NO_NAME;
      s_name[i] = nm32;
      s_kept[i] = a.node_mask[n] > a.threshold ? nm32 : COO_NO_NAME;      // a NaN compares false
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const int nm = s_name[i], kn = s_kept[i];                  // one address for the wave: a broadcast
#pragma unroll
      for (int j = 0; j < COO_VALUES; ++j) {
        in_graph |= (unsigned)(v[j] == nm) << j;
        in_kept |= (unsigned)(v[j] == kn) << j;
      }
    }
  }
  int words = 0, words_kept = 0, text = 0, text_kept = 0;
#pragma unroll
  for (int u = 0; u < COO_PER_LANE; ++u) {
    words += __popcll(__ballot((in_graph >> u) & 1u));
    words_kept += __popcll(__ballot((in_kept >> u) & 1u));
    text += __popcll(__ballot((in_graph >> (COO_PER_LANE + u)) & 1u));
    text_kept += __popcll(__ballot((in_kept >> (COO_PER_LANE + u)) & 1u));
  }
  const unsigned long long ans_graph = __ballot((in_graph >> (COO_VALUES - 1)) & 1u);
  const unsigned long long ans_kept = __ballot((in_kept >> (COO_VALUES - 1)) & 1u);
  if (lane < 8) {
    const int col = lane == 0 ? (int)(pr == lb) : lane == 1 ? (int)(ans_graph & 1ull) : lane == 2 ? (int)((ans_graph >> 1) & 1ull)
                  : lane == 3 ? (int)(ans_kept & 1ull) : lane == 4 ? words : lane == 5 ? words_kept : lane == 6 ? text : text_kept;
    a.table[(int64_t)g * 8 + lane] = col;
  }
}

__device__ __forceinline__ void coo_hist_add(unsigned long long *hist, int m, int hits) {
  m = min(max(m, 0), COO_HIST - 1);
  atomicAdd(&hist[m], 1ull);                   // LDS
  atomicAdd(&hist[COO_HIST + m], (unsigned long long)hits);
}

__global__ __launch_bounds__(COO_TOT_THREADS) void token_coo_totals_kernel(TokenCooArgs a) {
  __shared__ unsigned long long s_tot[ISG_COO_TOTALS];
  const int tid = threadIdx.x;
  for (int i = tid; i < ISG_COO_TOTALS; i += COO_TOT_THREADS) s_tot[i] = 0ull;
  __syncthreads();
  long long acc[COO_SUMS];
#pragma unroll
  for (int j = 0; j < COO_SUMS; ++j) acc[j] = 0;
  for (int g = tid; g < a.B; g += COO_TOT_THREADS) {
    const int *row = a.table + (int64_t)g * 8;
    const bool correct = row[0] != 0, color = a.qflags && (a.qflags[g] & 1);
    const bool pred_in = row[1] != 0, ans_valid = correct && row[2] != 0 && !color;
    const int words = row[4], words_kept = row[5], text = row[6], text_kept = row[7];
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
      coo_hist_add(s_tot + 16, words, words_kept);
    }
    if (correct && text > 0) {
      acc[9] += 1;
      acc[10] += text;
      acc[11] += text_kept;
      coo_hist_add(s_tot + 16 + 2 * COO_HIST, text, text_kept);
    }
  }
#pragma unroll
  for (int j = 0; j < COO_SUMS; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
    if ((tid & 63) == 0) atomicAdd(&s_tot[j], (unsigned long long)acc[j]);
  }
  __syncthreads();
  for (int i = tid; i < ISG_COO_TOTALS; i += COO_TOT_THREADS)
    if (i < COO_SUMS || i >= 16) a.totals[i] += (int64_t)s_tot[i];
}

}  // namespace isg

using namespace isg;

extern "C" int isg_token_coo(const int64_t *names, int64_t name_stride, const float *node_mask, float threshold, const int32_t *ptr,
                             const int64_t *pred, const int64_t *label, const int32_t *ans_sg, const int32_t *qtok,
                             const int32_t *qflags, const int32_t *ttok, const float *tkeep, int64_t N, int64_t B, int64_t A,
                             int32_t T, int32_t T2, int32_t *table, int64_t *totals, void *stream) {
  if (N < 0 || B < 0 || A < 0 || T < 0 || T2 < 0 || name_stride < 1) return ISG_EINVAL;
  const int64_t lim = (1ll << 31) - 1;
  if (T > ISG_COO_TOKENS_MAX || T2 > ISG_COO_TOKENS_MAX || N >= lim || B >= lim || A >= lim || name_stride >= lim)
    return ISG_EUNSUPPORTED;
  TokenCooArgs a = {.names = names, .name_stride = (int)name_stride, .node_mask = node_mask, .threshold = threshold, .ptr = ptr,
                    .pred = pred, .label = label, .ans_sg = ans_sg, .qtok = qtok, .qflags = qflags, .ttok = ttok, .tkeep = tkeep,
                    .N = (int)N, .B = (int)B, .A = (int)A, .T = T, .T2 = T2, .table = table, .totals = totals};
  if (!a.ptr || (a.N > 0 && (!a.names || !a.node_mask)) || (a.B > 0 && (!a.pred || !a.label || !a.table)) ||
      (a.A > 0 && !a.ans_sg) || (a.T > 0 && !a.qtok) || (a.T2 > 0 && (!a.ttok || !a.tkeep)))
    return ISG_EINVAL;
  if (a.B == 0) return ISG_OK;
  hipStream_t st = as_stream(stream);
  token_coo_rows_kernel<<<a.B, ISG_WAVE, 0, st>>>(a);
  if (a.totals) token_coo_totals_kernel<<<1, COO_TOT_THREADS, 0, st>>>(a);
  return check_launch();
}
