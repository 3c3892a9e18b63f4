// The tail of a training step (include/isg_optim.h): softmax cross-entropy + top-1 + running meters, the global gradient norm
// with torch's clipping coefficient, and Adam over a table of tensors.
//
// Nothing here is compute-bound and nothing is clever.  The cross-entropy reads [B, 1842] logits (30 MB at B = 4096) a wave per
// row; the two multi-tensor kernels stream fixed chunks of MT_CHUNK elements, one workgroup per chunk and a capped grid that
// strides over the rest, with 16-byte accesses wherever the addresses allow them.  No atomic in global memory: a sum is lanes
// (fp32) -> xor butterfly -> the four waves in order -> ONE finishing workgroup over rows / chunks ascending, all three in double.
#include "isg_common.hpp"
#include "isg_mt.hpp"                 // MT_CHUNK, MT_THREADS, MT_GRID_MAX, chunk_tensor, head_elems, mt_grid: shared with isg_dist.hip
#include "../../include/isg_optim.h"

#include <limits.h>
#include <math.h>

namespace isg {

constexpr int FIN_THREADS = 256;     // the finishing workgroups: thread i sums a contiguous run, thread 0 the 256 runs in order
constexpr int XENT_ROWS = 4;          // rows (waves) per workgroup of the cross-entropy kernels

// ---- cross-entropy ------------------------------------------------------------------------------------------------------------
struct XentArgs {
  const float *logits;       // [B, A], row stride ld, rows 4-byte aligned
  const int64_t *labels;     // [B]
  float *row_loss;           // [B]
  double *row_lse;           // [B]
  int32_t *pred;             // [B]
  double *stats;             // [4] = {mean_loss, n_counted, n_correct, n_rows}
  float *loss;               // optional: mean_loss once more, rounded to fp32 (what a caller hands to autograd)
  double *totals;            // optional: the running meters, ISG_TOT_*
  int64_t ignore_index;
  int B, A, ld;
};

// torch orders NaN above every number (topk, argmax): so does the top-1 here, and a NaN maximum makes the row's loss NaN
__device__ __forceinline__ bool above(float v, float m) { return v > m || (v != v && m == m); }
__device__ __forceinline__ bool same(float v, float m) { return v == m || (v != v && m != m); }

__global__ __launch_bounds__(64 * XENT_ROWS) void xent_rows_kernel(XentArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * XENT_ROWS + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const float *x = a.logits + (size_t)row * a.ld;
  float mx = -INFINITY;
  int arg = INT_MAX;                                  // no element seen yet (A < 64 leaves lanes without one)
  for (int j = lane; j < a.A; j += 64) {
    const float v = x[j];
    if (arg == INT_MAX || above(v, mx)) { mx = v; arg = j; }        // ascending j: a tie keeps the lower index
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mx, off, 64);
    const int oa = __shfl_xor(arg, off, 64);
    if (oa != INT_MAX && (arg == INT_MAX || above(om, mx) || (same(om, mx) && oa < arg))) { mx = om; arg = oa; }
  }
  float s = 0.f;
  for (int j = lane; j < a.A; j += 64) s += expf(x[j] - mx);       // the second read of a 7 KB row comes from the cache
  const double total = wave_sum_f64((double)s);       // 64 lane sums of at most ceil(A / 64) terms each, added in double
  if (lane == 0) {
    // the logarithm in double as well: a 1-ulp logf is one fp32 ulp of the LOSS when the label's logit is the maximum
    const double lse = (double)mx + log(total);
    const int64_t lab = a.labels[row];
    float loss = 0.f;
    if (lab != a.ignore_index) loss = lab < 0 || lab >= a.A ? NAN : (float)(lse - (double)x[lab]);
    a.row_lse[row] = lse;
    a.row_loss[row] = loss;
    a.pred[row] = arg;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void xent_finish_kernel(XentArgs a) {
  __shared__ double s_loss[FIN_THREADS];
  __shared__ int s_cnt[FIN_THREADS], s_cor[FIN_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = ((int64_t)a.B + FIN_THREADS - 1) / FIN_THREADS;
  const int64_t r0 = min(tid * per, (int64_t)a.B), r1 = min(r0 + per, (int64_t)a.B);
  double loss = 0.0;
  int cnt = 0, cor = 0;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t lab = a.labels[r];
    if (lab == a.ignore_index) continue;
    loss += (double)a.row_loss[r];
    cnt += 1;
    cor += lab == (int64_t)a.pred[r];
  }
  s_loss[tid] = loss;
  s_cnt[tid] = cnt;
  s_cor[tid] = cor;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < FIN_THREADS; ++i) {
    loss += s_loss[i];
    cnt += s_cnt[i];
    cor += s_cor[i];
  }
  const double mean = loss / (double)cnt;             // 0 / 0 = NaN when no row is counted, as torch gives
  const float mean32 = (float)mean;
  a.stats[0] = mean;
  a.stats[1] = (double)cnt;
  a.stats[2] = (double)cor;
  a.stats[3] = (double)a.B;
  if (a.loss) *a.loss = mean32;
  if (a.totals) {
    double *t = a.totals;
    const bool finite = isfinite(mean32);
    if (finite) {       // the reference's AverageMeter.update(loss.item(), B), which a NaN loss skips: the fp32 loss, weighted by B
      t[ISG_TOT_LOSS_SUM] += (double)mean32 * (double)a.B;
      t[ISG_TOT_LOSS_ROWS] += (double)a.B;
    }
    t[ISG_TOT_CORRECT] += (double)cor;
    t[ISG_TOT_ROWS] += (double)a.B;
    t[ISG_TOT_CALLS] += 1.0;
    if (!finite) t[ISG_TOT_NONFINITE] += 1.0;
  }
}

struct XentBwdArgs {
  const float *logits;       // [B, A], row stride ld
  const int64_t *labels;     // [B]
  const double *row_lse;     // [B]
  const double *stats;       // [4]: n_counted is read
  const float *g;            // optional: the upstream gradient, one fp32; NULL = 1
  float *d_logits;           // [B, A], row stride ldd
  int64_t ignore_index;
  int B, A, ld, ldd;
};

__global__ __launch_bounds__(64 * XENT_ROWS) void xent_bwd_kernel(XentBwdArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * XENT_ROWS + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const float *x = a.logits + (size_t)row * a.ld;
  float *d = a.d_logits + (size_t)row * a.ldd;
  const int64_t lab = a.labels[row];
  if (lab == a.ignore_index || lab < 0 || lab >= a.A) {
    const float fill = lab == a.ignore_index ? 0.f : NAN;
    for (int j = lane; j < a.A; j += 64) d[j] = fill;
    return;
  }
  const double lse = a.row_lse[row];
  const float scale = (a.g ? *a.g : 1.f) / (float)a.stats[1];
  const int hot = (int)lab;
  for (int j = lane; j < a.A; j += 64) {
    // exp(x - lse) with the difference taken in double: its fp32 rounding (hi) goes through expf, what the rounding dropped
    // (lo, below 2^-24 |hi|) comes back as the factor 1 + lo -- near 1e4 an fp32 difference would keep three digits
    const double diff = (double)x[j] - lse;
    const float hi = (float)diff, lo = (float)(diff - (double)hi);
    float p = expf(hi);
    p = fmaf(p, lo, p);
    d[j] = (p - (j == hot ? 1.f : 0.f)) * scale;
  }
}

// ---- the tensor table (its geometry: isg_mt.hpp) --------------------------------------------------------------------------------
// Sum of the lanes' fp32 totals over the workgroup, in double and in a fixed order: the xor butterfly inside a wave, then the
// four waves ascending.  Every thread returns the total.  (Added in fp32, the 256 lane totals of a 4096-element chunk cost the
// norm a whole fp32 ulp; in double the lanes' own roundings are all that is left, and they average out.)  `s` is 4 doubles of
// LDS; the trailing barrier lets the caller's next chunk reuse it.
__device__ __forceinline__ double block_sum(float lane_total, double *s) {
  const double v = wave_sum_f64((double)lane_total);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = dadd_rn(dadd_rn(dadd_rn(s[0], s[1]), s[2]), s[3]);
  __syncthreads();
  return t;
}

struct SqnormArgs {
  const int64_t *table;      // [T][4]: column 1, the gradient's address, is read
  const int64_t *numel;      // [T]
  const int64_t *prefix;     // [T + 1]
  double *parts;             // [chunks]
  float *clip;               // [4] = {norm, coef, finite, 0}
  int T;
  int64_t chunks;
  float max_norm;
};

__global__ __launch_bounds__(MT_THREADS) void mt_sqnorm_kernel(SqnormArgs a) {
  __shared__ double s_wave[4];
  const int tid = threadIdx.x;
  const int64_t base = a.prefix[0];
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    const int t = chunk_tensor(a.prefix, a.T, c + base);
    const int64_t start = (c + base - a.prefix[t]) * MT_CHUNK;
    const int n = (int)max((int64_t)0, min((int64_t)MT_CHUNK, a.numel[t] - start));
    const float *g = reinterpret_cast<const float *>(a.table[4 * (int64_t)t + 1]) + start;
    const int head = min(n, head_elems(g)), nv = (n - head) >> 2, tail0 = head + 4 * nv;
    float acc = 0.f;
    if (tid < head) acc = g[tid] * g[tid];
    const float4 *gv = reinterpret_cast<const float4 *>(g + head);
    for (int i = tid; i < nv; i += MT_THREADS) {
      const float4 v = gv[i];
      acc = fmaf(v.x, v.x, acc);
      acc = fmaf(v.y, v.y, acc);
      acc = fmaf(v.z, v.z, acc);
      acc = fmaf(v.w, v.w, acc);
    }
    if (tid < n - tail0) acc = fmaf(g[tail0 + tid], g[tail0 + tid], acc);
    const double total = block_sum(acc, s_wave);
    if (tid == 0) a.parts[c] = total;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void mt_sqnorm_finish_kernel(SqnormArgs a) {
  __shared__ double s_sum[FIN_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (a.chunks + FIN_THREADS - 1) / FIN_THREADS;
  const int64_t c0 = min(tid * per, a.chunks), c1 = min(c0 + per, a.chunks);
  double sum = 0.0;
  for (int64_t c = c0; c < c1; ++c) sum += a.parts[c];
  s_sum[tid] = sum;
  __syncthreads();
  if (tid != 0) return;
  for (int i = 1; i < FIN_THREADS; ++i) sum += s_sum[i];
  const float norm = (float)sqrt(sum);
  float coef = 1.f;
  if (a.max_norm > 0.f) {                             // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
    const float c = a.max_norm / (norm + 1e-6f);
    coef = c < 1.f || c != c ? c : 1.f;
  }
  a.clip[0] = norm;
  a.clip[1] = coef;
  a.clip[2] = isfinite(norm) ? 1.f : 0.f;
  a.clip[3] = 0.f;
}

// ---- Adam ---------------------------------------------------------------------------------------------------------------------
struct AdamStepArgs {
  const float *clip;         // optional: {norm, coef, finite, 0} of isg_mt_sqnorm; NULL = the step always applies
  double *step;              // the step counter every parameter shares
  double *state;             // [4] = {bc1, bc2, applies, step}
  double *skipped;           // steps skipped so far
  int advance;
  double beta1, beta2;
};

__global__ __launch_bounds__(64) void mt_adam_step_kernel(AdamStepArgs a) {
  if (threadIdx.x != 0) return;
  const bool applies = !a.clip || a.clip[2] != 0.f;
  double step = *a.step;
  if (applies && a.advance) {
    step += 1.0;
    *a.step = step;
  }
  if (!applies && a.advance) *a.skipped += 1.0;
  a.state[0] = 1.0 - pow(a.beta1, step);
  a.state[1] = 1.0 - pow(a.beta2, step);
  a.state[2] = applies ? 1.0 : 0.0;
  a.state[3] = step;
}

struct AdamArgs {
  const int64_t *table;      // [T][4]: (param, grad, exp_avg, exp_avg_sq)
  const int64_t *numel;      // [T]
  const int64_t *prefix;     // [T + 1]
  const float *clip;         // optional: coef = clip[1]; NULL = 1
  const double *state;       // [4] of the prologue
  int T;
  int64_t chunks;
  double lr, beta1, beta2, eps, wd;
  int decoupled;
};

struct AdamK {      // the step's scalars as torch hands them to its fp32 kernels: formed in double, rounded once
  float coef, wd, decay, w1, b2, w2, step_size, bc2_sqrt, eps;
  bool decoupled;
};

// torch.optim.adam._single_tensor_adam, statement by statement
__device__ __forceinline__ void adam_update(float &p, float g, float &m, float &v, const AdamK &k) {
  g = mul_rn(g, k.coef);                              // clip_grad_norm_: g.mul_(coef), rounded before anything consumes it
  if (k.wd != 0.f) {
    if (k.decoupled) p = mul_rn(p, k.decay);          // AdamW: param.mul_(1 - lr * wd)
    else g = g + k.wd * p;                            // grad.add(param, alpha = wd)
  }
  m = m + (g - m) * k.w1;                             // exp_avg.lerp_(grad, 1 - beta1)
  v = v * k.b2 + g * g * k.w2;                        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;  // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
  p = p - k.step_size * (m / denom);                  // param.addcdiv_(exp_avg, denom, value = -lr / bc1)
}

__global__ __launch_bounds__(MT_THREADS) void mt_adam_kernel(AdamArgs a) {
  if (a.state[2] == 0.0) return;                      // a nonfinite gradient norm: the step is skipped as a whole
  const int tid = threadIdx.x;
  const AdamK k = {.coef = a.clip ? a.clip[1] : 1.f, .wd = (float)a.wd, .decay = (float)(1.0 - a.lr * a.wd),
                   .w1 = (float)(1.0 - a.beta1), .b2 = (float)a.beta2, .w2 = (float)(1.0 - a.beta2),
                   .step_size = (float)(a.lr / a.state[0]), .bc2_sqrt = (float)sqrt(a.state[1]), .eps = (float)a.eps,
                   .decoupled = a.decoupled != 0};
  const int64_t base = a.prefix[0];
  for (int64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {
    const int t = chunk_tensor(a.prefix, a.T, c + base);
    const int64_t start = (c + base - a.prefix[t]) * MT_CHUNK;
    const int n = (int)max((int64_t)0, min((int64_t)MT_CHUNK, a.numel[t] - start));
    const int64_t *row = a.table + 4 * (int64_t)t;
    float *p = reinterpret_cast<float *>(row[0]) + start;
    const float *g = reinterpret_cast<const float *>(row[1]) + start;
    float *m = reinterpret_cast<float *>(row[2]) + start;
    float *v = reinterpret_cast<float *>(row[3]) + start;
    // the float4 body needs ONE head for all four: the same offset from a 16-byte boundary (chunks are whole multiples of 16 B,
    // so a tensor's chunks all agree).  Separate allocations share it; views at odd offsets of a flat buffer may not: scalars.
    const int hp = head_elems(p);
    const bool vec = hp == head_elems(g) && hp == head_elems(m) && hp == head_elems(v);
    const int head = vec ? min(n, hp) : n, nv = (n - head) >> 2, tail0 = head + 4 * nv;
    for (int i = tid; i < head; i += MT_THREADS) {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_update(pi, g[i], mi, vi, k);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    float4 *pv = reinterpret_cast<float4 *>(p + head), *mv = reinterpret_cast<float4 *>(m + head),
           *vv = reinterpret_cast<float4 *>(v + head);
    const float4 *gv = reinterpret_cast<const float4 *>(g + head);
    for (int i = tid; i < nv; i += MT_THREADS) {
      float4 p4 = pv[i], m4 = mv[i], v4 = vv[i];
      const float4 g4 = gv[i];
      adam_update(p4.x, g4.x, m4.x, v4.x, k);
      adam_update(p4.y, g4.y, m4.y, v4.y, k);
      adam_update(p4.z, g4.z, m4.z, v4.z, k);
      adam_update(p4.w, g4.w, m4.w, v4.w, k);
      pv[i] = p4; mv[i] = m4; vv[i] = v4;
    }
    if (tid < n - tail0) {
      const int i = tail0 + tid;
      float pi = p[i], mi = m[i], vi = v[i];
      adam_update(pi, g[i], mi, vi, k);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

}  // namespace isg

using namespace isg;

extern "C" int isg_optim_abi_version(void) { return ISG_OPTIM_ABI_VERSION; }

extern "C" int isg_xent_fwd(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, float *row_loss,
                            double *row_lse, int32_t *pred, double *stats, float *loss, double *totals, int64_t B, int32_t A,
                            void *stream) {
  if (B < 0 || A < 1 || ld < A) return ISG_EINVAL;
  if (B >= (1ll << 31)) return ISG_EUNSUPPORTED;
  XentArgs a = {.logits = logits, .labels = labels, .row_loss = row_loss, .row_lse = row_lse, .pred = pred, .stats = stats,
                .loss = loss, .totals = totals, .ignore_index = ignore_index, .B = (int)B, .A = A, .ld = ld};
  if (!a.stats || (a.B > 0 && (!a.logits || !a.labels || !a.row_loss || !a.row_lse || !a.pred))) return ISG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (a.B > 0) xent_rows_kernel<<<(unsigned)((a.B + XENT_ROWS - 1) / XENT_ROWS), 64 * XENT_ROWS, 0, st>>>(a);
  xent_finish_kernel<<<1, FIN_THREADS, 0, st>>>(a);
  return check_launch();
}

extern "C" int isg_xent_bwd(const float *logits, int32_t ld, const int64_t *labels, int64_t ignore_index, const double *row_lse,
                            const double *stats, const float *g, float *d_logits, int32_t ldd, int64_t B, int32_t A, void *stream) {
  if (B < 0 || A < 1 || ld < A || ldd < A) return ISG_EINVAL;
  if (B >= (1ll << 31)) return ISG_EUNSUPPORTED;
  if (B == 0) return ISG_OK;
  XentBwdArgs a = {.logits = logits, .labels = labels, .row_lse = row_lse, .stats = stats, .g = g, .d_logits = d_logits,
                   .ignore_index = ignore_index, .B = (int)B, .A = A, .ld = ld, .ldd = ldd};
  if (!a.logits || !a.labels || !a.row_lse || !a.stats || !a.d_logits) return ISG_EINVAL;
  xent_bwd_kernel<<<(unsigned)((a.B + XENT_ROWS - 1) / XENT_ROWS), 64 * XENT_ROWS, 0, as_stream(stream)>>>(a);
  return check_launch();
}

extern "C" int32_t isg_mt_chunk_elems(void) { return MT_CHUNK; }

extern "C" int64_t isg_mt_sqnorm_parts(int64_t total_chunks) { return total_chunks > 1 ? total_chunks : 1; }

extern "C" int isg_mt_sqnorm(const int64_t *table, const int64_t *numel, const int64_t *chunk_prefix, int32_t T,
                             int64_t total_chunks, double *parts, float max_norm, float *clip, void *stream) {
  if (T < 0 || total_chunks < 0 || (T == 0 && total_chunks != 0)) return ISG_EINVAL;
  SqnormArgs a = {.table = table, .numel = numel, .prefix = chunk_prefix, .parts = parts, .clip = clip, .T = T,
                  .chunks = total_chunks, .max_norm = max_norm};
  if (!a.clip || (a.chunks > 0 && (!a.table || !a.numel || !a.prefix || !a.parts))) return ISG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (a.chunks > 0) mt_sqnorm_kernel<<<mt_grid(a.chunks), MT_THREADS, 0, st>>>(a);
  mt_sqnorm_finish_kernel<<<1, FIN_THREADS, 0, st>>>(a);
  return check_launch();
}

extern "C" int isg_mt_adam(const int64_t *table, const int64_t *numel, const int64_t *chunk_prefix, int32_t T, int64_t total_chunks,
                           const float *clip, double *step, double *state, double *skipped, int32_t advance, double lr,
                           double beta1, double beta2, double eps, double wd, int32_t decoupled, void *stream) {
  if (T < 0 || total_chunks < 0 || (T == 0 && total_chunks != 0)) return ISG_EINVAL;
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(wd >= 0.0))
    return ISG_EINVAL;
  AdamStepArgs s = {.clip = clip, .step = step, .state = state, .skipped = skipped, .advance = advance, .beta1 = beta1,
                    .beta2 = beta2};
  if (!s.step || !s.state || !s.skipped) return ISG_EINVAL;
  AdamArgs a = {.table = table, .numel = numel, .prefix = chunk_prefix, .clip = clip, .state = state, .T = T,
                .chunks = total_chunks, .lr = lr, .beta1 = beta1, .beta2 = beta2, .eps = eps, .wd = wd, .decoupled = decoupled};
  if (!a.state || (a.chunks > 0 && (!a.table || !a.numel || !a.prefix))) return ISG_EINVAL;
  hipStream_t st = as_stream(stream);
  mt_adam_step_kernel<<<1, 64, 0, st>>>(s);
  if (a.chunks > 0) mt_adam_kernel<<<mt_grid(a.chunks), MT_THREADS, 0, st>>>(a);
  return check_launch();
}
