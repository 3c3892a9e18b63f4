// Attention rollout (include/ext/isg_rollout.h): the read-out's pooling weights walked back through the layers' head-averaged
// attention weights with a residual share per layer -- a node attribution from one forward; DESIGN.md 35.
//
// One wave per graph, in a workgroup of its own (64 threads: __syncthreads() is the wave's own barrier, and the strict twin is
// this code).  The graph's two relevance vectors live in dynamic LDS, ping-pong (2 x nmax floats, each a multiple of 16 bytes).
// Lane i owns the source nodes i, i + 64, ...: per layer it walks its nodes' out-slots in order, reads the slot's row of alpha,
// the two mask entries and r[dst - ptr[g]] from LDS, stores the slot's flow and then the node's new relevance.  All L layers run
// in the one launch; the only barriers stand in the loop over the layers, whose trip count is the same for every workgroup, and
// none stands in a loop whose trip count depends on the graph.  Every sum is plain fp32 with nothing contracted (add_rn /
// mul_rn), in an order the header states, so the result is a function of the inputs alone; both load paths of the alpha row add
// the heads in the same order.  No atomics: a node's relevance and an edge's flow have one writer.  Every number read from
// memory that becomes an address is clamped or compared first, so a bad ptr, rowptr_s, eid_s or dst_s gives wrong rows and never
// a fault.
#include "isg_common.hpp"

#include "../../include/ext/isg_rollout.h"

namespace isg {

constexpr int ROLL_MAX_LAYERS = 8;
constexpr int ROLL_MAX_NODES = 4096;          // 2 x 4096 floats = 32 KiB of dynamic LDS, half of what a workgroup gets unasked
constexpr int ROLL_THREADS = ISG_WAVE;

struct RollLayer {
  const float *alpha;            // fp32 [E, H] by edge id, row stride lda; may be NULL when E == 0
  const float *mask;             // fp32 [N], or NULL: all ones
  int lda;
  int vec4;                      // H == 4, lda a multiple of 4 and a 16-byte aligned base: one 16-byte load per row
};
struct RollLayers {
  RollLayer l[ROLL_MAX_LAYERS];
};

struct RollArgs {
  const int *ptr;                // int32 [B + 1]
  const int *rowptr_s;           // int32 [N + 1]
  const int *eid_s;              // int32 [E]; may be NULL when E == 0
  const int *dst_s;              // int32 [E]; may be NULL when E == 0
  RollLayers layers;
  int L, H;
  float lambda, one_minus;       // the residual share and the fp32 value of 1 - lambda
  float inv_h;                   // the fp32 value of 1 / H
  const float *start;            // fp32 [N]
  int N, E, B, nmax;
  int stride;                    // floats between the two LDS vectors: nmax rounded up to a multiple of 4
  float *relevance;              // fp32 [N]
  float *edge_flow;              // fp32 [L, E], row stride E; NULL: optional, no flow is stored
};

// the head-averaged attention weight of edge e: the heads added h ascending, then one multiplication by 1 / H -- on both paths
__device__ __forceinline__ float roll_head_mean(const RollLayer &ly, int e, int H, float inv_h) {
  const float *row = ly.alpha + (int64_t)e * ly.lda;
  float s;
  if (ly.vec4) {
    const float4 v = *reinterpret_cast<const float4 *>(row);
    s = add_rn(add_rn(add_rn(v.x, v.y), v.z), v.w);
  } else {
    s = row[0];
    for (int h = 1; h < H; ++h) s = add_rn(s, row[h]);
  }
  return mul_rn(s, inv_h);
}

__global__ __launch_bounds__(ROLL_THREADS, 8) void attention_rollout_kernel(RollArgs a) {
  extern __shared__ __align__(16) float roll_lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int lo = max(0, min(a.ptr[g], a.N));
  const int hi = max(lo, min(a.ptr[g + 1], a.N));
  const int n = hi - lo;
  if (n > a.nmax) {                                              // (the whole workgroup: no barrier is left waiting)
    for (int i = lane; i < n; i += ROLL_THREADS) a.relevance[lo + i] = __int_as_float(0x7fc00000);
    return;
  }
  float *cur = roll_lds, *nxt = roll_lds + a.stride;
  for (int i = lane; i < n; i += ROLL_THREADS) cur[i] = a.start[lo + i];
  __syncthreads();
  for (int l = a.L - 1; l >= 0; --l) {                           // (uniform over the grid)
    const RollLayer ly = a.layers.l[l];
    float *flow = a.edge_flow ? a.edge_flow + (int64_t)l * a.E : nullptr;
    for (int i = lane; i < n; i += ROLL_THREADS) {
      const int s = lo + i;
      const int jlo = max(0, min(a.rowptr_s[s], a.E));
      const int jhi = max(jlo, min(a.rowptr_s[s + 1], a.E));
      const float ms = ly.mask ? ly.mask[s] : 1.0f;
      float acc = mul_rn(a.lambda, cur[i]);
      for (int j = jlo; j < jhi; ++j) {
        const int e = a.eid_s[j], d = a.dst_s[j];
        if (e < 0 || e >= a.E || d < lo || d >= hi) continue;    // contributes nothing, is never an address
        float w = roll_head_mean(ly, e, a.H, a.inv_h);
        if (ly.mask) w = mul_rn(mul_rn(w, ms), ly.mask[d]);      // (without a mask: twice times 1.0f, the same bits)
        const float f = mul_rn(mul_rn(a.one_minus, w), cur[d - lo]);
        if (flow) flow[e] = f;
        acc = add_rn(acc, f);
      }
      nxt[i] = acc;
    }
    __syncthreads();                                             // r_l is complete before anyone reads it as r_{l+1}
    float *t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int i = lane; i < n; i += ROLL_THREADS) a.relevance[lo + i] = cur[i];
}

}  // namespace isg

using namespace isg;

extern "C" int isg_rollout_abi_version(void) { return ISG_ROLLOUT_ABI_VERSION; }
extern "C" int isg_rollout_max_layers(void) { return ROLL_MAX_LAYERS; }
extern "C" int isg_rollout_max_nodes(void) { return ROLL_MAX_NODES; }

static inline bool roll_too_large(int64_t v) { return v >= (1ll << 31) - 1024; }

extern "C" int isg_attention_rollout(const int32_t *ptr, const int32_t *rowptr_s, const int32_t *eid_s, const int32_t *dst_s,
                                     const int64_t *layers, int64_t L, int64_t H, float residual, const float *start, int64_t N,
                                     int64_t E, int64_t B, int64_t nmax, float *relevance, float *edge_flow, void *stream) {
  if (N < 0 || E < 0 || B < 0 || nmax < 0 || L < 1 || H < 1) return ISG_EINVAL;
  if (!(residual >= 0.0f && residual <= 1.0f)) return ISG_EINVAL;                   // (a NaN compares false)
  if (L > ROLL_MAX_LAYERS || nmax > ROLL_MAX_NODES || roll_too_large(N) || roll_too_large(E) || roll_too_large(B) ||
      roll_too_large(H))
    return ISG_EUNSUPPORTED;
  if (B == 0 || N == 0) return ISG_OK;
  if (!layers) return ISG_EINVAL;
  RollLayers table;
  for (int i = 0; i < ROLL_MAX_LAYERS; ++i) {
    const int64_t *f = layers + 3 * (int64_t)(i < L ? i : 0);                        // unused slots repeat layer 0 (never read)
    const float *alpha = reinterpret_cast<const float *>(f[0]);
    const int64_t lda = f[1];
    if (lda < H || (E > 0 && !alpha)) return ISG_EINVAL;
    if (roll_too_large(lda)) return ISG_EUNSUPPORTED;
    const int vec4 = H == 4 && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(alpha) & 15u) == 0;
    table.l[i] = RollLayer{alpha, reinterpret_cast<const float *>(f[2]), (int)lda, vec4};
  }
  const int stride = ((int)nmax + 3) / 4 * 4;
  RollArgs a = {.ptr = ptr, .rowptr_s = rowptr_s, .eid_s = eid_s, .dst_s = dst_s, .layers = table, .L = (int)L, .H = (int)H,
                .lambda = residual, .one_minus = 1.0f - residual, .inv_h = 1.0f / (float)H, .start = start, .N = (int)N,
                .E = (int)E, .B = (int)B, .nmax = (int)nmax, .stride = stride, .relevance = relevance, .edge_flow = edge_flow};
  if (!a.ptr || !a.rowptr_s || !a.start || !a.relevance || (a.E > 0 && (!a.eid_s || !a.dst_s))) return ISG_EINVAL;
  attention_rollout_kernel<<<(unsigned)B, ROLL_THREADS, 2 * (size_t)stride * sizeof(float), as_stream(stream)>>>(a);
  return check_launch();
}
