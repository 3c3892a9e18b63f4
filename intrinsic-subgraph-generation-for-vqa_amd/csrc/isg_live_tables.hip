// The masked layer kernel's table sets, built once per launch (include/isg_masked.h).
//
// gatv2_layer_conv_groups_kernel (csrc/isg_layer_conv.hip) opens every group of tiles with a scan: tile descriptors, then
// rowptr / src / eid / dst / ep_inv, then the masks those name -- three dependent round trips in a workgroup that is alone on its
// CU -- followed by ballots, the named rows' OR and a 4176-byte table set per tile in LDS.  None of it depends on the head or the
// weights, and a tile's four head workgroups each redo it.  Here one 256-thread workgroup per tile does it once, at full
// occupancy, and writes the table set to memory in the kernel's LDS layout (csrc/isg_live_tables.hpp); the kernel copies it in.
// Every value is formed as the kernel's scan forms it (the same clamps, the same single fp32 product of the two node masks, the
// same live test), so the same table values reach the same code.
#include "isg_common.hpp"
#include "isg_live_tables.hpp"
#include "../../include/isg_masked.h"

namespace isg {

static_assert(LG_TILE_BYTES == ISG_LIVE_TABLES_TILE_BYTES, "include/isg_masked.h states the image size");

struct LtArgs {
  const int *rowptr, *eid, *src, *dst, *ntiles;
  const float *ep_inv;              // [E] inverse scales of the edge planes
  const int4 *tile_info;            // the list the layer kernel walks: image t belongs to entry t
  const float *node_mask;           // optional: read when edge_mask is NULL
  const float *edge_mask;           // optional (NULL: node_mask[src] * node_mask[dst])
  unsigned char *tables;            // [capacity][LG_TILE_BYTES]
  int N, E;
};

__global__ __launch_bounds__(LT_ECAP) void layer_conv_live_tables_kernel(LtArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_img[LG_TILE_BYTES];
  __shared__ unsigned long long s_touch, s_livew[4];
  const int t = blockIdx.x;
  if (t >= *a.ntiles) return;
  const int tl = threadIdx.x, ll = tl & 63, wave = tl >> 6;
  const int4 d = a.tile_info[t];
  const int r0n = d.x, nrn = min(d.y, LT_ROWS), e0n = d.z, nen = min(d.w, LT_ECAP);
  for (int i = tl; i < LG_TILE_BYTES / 16; i += LT_ECAP) reinterpret_cast<uint4 *>(s_img)[i] = make_uint4(0u, 0u, 0u, 0u);
  if (tl == 0) s_touch = 0ull;
  int srcv = 0, eidv = 0, dstv = 0, rpv = 0;
  float einv = 1.f, msk = 1.f;
  if (tl <= nrn && r0n >= 0 && r0n + tl <= a.N) rpv = a.rowptr[r0n + tl];
  const bool in = tl < nen && e0n >= 0 && e0n + tl < a.E;      // a descriptor of the plan's never fails the range tests
  if (in) {
    srcv = a.src[e0n + tl];
    eidv = a.eid[e0n + tl];
    dstv = a.dst[e0n + tl];
    einv = a.ep_inv[e0n + tl];
    if (a.edge_mask)
      msk = a.edge_mask[min(max(eidv, 0), a.E - 1)];
    else
      msk = a.node_mask[min(max(srcv, 0), a.N - 1)] * a.node_mask[min(max(dstv, 0), a.N - 1)];
  }
  __syncthreads();           // the image is zero
  if (tl <= nrn) reinterpret_cast<int *>(s_img + LG_T_RP)[tl] = rpv - e0n;
  const int sx = min(max(srcv - r0n, 0), max(nrn - 1, 0));       // a source outside its tile is clamped into it
  const int dz = min(max(dstv - r0n, 0), max(nrn - 1, 0));
  const bool lv = tl < nen && (__float_as_int(msk) & 0x7fffffff) != 0;
  const unsigned long long bw = __ballot(lv);
  if (ll == 0) s_livew[wave] = bw;
  if (lv) atomicOr(&s_touch, (1ull << sx) | (1ull << dz));
  reinterpret_cast<int2 *>(s_img)[tl] = make_int2(eidv, __float_as_int(msk));
  reinterpret_cast<float *>(s_img + LG_T_LG)[tl] = lv ? einv : 0.f;        // a dead slot's logit is +0
  s_img[LG_T_SP + tl] = (unsigned char)sx;
  s_img[LG_T_DR + tl] = (unsigned char)dz;
  __syncthreads();           // ballots and the named rows complete
  int pre = 0;
  for (int i = 0; i < wave; ++i) pre += __popcll(s_livew[i]);
  if (lv) s_img[LG_T_LV + pre + __popcll(bw & ((1ull << ll) - 1ull))] = (unsigned char)tl;
  if (tl == 0) {
    *reinterpret_cast<int4 *>(s_img + LG_H_DESC) = make_int4(r0n, nrn, e0n, nen);
    *reinterpret_cast<unsigned long long *>(s_img + LG_H_TOUCH) = s_touch;
  }
  if (tl < 4) reinterpret_cast<unsigned long long *>(s_img + LG_H_LIVE)[tl] = s_livew[tl];
  __syncthreads();
  uint4 *dst = reinterpret_cast<uint4 *>(a.tables + (size_t)t * LG_TILE_BYTES);
  for (int i = tl; i < LG_TILE_BYTES / 16; i += LT_ECAP) dst[i] = reinterpret_cast<const uint4 *>(s_img)[i];
}

}  // namespace isg

using namespace isg;

extern "C" int isg_masked_abi_version(void) { return ISG_MASKED_ABI_VERSION; }

extern "C" int64_t isg_layer_conv_live_tables_bytes(int64_t capacity) { return capacity > 0 ? capacity * (int64_t)LG_TILE_BYTES : 0; }

extern "C" int isg_layer_conv_live_tables(const int32_t *rowptr, const int32_t *eid, const int32_t *src, const int32_t *dst,
                                          const float *edge_inv_scale, const int32_t *tile_info, const int32_t *ntiles,
                                          int64_t capacity, const float *node_mask, const float *edge_mask, uint8_t *tables,
                                          int64_t N, int64_t E, void *stream) {
  if (N < 0 || E < 0 || capacity < 0) return ISG_EINVAL;
  auto mis = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (mis(tables) || mis(tile_info) || N >= (1ll << 31) || E >= (1ll << 31) || capacity >= (1ll << 31)) return ISG_EUNSUPPORTED;
  if (N == 0 || capacity == 0) return ISG_OK;
  if (!node_mask && !edge_mask) return ISG_EINVAL;
  if (E > 0 && (!eid || !src || !dst || !edge_inv_scale)) return ISG_EINVAL;
  // every field named, in declaration order: -Werror=missing-field-initializers (HIP_FLAGS) refuses a field left out
  LtArgs a = {.rowptr = rowptr, .eid = eid, .src = src, .dst = dst, .ntiles = ntiles, .ep_inv = edge_inv_scale,
              .tile_info = reinterpret_cast<const int4 *>(tile_info), .node_mask = node_mask, .edge_mask = edge_mask,
              .tables = tables, .N = (int)N, .E = (int)E};
  if (!a.rowptr || (a.E > 0 && (!a.eid || !a.src || !a.dst || !a.ep_inv)) || !a.ntiles || !a.tile_info || !a.tables ||
      (!a.node_mask && !a.edge_mask))
    return ISG_EINVAL;                         // the struct the kernel dereferences, not the parameters it was filled from
  layer_conv_live_tables_kernel<<<(unsigned)capacity, LT_ECAP, 0, as_stream(stream)>>>(a);
  return check_launch();
}
