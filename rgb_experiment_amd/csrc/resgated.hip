// ResGatedGraphConv (residual gated graph convolution): fused per-channel gate + aggregation and its backward, for
// gfx950. Stands in for ResGatedGraphConv.forward / message [PyG] (Bresson & Laurent, "Residual Gated Graph ConvNets";
// the benchmarking literature's GatedGCN).
//
// For an edge j -> i in forward CSR slot p, with k, q, v [N, C] (each its own pointer and leading dimension; the layer
// hands q and v as neighbouring column blocks of one product, so the two rows of a source are one stream):
//   s_p      = sigmoid(k[i,:] + q[j,:])            (a VECTOR per edge: one gate per channel)
//   out[i,:] = sum_p s_p (.) v[j,:]
// No softmax, no normaliser, no head reduction: the lane layout is attn_common.h's with H = 1 (a row fragment of VEC
// channels per lane, G lanes per neighbour row, 64 / G rows per wave-instruction), and a lane never talks to its
// neighbours inside a slot. The edges are taken as given, so a row may have no slot at all: it stores exact zeros.
//
// Nothing per edge is written or read back and no record passes between the kernels: both backward passes recompute
// the gate from k, q alone. No float atomics; every sum runs in a fixed order (slots of a lane group in slot order, lane
// groups by a butterfly, hub-row chunks in chunk order).
#include <cmath>

#include "edge_common.h"

namespace rgbx {
namespace {

// sigmoid(z) through e = exp(-|z|) in [0, 1]: the denominator 1 + e stays in [1, 2] and nothing on the way can
// overflow, whatever z is (for |z| > 104 e underflows to 0 and s is exactly 0 or 1). One division serves both branches.
__device__ __forceinline__ float gate(float z) {
  const float e = expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) / (1.f + e);
}

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR: the target's k row stays in registers, per slot the q and v rows of the source
// are gathered (U slots in flight per lane group). CHUNK: the wave owns a chunk of a hub row and leaves its partial sum.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
resgated_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ kx,
                    int64_t ldk, const float* __restrict__ qx, int64_t ldq, const float* __restrict__ vx, int64_t ldv,
                    float* __restrict__ out, int64_t ldo, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;  // neighbour rows in flight per lane group (q and v each)
  const LaneCoords lc = lane_coords<VEC>(L);
  const int lane = lc.lane, NG = lc.NG, g = lc.g, ch = lc.ch, wpb = lc.wpb, F = lc.F;
  const bool active = ch < L.C;  // H = 1: the group is the head, t / LPH = 0

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float ki[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ki[i] = acc[i] = 0.f;
    if (active) load_vec<VEC>(ki, kx + (int64_t)row * ldk + ch);

    walk_slots<U, 2, VEC>(
        col, start, end, lane, NG, g, active,
        [&](float (&f)[2][VEC], int src, int) {
          load_vec<VEC>(f[0], qx + (int64_t)src * ldq + ch);
          load_vec<VEC>(f[1], vx + (int64_t)src * ldv + ch);
        },
        [&](const float (&f)[2][VEC], int, bool) {  // a slot past the row's end holds v = 0: its (finite) gate adds nothing
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(gate(ki[i] + f[0][i]), f[1][i], acc[i]);
        });
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);  // rows without slots: zeros, written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward. With d_p = s_p (1 - s_p) (the gate's derivative, from the recomputed gate):
//   g_k[i,:] = gout[i,:] (.) sum_p v_j (.) d_p
//   g_q[j,:] = v[j,:] (.) sum_p gout_i (.) d_p,    g_v[j,:] = sum_p s_p (.) gout_i
//
// Target side, over the forward CSR (row = target i): the same gather as the forward. The row's gout factor is applied
// to whatever the wave stores, a chunk's partial sum included, so the combine kernel only adds.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
resgated_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ kx,
                        int64_t ldk, const float* __restrict__ qx, int64_t ldq, const float* __restrict__ vx,
                        int64_t ldv, const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_k,
                        int64_t ldgk, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const LaneCoords lc = lane_coords<VEC>(L);
  const int lane = lc.lane, NG = lc.NG, g = lc.g, ch = lc.ch, wpb = lc.wpb, F = lc.F;
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float ki[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) ki[i] = acc[i] = 0.f;
    if (active) load_vec<VEC>(ki, kx + (int64_t)row * ldk + ch);

    walk_slots<U, 2, VEC>(
        col, start, end, lane, NG, g, active,
        [&](float (&f)[2][VEC], int src, int) {
          load_vec<VEC>(f[0], qx + (int64_t)src * ldq + ch);
          load_vec<VEC>(f[1], vx + (int64_t)src * ldv + ch);
        },
        [&](const float (&f)[2][VEC], int, bool) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float s = gate(ki[i] + f[0][i]);
            acc[i] = fmaf(s * (1.f - s), f[1][i], acc[i]);
          }
        });
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      float go[VEC];
      load_vec<VEC>(go, gout + (int64_t)row * ldg + ch);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] *= go[i];
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(g_k + (int64_t)row * ldgk + ch, acc);  // rows without slots: zeros, written
    }
  }
}

// Source side, over the TRANSPOSED CSR (row = source j, col_t[p] = target i): the source's own q and v rows stay in
// registers; the k and gout rows of the target are gathered per slot. A chunk's record is (g_q | g_v). A source without
// out-edges stores zeros.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
resgated_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const float* __restrict__ kx,
                        int64_t ldk, const float* __restrict__ qx, int64_t ldq, const float* __restrict__ vx,
                        int64_t ldv, const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_q,
                        int64_t ldgq, float* __restrict__ g_v, int64_t ldgv, int N, const GatLayout L,
                        const AttnSplit sp) {
  constexpr int U = 4;
  const LaneCoords lc = lane_coords<VEC>(L);
  const int lane = lc.lane, NG = lc.NG, g = lc.g, ch = lc.ch, wpb = lc.wpb, F = lc.F;
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    float qj[VEC], aq[VEC], av[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) qj[i] = aq[i] = av[i] = 0.f;
    if (active) load_vec<VEC>(qj, qx + (int64_t)row * ldq + ch);

    walk_slots<U, 2, VEC>(
        col_t, start, end, lane, NG, g, active,
        [&](float (&f)[2][VEC], int tgt, int) {
          load_vec<VEC>(f[0], kx + (int64_t)tgt * ldk + ch);
          load_vec<VEC>(f[1], gout + (int64_t)tgt * ldg + ch);
        },
        [&](const float (&f)[2][VEC], int, bool) {  // a slot past the row's end holds gout = 0
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float s = gate(f[0][i] + qj[i]);
            aq[i] = fmaf(s * (1.f - s), f[1][i], aq[i]);
            av[i] = fmaf(s, f[1][i], av[i]);
          }
        });
    groups_sum<VEC>(aq, L.G);
    groups_sum<VEC>(av, L.G);
    if (g == 0 && active) {
      float vj[VEC];
      load_vec<VEC>(vj, vx + (int64_t)row * ldv + ch);
#pragma unroll
      for (int i = 0; i < VEC; ++i) aq[i] *= vj[i];
      if constexpr (CHUNK) {
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + ch, aq);
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + F + ch, av);
      } else {
        store_vec<VEC>(g_q + (int64_t)row * ldgq + ch, aq);
        store_vec<VEC>(g_v + (int64_t)row * ldgv + ch, av);
      }
    }
  }
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_resgated_supported(int C) { return head_width_supported(C); }

extern "C" int rgbx_resgated_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* k, int64_t ldk,
                                     const float* q, int64_t ldq, const float* v, int64_t ldv, float* out, int64_t ldo,
                                     int64_t N, int C, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "resgated_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !k || !q || !v || !out) return fail(RGBX_E_ARG, "resgated_fwd: null pointer");
  if (ldk < C || ldq < C || ldv < C || ldo < C) return fail(RGBX_E_ARG, "resgated_fwd: leading dimension < C");
  if (!aligned_to({k, q, v, out}, 4))
    return fail(RGBX_E_ALIGN, "resgated_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "resgated_fwd")) return rc;
  const int vec = pick_vec(C, {k, q, v, out, sd.pacc}, {ldk, ldq, ldv, ldo});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "resgated_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(resgated_fwd_kernel, N, rowptr, col, k, ldk, q, ldq, v, ldv, out, ldo, n_items, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(out, ldo, C, 0);  // a plain sum: the chunk partials added in chunk order
  RGBX_CHECK_LAUNCH("resgated_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_resgated_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* k, int64_t ldk,
                                         const float* q, int64_t ldq, const float* v, int64_t ldv, const float* gout,
                                         int64_t ldg, float* g_k, int64_t ldgk, int64_t N, int C,
                                         const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "resgated_bwd_dst")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !k || !q || !v || !gout || !g_k) return fail(RGBX_E_ARG, "resgated_bwd_dst: null pointer");
  if (ldk < C || ldq < C || ldv < C || ldg < C || ldgk < C)
    return fail(RGBX_E_ARG, "resgated_bwd_dst: leading dimension < C");
  if (!aligned_to({k, q, v, gout, g_k}, 4))
    return fail(RGBX_E_ALIGN, "resgated_bwd_dst: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "resgated_bwd_dst")) return rc;
  const int vec = pick_vec(C, {k, q, v, gout, g_k, sd.pacc}, {ldk, ldq, ldv, ldg, ldgk});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "resgated_bwd_dst")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(resgated_bwd_dst_kernel, N, rowptr, col, k, ldk, q, ldq, v, ldv, gout, ldg, g_k, ldgk, n_items, L,
                 sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_k, ldgk, C, 0);
  RGBX_CHECK_LAUNCH("resgated_bwd_dst_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_resgated_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* k, int64_t ldk,
                                         const float* q, int64_t ldq, const float* v, int64_t ldv, const float* gout,
                                         int64_t ldg, float* g_q, int64_t ldgq, float* g_v, int64_t ldgv, int64_t N,
                                         int C, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "resgated_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !k || !q || !v || !gout || !g_q || !g_v)
    return fail(RGBX_E_ARG, "resgated_bwd_src: null pointer");
  if (ldk < C || ldq < C || ldv < C || ldg < C || ldgq < C || ldgv < C)
    return fail(RGBX_E_ARG, "resgated_bwd_src: leading dimension < C");
  if (!aligned_to({k, q, v, gout, g_q, g_v}, 4))
    return fail(RGBX_E_ALIGN, "resgated_bwd_src: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "resgated_bwd_src")) return rc;
  const int vec = pick_vec(C, {k, q, v, gout, g_q, g_v, sd.pacc}, {ldk, ldq, ldv, ldg, ldgq, ldgv});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "resgated_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(resgated_bwd_src_kernel, N, rowptr_t, col_t, k, ldk, q, ldq, v, ldv, gout, ldg, g_q, ldgq, g_v,
                 ldgv, n_items, L, sd);
  if (sd.threshold > 0) {  // a chunk's record is (g_q | g_v)
    RGBX_ATTN_BWD_COMBINE(g_q, ldgq, 2 * (int64_t)C, 0);
    RGBX_ATTN_BWD_COMBINE(g_v, ldgv, 2 * (int64_t)C, C);
  }
  RGBX_CHECK_LAUNCH("resgated_bwd_src_kernel");
  return RGBX_OK;
}
