// GINEConv (GIN with edge features): fused message relu(x_j + e_ji) + sum aggregation + root term, and its backward,
// for gfx950. Stands in for GINEConv.forward / message [PyG] (Hu et al., "Strategies for Pre-training Graph Neural
// Networks"; the OGB baselines' layer).
//
// For an edge j -> i in forward CSR slot p, with x [N, C] and e [nnz, C] (one row PER SLOT, in forward slot order; each
// operand its own pointer and leading dimension):
//   out[i,:] = (1 + eps) * x[i,:] + sum_p relu(x[j,:] + e[p,:])
// This is the one family here whose per-slot message depends on a per-slot row. The e rows of a target are consecutive,
// so the forward and the edge pass read them as a stream beside the gather of x; only the source pass, which walks the
// transposed CSR, gathers them (through t2f, the forward slot of every transposed slot). The lane layout is
// attn_common.h's with H = 1 (a row fragment of VEC channels per lane, G lanes per neighbour row, 64 / G rows per
// wave-instruction), and a lane never talks to its neighbours inside a slot. The edges are taken as given, so a row may
// have no slot at all: it stores the root term alone.
//
// Nothing per edge is saved and no record passes between the kernels: all three recompute the mask from the same single
// float32 add x[j,:] + e[p,:] (> 0; relu'(0) = 0). eps is read from DEVICE memory, so a captured launch follows a
// parameter that an optimizer moves. No float atomics; every sum runs in a fixed order (slots of a lane group in slot
// order, lane groups by a butterfly, hub-row chunks in chunk order, the root term on the row's first chunk).
#include "edge_common.h"

namespace rgbx {
namespace {

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR: per slot the x row of the source is gathered and the slot's e row streamed (U
// slots in flight per lane group). CHUNK: the wave owns a chunk of a hub row and leaves its partial sum; the chunk that
// starts the row carries the root term, so the combine kernel only adds.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gine_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ x, int64_t ldx,
                const float* __restrict__ e, int64_t lde, const float* __restrict__ eps, float* __restrict__ out,
                int64_t ldo, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;  // slots in flight per lane group (an x row and an e row each)
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;  // H = 1: the group is the head, t / LPH = 0

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float xv[U][VEC], ev[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) xv[u][i] = ev[u][i] = 0.f;
          if (active && idx < n) {
            load_vec<VEC>(xv[u], x + (int64_t)src * ldx + ch);
            load_vec<VEC>(ev[u], e + (int64_t)(base + idx) * lde + ch);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // a slot past the row's end holds x = e = 0: relu(0) adds nothing
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float s = xv[u][i] + ev[u][i];
            acc[i] += s > 0.f ? s : 0.f;
          }
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      bool root = eps != nullptr;
      if constexpr (CHUNK) root = root && start == rowptr[row];
      if (root) {
        const float a = 1.f + eps[0];
        float xi[VEC];
        load_vec<VEC>(xi, x + (int64_t)row * ldx + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(a, xi[i], acc[i]);
      }
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);  // rows without slots: the root term, written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward. With the mask m_p = [x[j,:] + e[p,:] > 0] (recomputed from the forward's own add):
//   g_e[p,:] = gout[i,:] (.) m_p
//   g_x[j,:] = (1 + eps) gout[j,:] + sum over the out-edges (j -> i, slot p) of gout[i,:] (.) m_p
//
// Edge pass, over the forward CSR (row = target i): the row's gout fragment stays in registers; per slot the x row of
// the source is gathered, the e row streamed and the g_e row stored. No sum is formed: every stored value is a copy of
// gout or an exact zero. The chunk items only balance the hub rows; there is nothing to combine.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gine_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ x,
                     int64_t ldx, const float* __restrict__ e, int64_t lde, const float* __restrict__ gout,
                     int64_t ldg, float* __restrict__ g_e, int64_t ldge, int N, const GatLayout L,
                     const AttnSplit sp) {
  constexpr int U = 4;
  const LaneCoords lc = lane_coords<VEC>(L);
  const int lane = lc.lane, NG = lc.NG, g = lc.g, ch = lc.ch, wpb = lc.wpb;
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    if (start == end) continue;
    float go[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) go[i] = 0.f;
    if (active) load_vec<VEC>(go, gout + (int64_t)row * ldg + ch);

    walk_slots<U, 2, VEC>(
        col, start, end, lane, NG, g, active,
        [&](float (&f)[2][VEC], int src, int slot) {
          load_vec<VEC>(f[0], x + (int64_t)src * ldx + ch);
          load_vec<VEC>(f[1], e + (int64_t)slot * lde + ch);
        },
        [&](const float (&f)[2][VEC], int slot, bool ok) {
          if (ok) {
            float ge[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) ge[i] = f[0][i] + f[1][i] > 0.f ? go[i] : 0.f;
            store_vec<VEC>(g_e + (int64_t)slot * ldge + ch, ge);
          }
        });
  }
}

// Source pass, over the TRANSPOSED CSR (row = source j, col_t[q] = target i, t2f[q] = the edge's forward slot): the
// source's own x row stays in registers; the gout row of the target and the e row of the edge are gathered per slot. A
// source without out-edges stores the root term alone.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gine_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ t2f,
                    const float* __restrict__ x, int64_t ldx, const float* __restrict__ e, int64_t lde,
                    const float* __restrict__ gout, int64_t ldg, const float* __restrict__ eps,
                    float* __restrict__ g_x, int64_t ldgx, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    float xj[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) xj[i] = acc[i] = 0.f;
    if (active) load_vec<VEC>(xj, x + (int64_t)row * ldx + ch);

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col_t[base + lane] : 0;
      const int myslot = lane < n ? t2f[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float go[U][VEC], ev[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int tgt = __shfl(mycol, idx & 63);
          const int slot = __shfl(myslot, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) go[u][i] = ev[u][i] = 0.f;
          if (active && idx < n) {
            load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + ch);
            load_vec<VEC>(ev[u], e + (int64_t)slot * lde + ch);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // a slot past the row's end holds gout = 0
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += xj[i] + ev[u][i] > 0.f ? go[u][i] : 0.f;
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      bool root = eps != nullptr;
      if constexpr (CHUNK) root = root && start == rowptr_t[row];
      if (root) {
        const float a = 1.f + eps[0];
        float gj[VEC];
        load_vec<VEC>(gj, gout + (int64_t)row * ldg + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(a, gj[i], acc[i]);
      }
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(g_x + (int64_t)row * ldgx + ch, acc);
    }
  }
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gine_supported(int C) { return head_width_supported(C); }

extern "C" int rgbx_gine_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, const float* e,
                                 int64_t lde, const float* eps, float* out, int64_t ldo, int64_t N, int C,
                                 const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "gine_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !x || !e || !out) return fail(RGBX_E_ARG, "gine_fwd: null pointer");
  if (ldx < C || lde < C || ldo < C) return fail(RGBX_E_ARG, "gine_fwd: leading dimension < C");
  if (!aligned_to({x, e, eps, out}, 4)) return fail(RGBX_E_ALIGN, "gine_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "gine_fwd")) return rc;
  const int vec = pick_vec(C, {x, e, out, sd.pacc}, {ldx, lde, ldo});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "gine_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(gine_fwd_kernel, N, rowptr, col, x, ldx, e, lde, eps, out, ldo, n_items, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(out, ldo, C, 0);  // a plain sum: the chunk partials added in chunk order
  RGBX_CHECK_LAUNCH("gine_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gine_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                                      const float* e, int64_t lde, const float* gout, int64_t ldg, float* g_e,
                                      int64_t ldge, int64_t N, int C, const rgbx_row_split_t* split,
                                      rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "gine_bwd_edge")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !x || !e || !gout || !g_e) return fail(RGBX_E_ARG, "gine_bwd_edge: null pointer");
  if (ldx < C || lde < C || ldg < C || ldge < C) return fail(RGBX_E_ARG, "gine_bwd_edge: leading dimension < C");
  if (!aligned_to({x, e, gout, g_e}, 4))
    return fail(RGBX_E_ALIGN, "gine_bwd_edge: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "gine_bwd_edge")) return rc;
  const int vec = pick_vec(C, {x, e, gout, g_e}, {ldx, lde, ldg, ldge});  // no chunk record is written or read
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "gine_bwd_edge")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(gine_bwd_edge_kernel, N, rowptr, col, x, ldx, e, lde, gout, ldg, g_e, ldge, n_items, L, sd);
  RGBX_CHECK_LAUNCH("gine_bwd_edge_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gine_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* x,
                                     int64_t ldx, const float* e, int64_t lde, const float* gout, int64_t ldg,
                                     const float* eps, float* g_x, int64_t ldgx, int64_t N, int C,
                                     const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "gine_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !t2f || !x || !e || !gout || !g_x) return fail(RGBX_E_ARG, "gine_bwd_src: null pointer");
  if (ldx < C || lde < C || ldg < C || ldgx < C) return fail(RGBX_E_ARG, "gine_bwd_src: leading dimension < C");
  if (!aligned_to({x, e, gout, eps, g_x}, 4))
    return fail(RGBX_E_ALIGN, "gine_bwd_src: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "gine_bwd_src")) return rc;
  const int vec = pick_vec(C, {x, e, gout, g_x, sd.pacc}, {ldx, lde, ldg, ldgx});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "gine_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(gine_bwd_src_kernel, N, rowptr_t, col_t, t2f, x, ldx, e, lde, gout, ldg, eps, g_x, ldgx, n_items, L,
                 sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_x, ldgx, C, 0);
  RGBX_CHECK_LAUNCH("gine_bwd_src_kernel");
  return RGBX_OK;
}
