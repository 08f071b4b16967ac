// Softmax aggregation (DeeperGCN's learnable aggregator): a softmax PER CHANNEL over the in-edges at a trained
// temperature, fused with the aggregation, and its backward, for gfx950. Stands in for SoftmaxAggregation /
// GENConv(aggr="softmax") [PyG] (Li et al., "DeeperGCN: All You Need to Train Deeper GCNs").
//
// For an edge j -> i in forward CSR slot p, messages m [N, C] and a temperature t (device memory: one float, or one per
// channel, told apart by a stride of 0 or 1):
//   z_p[c]    = t[c] m[j,c]
//   alpha_p[c] = exp(z_p[c] - lse[i,c]),   lse[i,c] = log sum_p exp(z_p[c])
//   out[i,c]  = sum_p alpha_p[c] m[j,c]
// t = 0 is the mean, t -> inf the maximum, t < 0 a soft minimum: the running maximum is taken of z, not of m.
//
// The lane layout is attn_common.h's with H = 1 (a row fragment of VEC channels per lane, G lanes per neighbour row,
// 64 / G rows per wave-instruction). Unlike the attention families the softmax state (max, den, acc) is per lane
// ELEMENT: nothing crosses lanes inside a slot. The edges are taken as given, so a row may have no slot at all: it
// stores exact zeros (and lse = 0).
//
// Nothing per edge is written. The backward recomputes alpha = exp(t m_j - lse_i) <= 1 from the saved lse. No float
// atomics; every sum runs in a fixed order (slots of a lane group in slot order, lane groups by a butterfly, hub-row
// chunks in chunk order, g_t's records in record order).
#include <cmath>

#include "edge_common.h"

namespace rgbx {
namespace {

// The temperature of this lane's channels; `ts` = 0: one scalar for all of them.
template <int VEC>
__device__ __forceinline__ void load_temp(float (&tc)[VEC], const float* __restrict__ t, int ts, int ch, bool active) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) tc[i] = active ? t[(int64_t)(ch + i) * ts] : 0.f;
}

// The per-element online-softmax state (m2, l2, a2) merged into (mx, den, acc). Two states without a slot (max =
// kNegBig, den = 0) merge to one without a slot: exp(0) * 0 + exp(0) * 0.
__device__ __forceinline__ void state_merge(float& mx, float& den, float& acc, float m2, float l2, float a2) {
  const float mn = fmaxf(mx, m2);
  const float s1 = expf(mx - mn), s2 = expf(m2 - mn);
  den = den * s1 + l2 * s2;
  acc = acc * s1 + a2 * s2;
  mx = mn;
}

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR: U rows m_j in flight per lane group. The state is rescaled ONCE per batch of U
// slots (the batch maximum first), so a slot costs one expf per element and a batch one more; a per-slot online update
// would cost two per slot. CHUNK: the wave owns a chunk of a hub row and leaves its state (acc | max | den).
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
softmax_aggr_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ mx_in,
                        int64_t ldm, const float* __restrict__ temp, int ts, float* __restrict__ out, int64_t ldo,
                        float* __restrict__ lse, int64_t ldl, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;  // H = 1: the group is the head
  float tc[VEC];
  load_temp<VEC>(tc, temp, ts, ch, active);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float mx[VEC], den[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mx[i] = kNegBig;
      den[i] = acc[i] = 0.f;
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float mv[U][VEC];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
          ok[u] = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) mv[u][i] = 0.f;
          if (ok[u]) load_vec<VEC>(mv[u], mx_in + (int64_t)src * ldm + ch);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float z[U];
          float mn = mx[i];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            z[u] = tc[i] * mv[u][i];
            mn = fmaxf(mn, ok[u] ? z[u] : kNegBig);
          }
          const float s = expf(mx[i] - mn);  // a batch without a slot: exp(0) = 1
          float d = den[i] * s, a = acc[i] * s;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float e = ok[u] ? expf(z[u] - mn) : 0.f;
            d += e;
            a = fmaf(e, mv[u][i], a);
          }
          mx[i] = mn;
          den[i] = d;
          acc[i] = a;
        }
      }
    }
    // the lane groups' states, merged in a fixed order; group 0 ends with the row's (or the chunk's)
    for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float m2 = __shfl_xor(mx[i], off);
        const float l2 = __shfl_xor(den[i], off);
        const float a2 = __shfl_xor(acc[i], off);
        state_merge(mx[i], den[i], acc[i], m2, l2, a2);
      }
    }
    if (g == 0 && active) {
      if constexpr (CHUNK) {
        float* rec = sp.pacc + (int64_t)item * 3 * F + ch;
        store_vec<VEC>(rec, acc);
        store_vec<VEC>(rec + F, mx);
        store_vec<VEC>(rec + 2 * F, den);
      } else {
        float o[VEC], ls[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {  // a row without slots: zeros and a finite lse, written
          o[i] = den[i] > 0.f ? acc[i] / den[i] : 0.f;
          ls[i] = den[i] > 0.f ? mx[i] + logf(den[i]) : 0.f;
        }
        store_vec<VEC>(out + (int64_t)row * ldo + ch, o);
        if (lse) store_vec<VEC>(lse + (int64_t)row * ldl + ch, ls);
      }
    }
  }
}

// One wave per hub row: the chunk states (acc | max | den) merged in chunk order, normalised, stored.
template <int VEC>
__global__ void __launch_bounds__(256)
softmax_aggr_fwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                                float* __restrict__ out, int64_t ldo, float* __restrict__ lse, int64_t ldl,
                                const GatLayout L, const AttnSplit sp) {
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    if (!(g == 0 && ch < L.C)) continue;
    float mx[VEC], den[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mx[i] = kNegBig;
      den[i] = acc[i] = 0.f;
    }
    for (int c = c0; c < c1; ++c) {
      const float* rec = sp.pacc + (int64_t)c * 3 * F + ch;
      float a2[VEC], m2[VEC], l2[VEC];
      load_vec<VEC>(a2, rec);
      load_vec<VEC>(m2, rec + F);
      load_vec<VEC>(l2, rec + 2 * F);
#pragma unroll
      for (int i = 0; i < VEC; ++i) state_merge(mx[i], den[i], acc[i], m2[i], l2[i], a2[i]);
    }
    float o[VEC], ls[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      o[i] = den[i] > 0.f ? acc[i] / den[i] : 0.f;
      ls[i] = den[i] > 0.f ? mx[i] + logf(den[i]) : 0.f;
    }
    store_vec<VEC>(out + (int64_t)row * ldo + ch, o);
    if (lse) store_vec<VEC>(lse + (int64_t)row * ldl + ch, ls);
  }
}

// ------------------------------------------------------------------------------------------
// Backward over the TRANSPOSED CSR (row = source j, col_t[p] = target i). With d = m_j - out_i and
// alpha = exp(t m_j - lse_i):
//   g_m[j,c] = sum_p alpha g_i (1 + t d),     g_t[c] = sum_edges alpha g_i d^2
// (the squared form of g_t: sum_p alpha_p (m_p - out) = 0 per target, and d^2 does not cancel a large mean). The
// source's own row stays in registers; g_i, out_i and lse_i are gathered per slot through their own pointers.
// GT: a lane keeps its channels' share of g_t over all the rows of its wave; the waves of a workgroup are added in
// wave order through LDS and stored as record blockIdx.x of gt_part [gridDim.x, C]. A source without out-edges stores
// zeros.
template <int VEC, bool CHUNK, bool GT>
__global__ void __launch_bounds__(256)
softmax_aggr_bwd_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const float* __restrict__ mx_in,
                        int64_t ldm, const float* __restrict__ temp, int ts, const float* __restrict__ out, int64_t ldo,
                        const float* __restrict__ lse, int64_t ldl, const float* __restrict__ gout, int64_t ldg,
                        float* __restrict__ g_m, int64_t ldgm, float* __restrict__ gt_part, int N, const GatLayout L,
                        const AttnSplit sp) {
  constexpr int U = 3;  // three rows per slot: 9 fragments in flight per lane
  __shared__ float red[4][kWave * 4];
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const int wave = threadIdx.x >> 6;
  const bool active = ch < L.C;
  float tc[VEC], gt[VEC];
  load_temp<VEC>(tc, temp, ts, ch, active);
#pragma unroll
  for (int i = 0; i < VEC; ++i) gt[i] = 0.f;

  for (int item = blockIdx.x * wpb + wave; item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    float mj[VEC], zj[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) mj[i] = acc[i] = 0.f;
    if (active) load_vec<VEC>(mj, mx_in + (int64_t)row * ldm + ch);
#pragma unroll
    for (int i = 0; i < VEC; ++i) zj[i] = tc[i] * mj[i];

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col_t[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float go[U][VEC], oi[U][VEC], li[U][VEC];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int tgt = __shfl(mycol, idx & 63);
          ok[u] = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) go[u][i] = oi[u][i] = li[u][i] = 0.f;
          if (ok[u]) {
            load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + ch);
            load_vec<VEC>(oi[u], out + (int64_t)tgt * ldo + ch);
            load_vec<VEC>(li[u], lse + (int64_t)tgt * ldl + ch);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            // a slot past the row's end: alpha = 0 by the select (exp(z_j - 0) may be anything)
            const float w = ok[u] ? expf(zj[i] - li[u][i]) * go[u][i] : 0.f;
            const float d = mj[i] - oi[u][i];
            acc[i] = fmaf(w, fmaf(tc[i], d, 1.f), acc[i]);
            if constexpr (GT) gt[i] = fmaf(w * d, d, gt[i]);
          }
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(g_m + (int64_t)row * ldgm + ch, acc);  // sources without slots: zeros, written
    }
  }

  if constexpr (GT) {  // this workgroup's g_t record: lane groups, then waves, in a fixed order
    groups_sum<VEC>(gt, L.G);
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) red[wave][t * VEC + i] = gt[i];
    }
    __syncthreads();
    if (wave == 0 && g == 0 && active) {
      float r[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        r[i] = red[0][t * VEC + i];
        for (int w = 1; w < wpb; ++w) r[i] += red[w][t * VEC + i];
      }
      store_vec<VEC>(gt_part + (int64_t)blockIdx.x * F + ch, r);
    }
  }
}

// g_t[c] = sum of the per-workgroup records part[b, c], b = 0 .. n_rec - 1. A block owns 16 columns; its 16 x 16
// threads add the records b = r, r + 16, ... of a column, then the 16 sums in a fixed tree (gatv2.hip's scheme).
__global__ void __launch_bounds__(256)
softmax_aggr_gt_reduce_kernel(const float* __restrict__ part, int64_t n_rec, int C, float* __restrict__ g_t) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int f = blockIdx.x * 16 + c;
  float s = 0.f;
  if (f < C)
    for (int64_t b = r; b < n_rec; b += 16) s += part[b * C + f];
  sh[r][c] = s;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (r < w) sh[r][c] += sh[r + w][c];
    __syncthreads();
  }
  if (r == 0 && f < C) g_t[f] = sh[0][c];
}

// With g_t the backward leaves one record per workgroup, so its grid is capped and the waves stride over the rows.
int gt_grid(int64_t N) { return capped_grid(N, 4); }

int64_t gt_records(int64_t N, const rgbx_row_split_t* split) {
  return gt_grid(N) + (split && split->threshold > 0 && split->n_chunks > 0 ? gt_grid(split->n_chunks) : 0);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_softmax_aggr_supported(int C) { return head_width_supported(C); }

extern "C" int rgbx_softmax_aggr_gt_partial_floats(int64_t N, int C, const rgbx_row_split_t* split, int64_t* count) {
  if (!count) return fail(RGBX_E_ARG, "softmax_aggr_gt_partial_floats: null pointer");
  if (int rc = check_common(N, 1, C, "softmax_aggr_gt_partial_floats")) return rc;
  *count = gt_records(N, split) * (int64_t)C;
  return RGBX_OK;
}

extern "C" int rgbx_softmax_aggr_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* m, int64_t ldm,
                                         const float* t, int t_stride, float* out, int64_t ldo, float* lse, int64_t ldl,
                                         int64_t N, int C, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "softmax_aggr_fwd")) return rc;
  if (t_stride != 0 && t_stride != 1) return fail(RGBX_E_ARG, "softmax_aggr_fwd: t_stride must be 0 or 1");
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !m || !t || !out) return fail(RGBX_E_ARG, "softmax_aggr_fwd: null pointer");
  if (ldm < C || ldo < C || (lse && ldl < C)) return fail(RGBX_E_ARG, "softmax_aggr_fwd: leading dimension < C");
  if (!aligned_to({m, t, out, lse}, 4))
    return fail(RGBX_E_ALIGN, "softmax_aggr_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "softmax_aggr_fwd")) return rc;
  const int vec = lse ? pick_vec(C, {m, out, lse, sd.pacc}, {ldm, ldo, ldl}) : pick_vec(C, {m, out, sd.pacc}, {ldm, ldo});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "softmax_aggr_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(softmax_aggr_fwd_kernel, N, rowptr, col, m, ldm, t, t_stride, out, ldo, lse, ldl, n_items, L, sd);
  if (sd.threshold > 0)
    RGBX_VEC_SWITCH(vec, softmax_aggr_fwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(
                             split->n_long, split->long_row, split->long_chunk_ptr, out, ldo, lse, ldl, L, sd));
  RGBX_CHECK_LAUNCH("softmax_aggr_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_softmax_aggr_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* m, int64_t ldm,
                                         const float* t, int t_stride, const float* out, int64_t ldo, const float* lse,
                                         int64_t ldl, const float* gout, int64_t ldg, float* g_m, int64_t ldgm,
                                         float* g_t, float* gt_partial, int64_t n_gt_partial, int64_t N, int C,
                                         const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, "softmax_aggr_bwd")) return rc;
  if (t_stride != 0 && t_stride != 1) return fail(RGBX_E_ARG, "softmax_aggr_bwd: t_stride must be 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    if (g_t) RGBX_HIP(hipMemsetAsync(g_t, 0, (size_t)C * sizeof(float), s));
    return RGBX_OK;
  }
  if (!rowptr_t || !col_t || !m || !t || !out || !lse || !gout || !g_m || (g_t && !gt_partial))
    return fail(RGBX_E_ARG, "softmax_aggr_bwd: null pointer");
  if (ldm < C || ldo < C || ldl < C || ldg < C || ldgm < C)
    return fail(RGBX_E_ARG, "softmax_aggr_bwd: leading dimension < C");
  if (!aligned_to({m, t, out, lse, gout, g_m, g_t, gt_partial}, 4))
    return fail(RGBX_E_ALIGN, "softmax_aggr_bwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "softmax_aggr_bwd")) return rc;
  const int64_t n_rec = gt_records(N, split);
  if (g_t && n_gt_partial < n_rec * C)
    return fail(RGBX_E_WS, "softmax_aggr_bwd: %lld partial floats < %lld", (long long)n_gt_partial,
                (long long)(n_rec * C));
  const int vec = g_t ? pick_vec(C, {m, out, lse, gout, g_m, gt_partial, sd.pacc}, {ldm, ldo, ldl, ldg, ldgm})
                      : pick_vec(C, {m, out, lse, gout, g_m, sd.pacc}, {ldm, ldo, ldl, ldg, ldgm});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "softmax_aggr_bwd")) return rc;
  if (g_t) {  // one g_t record per workgroup: the capped grid, the chunk pass's records behind the row pass's
    const int grid = gt_grid(N);
    RGBX_VEC_SWITCH(vec, RGBX_EDGE_LAUNCH(gt_grid, N, (softmax_aggr_bwd_kernel<V, false, true>),
                                          (softmax_aggr_bwd_kernel<V, true, true>), rowptr_t, col_t, m, ldm, t,
                                          t_stride, out, ldo, lse, ldl, gout, ldg, g_m, ldgm,
                                          gt_partial + (chunk_pass ? (int64_t)grid * C : 0), n_items, L, sd));
  } else {
    RGBX_EDGE_ROWS_X(softmax_aggr_bwd_kernel, (false), N, rowptr_t, col_t, m, ldm, t, t_stride, out, ldo, lse, ldl,
                     gout, ldg, g_m, ldgm, nullptr, n_items, L, sd);
  }
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_m, ldgm, C, 0);  // the chunk partials added in chunk order
  RGBX_CHECK_LAUNCH("softmax_aggr_bwd_kernel");
  if (g_t) {
    softmax_aggr_gt_reduce_kernel<<<(int)cdiv(C, 16), 256, 0, s>>>(gt_partial, n_rec, C, g_t);
    RGBX_CHECK_LAUNCH("softmax_aggr_gt_reduce_kernel");
  }
  return RGBX_OK;
}
