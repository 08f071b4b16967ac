// RGCNConv with a basis decomposition (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional
// Networks"): the per-(target, relation) mean weights and the fused mix of the B basis rows of a source, with its
// backward, for gfx950. Stands in for RGCNConv.forward's loop over the relations [PyG].
//
// Every edge j -> i carries a category, its relation r = etype[p] (p = the edge's forward CSR slot). With the basis
// products h = x @ [V_0 | ... | V_{B-1}] viewed as [N, B, C] and the trained table comp [R, B]:
//   a[p, b]  = w[p] * comp[etype[p], b]
//   out[i,:] = y0[i,:] + sum_p sum_b a[p, b] * h[col[p], b, :]
// where w[p] = 1 / #{slots of p's row with p's relation} gives the mean per (target, relation) and w = 1 the sum. The
// coefficient is neither a softmax nor saved anywhere: each slot reads its relation and weight and fetches its B
// coefficients from `comp` in DEVICE memory (a few hundred floats, cache-resident), so a captured launch follows the
// table an optimizer moves. The lane layout is attn_common.h's with H = B heads of C channels (a head on LPH lanes of
// VEC channels, HPC heads side by side in a group of G lanes, NG = 64 / G neighbour rows per wave-instruction); the
// output is ONE head wide, so the forward also sums over the heads of a group and over the head chunks.
//
// Nothing per edge passes between forward and backward. No float atomics, no scratch, no LDS; every sum runs in a
// fixed order: the slots of a lane group in slot order, the lane groups and then the heads of a group by a butterfly,
// the head chunks in ascending order, the hub-row chunks in chunk order (y0 rides on a row's first chunk).
#include "edge_common.h"

namespace rgbx {
namespace {

constexpr int kMaxBases = 64;  // a wave of one-lane heads; beyond it the caller composes W_r and runs the select form

// ------------------------------------------------------------------------------------------
// Slot weights of the mean per (target, relation): w[p] = 1 / #{p' in the row of p : etype[p'] == etype[p]}. Integers
// only until the one division. A wave owns a row (or a chunk of a hub row) and compares every tile of 64 of its slots
// with every tile of the WHOLE row, so no [N, R] table exists and R does not enter the cost: 64 lane reads per pair of
// tiles. A chunk item walks its own slots against all of its row's, which is why hub rows need no combine.
template <bool CHUNK>
__global__ void __launch_bounds__(256)
rgcn_slot_norm_kernel(const int* __restrict__ rowptr, const int* __restrict__ etype, float* __restrict__ w, int N,
                      const AttnSplit sp) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    int rs = start, re = end;
    if constexpr (CHUNK) {
      rs = __builtin_amdgcn_readfirstlane(rowptr[row]);
      re = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    }
    for (int a = start; a < end; a += kWave) {
      const int p = a + lane;
      const int ty = p < end ? etype[p] : -1;
      int cnt = 0;
      for (int b = rs; b < re; b += kWave) {
        const int n = min(kWave, re - b);
        const int tq = lane < n ? etype[b + lane] : -2;
        for (int k = 0; k < n; ++k) cnt += __shfl(tq, k) == ty ? 1 : 0;
      }
      if (p < end) w[p] = 1.0f / (float)cnt;  // cnt >= 1: the slot counts itself
    }
  }
}

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR. Per head chunk a lane accumulates coef * h over its slots (U slots in flight per
// lane group); the butterfly then adds the lane groups and the heads of a group, and the head chunks are added in
// ascending order. CHUNK: the wave owns a chunk of a hub row and leaves a partial row of C floats; the chunk that
// starts the row carries y0, so the combine kernel only adds.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
rgcn_mix_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ etype,
                    const float* __restrict__ w, const float* __restrict__ comp, const float* __restrict__ h,
                    int64_t ldh, const float* __restrict__ y0, int64_t ldy, float* __restrict__ out, int64_t ldo,
                    int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float tot[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) tot[i] = 0.f;

    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        const int mytype = lane < n ? etype[base + lane] : 0;
        const float myw = lane < n ? w[base + lane] : 0.f;
        for (int k = 0; k < n; k += NG * U) {
          float hv[U][VEC], coef[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            const int ty = __shfl(mytype, idx & 63);
            const float ws = __shfl(myw, idx & 63);
            coef[u] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) hv[u][i] = 0.f;
            if (active && idx < n) {
              load_vec<VEC>(hv[u], h + (int64_t)src * ldh + cofs);
              coef[u] = ws * comp[(int64_t)ty * L.H + head];
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {  // a slot past the row's end, a lane past the heads: coef = 0, h = 0
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(coef[u], hv[u][i], acc[i]);
          }
        }
      }
      // lane groups, then the heads of a group: the lanes that hold channel ch differ in the bits from LPH up
      for (int off = 32; off >= L.LPH; off >>= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) tot[i] += acc[i];
    }

    if (lane < L.LPH && ch < L.C) {  // group 0, head lane 0
      bool root = y0 != nullptr;
      if constexpr (CHUNK) root = root && start == rowptr[row];
      if (root) {
        float yv[VEC];
        load_vec<VEC>(yv, y0 + (int64_t)row * ldy + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) tot[i] += yv[i];
      }
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * L.C + ch, tot);
      else store_vec<VEC>(out + (int64_t)row * ldo + ch, tot);  // rows without slots: y0 or zeros, written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward, source side, over the TRANSPOSED CSR (row = source j, col_t[q] = target i, etype_t / w_t per transposed
// slot): g_h[j,b,:] = sum_q a[q,b] * gout[col_t[q],:]. Every head of a group gathers the same gout fragment. A source
// without out-edges stores zeros.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
rgcn_mix_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                        const int* __restrict__ etype_t, const float* __restrict__ w_t,
                        const float* __restrict__ comp, const float* __restrict__ gout, int64_t ldg,
                        float* __restrict__ g_h, int64_t ldgh, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col_t[base + lane] : 0;
        const int mytype = lane < n ? etype_t[base + lane] : 0;
        const float myw = lane < n ? w_t[base + lane] : 0.f;
        for (int k = 0; k < n; k += NG * U) {
          float go[U][VEC], coef[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int tgt = __shfl(mycol, idx & 63);
            const int ty = __shfl(mytype, idx & 63);
            const float ws = __shfl(myw, idx & 63);
            coef[u] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) go[u][i] = 0.f;
            if (active && idx < n) {
              load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + ch);
              coef[u] = ws * comp[(int64_t)ty * L.H + head];
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(coef[u], go[u][i], acc[i]);
          }
        }
      }
      groups_sum<VEC>(acc, L.G);
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_h + (int64_t)row * ldgh + cofs, acc);
      }
    }
  }
}

// Backward, coefficient side, over the forward CSR (row = target i): d[p,b] = w[p] * <h[col[p],b,:], gout[i,:]>, one
// store per (slot, head) into d [nnz, B]. No sum over slots is formed here: the chunk items only balance the hub rows
// and there is nothing to combine. The reduction by relation is the caller's (a fixed-order SpMM over the slots grouped
// by relation).
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
rgcn_mix_bwd_coef_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
                         const float* __restrict__ h, int64_t ldh, const float* __restrict__ gout, int64_t ldg,
                         float* __restrict__ d, int N, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    if (start == end) continue;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float go[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) go[i] = 0.f;
      if (active) load_vec<VEC>(go, gout + (int64_t)row * ldg + ch);

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        const float myw = lane < n ? w[base + lane] : 0.f;
        for (int k = 0; k < n; k += NG * U) {
          float hv[U][VEC];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
#pragma unroll
            for (int i = 0; i < VEC; ++i) hv[u][i] = 0.f;
            if (active && idx < n) load_vec<VEC>(hv[u], h + (int64_t)src * ldh + cofs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float ws = __shfl(myw, idx & 63);
            const float s = head_sum(dot_vec<VEC>(hv[u], go), L.LPH);
            if (active && idx < n && ch == 0) d[(int64_t)(base + idx) * L.H + head] = ws * s;
          }
        }
      }
    }
  }
}

bool mix_supported(int64_t B, int64_t C) { return B > 0 && B <= kMaxBases && head_width_supported(C); }

int check_sizes(int64_t N, int R, int B, int C, const char* name) {
  if (R <= 0) return fail(RGBX_E_ARG, "%s: num_relations must be positive (got %d)", name, R);
  if (int rc = check_common(N, B, C, name)) return rc;
  if ((int64_t)R * B >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: R * B exceeds int32", name);
  if (!mix_supported(B, C))
    return fail(RGBX_E_SHAPE, "%s: %d bases of %d channels (1 <= B <= %d; any C <= 64, even C <= 128, C %% 4 == 0 up to 256)",
                name, B, C, kMaxBases);
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_rgcn_slot_norm_f32(const int32_t* rowptr, const int32_t* etype, float* w, int64_t N, int R,
                                       const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0) return fail(RGBX_E_ARG, "rgcn_slot_norm: bad size");
  if (R <= 0) return fail(RGBX_E_ARG, "rgcn_slot_norm: num_relations must be positive (got %d)", R);
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "rgcn_slot_norm: size exceeds int32");
  if (N == 0) return RGBX_OK;
  if (!rowptr || !etype || !w) return fail(RGBX_E_ARG, "rgcn_slot_norm: null pointer");
  if (!aligned_to({rowptr, etype, w}, 4)) return fail(RGBX_E_ALIGN, "rgcn_slot_norm: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, 1, 0, &sd, "rgcn_slot_norm")) return rc;  // the plan only: no chunk record
  hipStream_t s = (hipStream_t)stream;
  rgcn_slot_norm_kernel<false><<<row_grid(N), 256, 0, s>>>(rowptr, etype, w, (int)N, sd);
  if (sd.threshold > 0) rgcn_slot_norm_kernel<true><<<row_grid(split->n_chunks), 256, 0, s>>>(rowptr, etype, w, split->n_chunks, sd);
  RGBX_CHECK_LAUNCH("rgcn_slot_norm_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_rgcn_mix_supported(int B, int C) { return mix_supported(B, C); }

extern "C" int rgbx_rgcn_mix_fwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* etype, const float* w,
                                     const float* comp, const float* h, int64_t ldh, const float* y0, int64_t ldy,
                                     float* out, int64_t ldo, int64_t N, int R, int B, int C,
                                     const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, B, C, "rgcn_mix_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !etype || !w || !comp || !h || !out) return fail(RGBX_E_ARG, "rgcn_mix_fwd: null pointer");
  if (ldh < (int64_t)B * C) return fail(RGBX_E_ARG, "rgcn_mix_fwd: leading dimension of h < B*C");
  if (ldo < C || (y0 && ldy < C)) return fail(RGBX_E_ARG, "rgcn_mix_fwd: leading dimension < C");
  if (out == h || out == y0) return fail(RGBX_E_ARG, "rgcn_mix_fwd: out must not alias h or y0");
  if (!aligned_to({etype, w, comp, h, y0, out}, 4))
    return fail(RGBX_E_ALIGN, "rgcn_mix_fwd: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "rgcn_mix_fwd")) return rc;
  const int vec = pick_vec(C, {h, y0, out, sd.pacc}, {ldh, y0 ? ldy : 0, ldo});
  GatLayout L, L1;
  if (int rc = make_layout(B, C, vec, &L, "rgcn_mix_fwd")) return rc;
  if (int rc = make_layout(1, C, vec, &L1, "rgcn_mix_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(rgcn_mix_fwd_kernel, N, rowptr, col, etype, w, comp, h, ldh, y0, ldy, out, ldo, n_items, L, sd);
  if (sd.threshold > 0)  // a plain sum of one-head rows: the chunk partials added in chunk order
    RGBX_VEC_SWITCH(vec, attn_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(
                             split->n_long, split->long_row, split->long_chunk_ptr, out, ldo, C, 0, L1, sd));
  RGBX_CHECK_LAUNCH("rgcn_mix_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_rgcn_mix_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* etype_t,
                                         const float* w_t, const float* comp, const float* gout, int64_t ldg,
                                         float* g_h, int64_t ldgh, int64_t N, int R, int B, int C,
                                         const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, B, C, "rgcn_mix_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !etype_t || !w_t || !comp || !gout || !g_h)
    return fail(RGBX_E_ARG, "rgcn_mix_bwd_src: null pointer");
  const int64_t F = (int64_t)B * C;
  if (ldg < C) return fail(RGBX_E_ARG, "rgcn_mix_bwd_src: leading dimension of gout < C");
  if (ldgh < F) return fail(RGBX_E_ARG, "rgcn_mix_bwd_src: leading dimension of g_h < B*C");
  if (g_h == gout) return fail(RGBX_E_ARG, "rgcn_mix_bwd_src: g_h must not alias gout");
  if (!aligned_to({etype_t, w_t, comp, gout, g_h}, 4))
    return fail(RGBX_E_ALIGN, "rgcn_mix_bwd_src: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, B, C, 0, &sd, "rgcn_mix_bwd_src")) return rc;
  const int vec = pick_vec(C, {gout, g_h, sd.pacc}, {ldg, ldgh});
  GatLayout L;
  if (int rc = make_layout(B, C, vec, &L, "rgcn_mix_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(rgcn_mix_bwd_src_kernel, N, rowptr_t, col_t, etype_t, w_t, comp, gout, ldg, g_h, ldgh, n_items, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_h, ldgh, F, 0);
  RGBX_CHECK_LAUNCH("rgcn_mix_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_rgcn_mix_bwd_coef_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* h,
                                          int64_t ldh, const float* gout, int64_t ldg, float* d, int64_t N, int R,
                                          int B, int C, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, B, C, "rgcn_mix_bwd_coef")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !w || !h || !gout || !d) return fail(RGBX_E_ARG, "rgcn_mix_bwd_coef: null pointer");
  if (ldh < (int64_t)B * C) return fail(RGBX_E_ARG, "rgcn_mix_bwd_coef: leading dimension of h < B*C");
  if (ldg < C) return fail(RGBX_E_ARG, "rgcn_mix_bwd_coef: leading dimension of gout < C");
  if (!aligned_to({w, h, gout, d}, 4)) return fail(RGBX_E_ALIGN, "rgcn_mix_bwd_coef: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, 1, 0, &sd, "rgcn_mix_bwd_coef")) return rc;  // the plan only: no chunk record
  const int vec = pick_vec(C, {h, gout}, {ldh, ldg});
  GatLayout L;
  if (int rc = make_layout(B, C, vec, &L, "rgcn_mix_bwd_coef")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(rgcn_mix_bwd_coef_kernel, N, rowptr, col, w, h, ldh, gout, ldg, d, n_items, L, sd);
  RGBX_CHECK_LAUNCH("rgcn_mix_bwd_coef_kernel");
  return RGBX_OK;
}
