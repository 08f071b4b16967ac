// FiLMConv (Brockschmidt, "GNN-FiLM: Graph Neural Networks with Feature-wise Linear Modulation"): the target node
// modulates every incoming message per channel, BEFORE the nonlinearity, and the modulated messages are aggregated per
// relation; forward and the two backward passes, for gfx950. Stands in for FiLMConv.forward / message [PyG].
//
// With R relations and C channels the dense products come first:
//   h  = x @ [W_0 | ... | W_{R-1}]            viewed [N * R, C]:  row j * R + r = the message row of source j under r
//   fb = [film_0(x) | ... | film_{R-1}(x)]    viewed [N * R, 2C]: row i * R + r = beta_r[i] | gamma_r[i]  (beta FIRST)
// (gamma sits `gofs` floats behind beta: C in this layout, the full width when the operands are a column block of
// wider matrices) and for an edge j -> i of relation r in forward CSR slot p, with slot weight w[p]:
//   z_p      = fmaf(gamma_r[i], h[j * R + r], beta_r[i])
//   out[i,:] = y0[i,:] + sum_p w[p] * act(z_p)                              act: 0 = identity, 1 = relu
// The lane layout is attn_common.h's with H = 1 (a row fragment of VEC channels per lane, G lanes per neighbour row,
// 64 / G rows per wave-instruction); a lane never talks to its neighbours inside a slot.
//
// Nothing per edge is written or read back and no record passes between the kernels: both backward passes recompute
// z with the forward's own fmaf, so the relu mask is the forward's bit for bit (relu'(0) = 0). No float atomics, no
// scratch, no LDS; every sum runs in a fixed order (slots of a lane group in slot order, lane groups by a butterfly,
// hub-row chunks in chunk order), and every output row is written.
#include "edge_common.h"

namespace rgbx {
namespace {

// (act && z <= 0) rather than fmaxf: a NaN stays a NaN, -0 and the tie z == 0 give 0 with derivative 0.
__device__ __forceinline__ float film_act(float z, int act) { return (act && z <= 0.f) ? 0.f : z; }
__device__ __forceinline__ float film_dact(float z, int act) { return (act && z <= 0.f) ? 0.f : 1.f; }

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR. TYPED: every slot reads its relation and weight, gathers row col * R + type of
// h and reads the film row (i, type) from device memory (a target's R * 2C floats stay cache-resident over its row).
// !TYPED (etype == NULL, R = 1): the target's one film row stays in registers and the weight is 1 / len from rowptr
// (mean) or 1. CHUNK: the wave owns a chunk of a hub row and leaves a partial row of C floats; the chunk that starts
// the row carries y0, so the combine kernel only adds.
template <int VEC, bool CHUNK, bool TYPED>
__global__ void __launch_bounds__(256)
film_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ etype,
                const float* __restrict__ w, const float* __restrict__ h, int64_t ldh, const float* __restrict__ fb,
                int64_t ldfb, int64_t gofs, const float* __restrict__ y0, int64_t ldy, float* __restrict__ out,
                int64_t ldo, int N, int R, int mean, int act, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;  // neighbour rows in flight per lane group
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;  // H = 1: the group is the head

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float acc[VEC], be[VEC], ga[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = be[i] = ga[i] = 0.f;
    float wrow = 1.f;
    if constexpr (!TYPED) {
      if (active) {
        load_vec<VEC>(be, fb + (int64_t)row * ldfb + ch);
        load_vec<VEC>(ga, fb + (int64_t)row * ldfb + gofs + ch);
      }
      if (mean) {
        int len = end - start;
        if constexpr (CHUNK) len = __builtin_amdgcn_readfirstlane(rowptr[row + 1] - rowptr[row]);  // the WHOLE row's
        wrow = len > 0 ? 1.0f / (float)len : 0.f;
      }
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col[base + lane] : 0;
      int mytype = 0;
      float myw = wrow;
      if constexpr (TYPED) {
        mytype = lane < n ? etype[base + lane] : 0;
        myw = lane < n ? w[base + lane] : 0.f;
      }
      for (int k = 0; k < n; k += NG * U) {
        float hv[U][VEC], bv[U][VEC], gv[U][VEC], ws[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
          int ty = 0;
          ws[u] = wrow;
          if constexpr (TYPED) {
            ty = __shfl(mytype, idx & 63);
            ws[u] = __shfl(myw, idx & 63);
          }
          ok[u] = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            hv[u][i] = 0.f;
            bv[u][i] = be[i];
            gv[u][i] = ga[i];
          }
          if (ok[u]) {
            load_vec<VEC>(hv[u], h + ((int64_t)src * R + ty) * ldh + ch);
            if constexpr (TYPED) {
              const float* frow = fb + ((int64_t)row * R + ty) * ldfb + ch;
              load_vec<VEC>(bv[u], frow);
              load_vec<VEC>(gv[u], frow + gofs);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float z = fmaf(gv[u][i], hv[u][i], bv[u][i]);
            const float m = ok[u] ? film_act(z, act) : 0.f;  // a slot past the row's end adds nothing, whatever beta
            acc[i] = fmaf(ws[u], m, acc[i]);
          }
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      bool root = y0 != nullptr;
      if constexpr (CHUNK) root = root && start == rowptr[row];
      if (root) {
        float yv[VEC];
        load_vec<VEC>(yv, y0 + (int64_t)row * ldy + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += yv[i];  // after the slot loop: out is written once
      }
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);  // rows without slots: y0 or zeros, written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward, source side, over the relation-expanded TRANSPOSED CSR of N * R rows (row j * R + r = the out-edges of j
// with relation r, col_t = targets i): the row's own h stays in registers, gout and the film row (i, r) of the target
// are gathered per slot.  g_h[j*R + r,:] = sum_q w_q * gamma_r[i_q] (.) act'(z_q) (.) gout[i_q].  The slot weight is
// w_t[q], or 1 / indeg(i_q) read from the forward rowptr `deg_rowptr`, or 1. A row without slots stores zeros.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
film_bwd_src_kernel(const int* __restrict__ rowptr_x, const int* __restrict__ col_t, const float* __restrict__ w_t,
                    const int* __restrict__ deg_rowptr, const float* __restrict__ h, int64_t ldh,
                    const float* __restrict__ fb, int64_t ldfb, int64_t gofs, const float* __restrict__ gout,
                    int64_t ldg, float* __restrict__ g_h, int64_t ldgh, int NR, int R, int act, const GatLayout L,
                    const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < NR; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_x, sp, item, row, start, end)) continue;
    const int r = row % R;
    float hj[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) hj[i] = acc[i] = 0.f;
    if (active && start < end) load_vec<VEC>(hj, h + (int64_t)row * ldh + ch);

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col_t[base + lane] : 0;
      float myw = lane < n ? 1.f : 0.f;
      if (lane < n) {
        if (w_t) myw = w_t[base + lane];
        else if (deg_rowptr) myw = 1.0f / (float)(deg_rowptr[mycol + 1] - deg_rowptr[mycol]);  // >= 1: this very edge
      }
      for (int k = 0; k < n; k += NG * U) {
        float go[U][VEC], bv[U][VEC], gv[U][VEC], ws[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int tgt = __shfl(mycol, idx & 63);
          ws[u] = __shfl(myw, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) go[u][i] = bv[u][i] = gv[u][i] = 0.f;
          if (active && idx < n) {
            const float* frow = fb + ((int64_t)tgt * R + r) * ldfb + ch;
            load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + ch);
            load_vec<VEC>(bv[u], frow);
            load_vec<VEC>(gv[u], frow + gofs);
          } else {
            ws[u] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // a slot past the row's end holds w = gamma = gout = 0
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float z = fmaf(gv[u][i], hj[i], bv[u][i]);
            acc[i] = fmaf(ws[u] * gv[u][i] * film_dact(z, act), go[u][i], acc[i]);
          }
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(g_h + (int64_t)row * ldgh + ch, acc);  // rows without slots: zeros, written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward, film side, over the relation-expanded FORWARD CSR of N * R rows (row i * R + r = the in-edges of i with
// relation r, col_e = sources j): the row's film row and gout[i] stay in registers, h[j * R + r] is gathered per slot.
//   g_beta[i*R + r]  = w (.) gout[i] (.) sum_p act'(z_p)          g_gamma[i*R + r] = w (.) gout[i] (.) sum_p act'(z_p) h_p
// stored as ONE row (g_beta | g_gamma) in fb's layout. One accumulator pair and one store per row; the row's weight is
// 1.0f / (float)len (mean: the bits of the typed view's w_f) or 1. A row without slots stores zeros. A chunk's record
// is (g_beta | g_gamma), already scaled, so the combine kernel only adds.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
film_bwd_film_kernel(const int* __restrict__ rowptr_e, const int* __restrict__ col_e, const float* __restrict__ h,
                     int64_t ldh, const float* __restrict__ fb, int64_t ldfb, int64_t gofs,
                     const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_fb, int64_t ldgfb, int NR, int R, int mean, int act,
                     const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < NR; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_e, sp, item, row, start, end)) continue;
    const int r = row % R;
    float be[VEC], ga[VEC], ab[VEC], ag[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) be[i] = ga[i] = ab[i] = ag[i] = 0.f;
    if (active && start < end) {
      load_vec<VEC>(be, fb + (int64_t)row * ldfb + ch);
      load_vec<VEC>(ga, fb + (int64_t)row * ldfb + gofs + ch);
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col_e[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float hv[U][VEC];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
          ok[u] = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) hv[u][i] = 0.f;
          if (ok[u]) load_vec<VEC>(hv[u], h + ((int64_t)src * R + r) * ldh + ch);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float z = fmaf(ga[i], hv[u][i], be[i]);
            const float d = ok[u] ? film_dact(z, act) : 0.f;  // a slot past the row's end has z = beta: masked out
            ab[i] += d;
            ag[i] = fmaf(d, hv[u][i], ag[i]);
          }
        }
      }
    }
    groups_sum<VEC>(ab, L.G);
    groups_sum<VEC>(ag, L.G);
    if (g == 0 && active) {
      float go[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) go[i] = 0.f;
      float wrow = 1.f;
      if (start < end) {
        load_vec<VEC>(go, gout + (int64_t)(row / R) * ldg + ch);
        if (mean) {
          int len = end - start;
          if constexpr (CHUNK) len = rowptr_e[row + 1] - rowptr_e[row];  // the WHOLE row's
          wrow = 1.0f / (float)len;
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float s = wrow * go[i];
        ab[i] *= s;
        ag[i] *= s;
      }
      if constexpr (CHUNK) {
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + ch, ab);
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + F + ch, ag);
      } else {
        store_vec<VEC>(g_fb + (int64_t)row * ldgfb + ch, ab);  // rows without slots: zeros, written
        store_vec<VEC>(g_fb + (int64_t)row * ldgfb + gofs + ch, ag);
      }
    }
  }
}

int check_sizes(int64_t N, int R, int C, int act, const char* name) {
  if (R <= 0) return fail(RGBX_E_ARG, "%s: num_relations must be positive (got %d)", name, R);
  if (act != 0 && act != 1) return fail(RGBX_E_ARG, "%s: act must be 0 (identity) or 1 (relu), got %d", name, act);
  if (int rc = check_common(N, 1, C, name)) return rc;
  if (N * (int64_t)R >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: N * R exceeds int32", name);
  return check_width(C, name);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_film_supported(int C) { return head_width_supported(C); }

extern "C" int rgbx_film_fwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* etype, const float* w,
                                 const float* h, int64_t ldh, const float* fb, int64_t ldfb, int64_t gofs,
                                 const float* y0, int64_t ldy, float* out, int64_t ldo, int64_t N, int R, int C, int mean, int act,
                                 const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, C, act, "film_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !h || !fb || !out) return fail(RGBX_E_ARG, "film_fwd: null pointer");
  if (etype && !w) return fail(RGBX_E_ARG, "film_fwd: null pointer (typed slots need their weights w)");
  if (!etype && R != 1) return fail(RGBX_E_ARG, "film_fwd: etype == NULL is the single-relation call (got R = %d)", R);
  if (ldh < C) return fail(RGBX_E_ARG, "film_fwd: leading dimension of h < C");
  if (gofs < C || ldfb < gofs + C)
    return fail(RGBX_E_ARG, "film_fwd: gamma offset < C or leading dimension of fb < gofs + C");
  if (ldo < C || (y0 && ldy < C)) return fail(RGBX_E_ARG, "film_fwd: leading dimension < C");
  if (out == h || out == fb || out == y0) return fail(RGBX_E_ARG, "film_fwd: out must not alias h, fb or y0");
  if (!aligned_to({rowptr, col, etype, w, h, fb, y0, out}, 4))
    return fail(RGBX_E_ALIGN, "film_fwd: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "film_fwd")) return rc;
  const int vec = pick_vec(C, {h, fb, y0, out, sd.pacc}, {ldh, ldfb, gofs, y0 ? ldy : 0, ldo});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "film_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (etype)
    RGBX_EDGE_ROWS_X(film_fwd_kernel, (true), N, rowptr, col, etype, w, h, ldh, fb, ldfb, gofs, y0, ldy, out,
                     ldo, n_items, R, mean, act, L, sd);
  else
    RGBX_EDGE_ROWS_X(film_fwd_kernel, (false), N, rowptr, col, etype, w, h, ldh, fb, ldfb, gofs, y0, ldy, out,
                     ldo, n_items, R, mean, act, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(out, ldo, C, 0);  // a plain sum: the chunk partials added in chunk order
  RGBX_CHECK_LAUNCH("film_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_film_bwd_src_f32(const int32_t* rowptr_x, const int32_t* col_t, const float* w_t,
                                     const int32_t* deg_rowptr, const float* h, int64_t ldh, const float* fb,
                                     int64_t ldfb, int64_t gofs, const float* gout, int64_t ldg, float* g_h,
                                     int64_t ldgh, int64_t N, int R, int C, int act, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, C, act, "film_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_x || !col_t || !h || !fb || !gout || !g_h) return fail(RGBX_E_ARG, "film_bwd_src: null pointer");
  if (ldh < C || ldg < C || ldgh < C) return fail(RGBX_E_ARG, "film_bwd_src: leading dimension < C");
  if (gofs < C || ldfb < gofs + C)
    return fail(RGBX_E_ARG, "film_bwd_src: gamma offset < C or leading dimension of fb < gofs + C");
  if (g_h == h || g_h == fb || g_h == gout) return fail(RGBX_E_ARG, "film_bwd_src: g_h must not alias h, fb or gout");
  if (!aligned_to({rowptr_x, col_t, w_t, deg_rowptr, h, fb, gout, g_h}, 4))
    return fail(RGBX_E_ALIGN, "film_bwd_src: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "film_bwd_src")) return rc;
  const int vec = pick_vec(C, {h, fb, gout, g_h, sd.pacc}, {ldh, ldfb, gofs, ldg, ldgh});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "film_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(film_bwd_src_kernel, N * R, rowptr_x, col_t, w_t, deg_rowptr, h, ldh, fb, ldfb, gofs, gout, ldg, g_h,
                 ldgh, n_items, R, act, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_h, ldgh, C, 0);
  RGBX_CHECK_LAUNCH("film_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_film_bwd_film_f32(const int32_t* rowptr_e, const int32_t* col_e, const float* h, int64_t ldh,
                                      const float* fb, int64_t ldfb, int64_t gofs, const float* gout, int64_t ldg,
                                      float* g_fb, int64_t ldgfb, int64_t N, int R, int C, int mean, int act,
                                      const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, R, C, act, "film_bwd_film")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_e || !col_e || !h || !fb || !gout || !g_fb) return fail(RGBX_E_ARG, "film_bwd_film: null pointer");
  if (ldh < C || ldg < C) return fail(RGBX_E_ARG, "film_bwd_film: leading dimension < C");
  if (gofs < C || ldfb < gofs + C || ldgfb < gofs + C)
    return fail(RGBX_E_ARG, "film_bwd_film: gamma offset < C or leading dimension of fb / g_fb < gofs + C");
  if (g_fb == h || g_fb == fb || g_fb == gout)
    return fail(RGBX_E_ARG, "film_bwd_film: g_fb must not alias h, fb or gout");
  if (!aligned_to({rowptr_e, col_e, h, fb, gout, g_fb}, 4))
    return fail(RGBX_E_ALIGN, "film_bwd_film: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, 2 * C, 0, &sd, "film_bwd_film")) return rc;
  const int vec = pick_vec(C, {h, fb, gout, g_fb, sd.pacc}, {ldh, ldfb, gofs, ldg, ldgfb});
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "film_bwd_film")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(film_bwd_film_kernel, N * R, rowptr_e, col_e, h, ldh, fb, ldfb, gofs, gout, ldg, g_fb, ldgfb, n_items,
                 R, mean, act, L, sd);
  if (sd.threshold > 0) {  // a chunk's record is (g_beta | g_gamma)
    RGBX_ATTN_BWD_COMBINE(g_fb, ldgfb, 2 * (int64_t)C, 0);
    RGBX_ATTN_BWD_COMBINE(g_fb + gofs, ldgfb, 2 * (int64_t)C, C);
  }
  RGBX_CHECK_LAUNCH("film_bwd_film_kernel");
  return RGBX_OK;
}
