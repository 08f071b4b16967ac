// TransformerConv (scaled dot-product graph attention): fused per-edge score + edge-softmax + aggregation and its
// backward, for gfx950. Stands in for TransformerConv.forward / message [PyG] (Shi et al., "Masked Label Prediction:
// Unified Message Passing Model for Semi-Supervised Classification").
//
// For an edge j -> i in forward CSR slot p and head h (lane layout as in gatv2.hip, one wave per CSR row), with
// q, k, v [N, H*C] (each its own pointer and leading dimension; the layer hands k and v as neighbouring column blocks
// of one product, so the two rows of a source are one stream):
//   e_p      = <q[i,h,:], k[j,h,:]> * scale        (scale = 1 / sqrt(C_true), passed in: padding must not change it)
//   alpha_p  = softmax over the in-edges of i      (online, max-shifted: expf(e - best))
//   out[i,h,:] = sum_p alpha_p kappa_p v[j,h,:]
// The scored row (k_j) is not the message (v_j): two rows are moved per slot. The edges are taken as given (no
// self-loop rewrite), so a row may have no slot at all: its softmax runs over an empty set, its output is exact zeros,
// its saved state is (m, rden) = (0, 0) and its record (shift, D) = (0, 0), which no slot ever reads.
//
// The attention dropout keep of (forward CSR slot, head) is the hash gatv2.hip uses (same stream constant, so
// rgbx_gatv2_draws_u8 writes these decisions out too); the backward recomputes it and every score. No [E', H] tensor
// is ever written, there are no float atomics, and every sum runs in a fixed order.
#include <cmath>

#include "attn_common.h"

namespace rgbx {
namespace {

// ------------------------------------------------------------------------------------------
// Forward: online softmax (running max, denominator, rescaled accumulator) over the slots of a row, read once; per
// slot the k row is scored against the target's q row in registers and the v row is accumulated.
// TRAIN: attention dropout in the accumulation (the normaliser stays that of the undropped softmax).
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
transformer_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ q,
                       int64_t ldq, const float* __restrict__ kx, int64_t ldk, const float* __restrict__ vx,
                       int64_t ldv, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                       float* __restrict__ rden_out, int N, float scale, const GatLayout L, const AttnSplit sp,
                       const AttnRng rng) {
  constexpr int U = 4;  // neighbour rows in flight per lane group (k and v each)
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float qi[VEC], acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) qi[i] = acc[i] = 0.f;
      if (active) load_vec<VEC>(qi, q + (int64_t)row * ldq + cofs);
      float m = kNegBig, l = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float kv[U][VEC], vv[U][VEC];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
#pragma unroll
            for (int i = 0; i < VEC; ++i) kv[u][i] = vv[u][i] = 0.f;
            if (ok[u]) {
              load_vec<VEC>(kv[u], kx + (int64_t)src * ldk + cofs);
              load_vec<VEC>(vv[u], vx + (int64_t)src * ldv + cofs);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float e = head_sum(dot_vec<VEC>(qi, kv[u]), L.LPH) * scale;
            const float mn = ok[u] ? fmaxf(m, e) : m;
            const float sc = expf(m - mn);
            const float p = ok[u] ? expf(e - mn) : 0.f;
            l = fmaf(l, sc, p);
            float pk = p;
            if constexpr (TRAIN)
              pk = drop_keep<kStreamAttnDrop>(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? p * rng.inv_keep : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc[i], sc, pk * vv[u][i]);
            m = mn;
          }
        }
      }
      softmax_merge_groups<VEC>(m, l, acc, L.G);
      if (g == 0 && active) {
        if constexpr (CHUNK) {  // un-normalised online-softmax state of this chunk
          store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
          if (ch == 0) {
            sp.p0[(int64_t)item * L.H + head] = m;
            sp.p1[(int64_t)item * L.H + head] = l;
          }
        } else {
          // a row without slots: l = 0, acc = 0 -> exact zeros and the state (0, 0)
          const float rd = l > 0.f ? 1.0f / (l + 1e-16f) : 0.f;
          float r[VEC];
#pragma unroll
          for (int i = 0; i < VEC; ++i) r[i] = acc[i] * rd;
          store_vec<VEC>(out + (int64_t)row * ldo + cofs, r);
          if (m_out && ch == 0) {
            m_out[(int64_t)row * L.H + head] = l > 0.f ? m : 0.f;
            rden_out[(int64_t)row * L.H + head] = rd;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward. With kappa = keep / (1 - p) (1 without dropout), D_i = <gout_i, out_i> per head:
//   de = alpha (kappa <gout_i, v_j> - D_i)
//   g_q[i] = scale sum_p de k_j,  g_k[j] = scale sum_p de q_i,  g_v[j] = sum_p alpha kappa gout_i
//
// Target side, over the forward CSR (row = target i): g_q and the per-(target, head) record
// nodeq = (m - log(rden), D) of the source pass. A row without slots runs no slot loop and STORES its zero
// accumulator and the record (0, 0): nothing is left unwritten.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
transformer_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ q,
                           int64_t ldq, const float* __restrict__ kx, int64_t ldk, const float* __restrict__ vx,
                           int64_t ldv, const float* __restrict__ m_in, const float* __restrict__ rden_in,
                           const float* __restrict__ out, int64_t ldo, const float* __restrict__ gout, int64_t ldg,
                           float2* __restrict__ nodeq, float* __restrict__ g_q, int64_t ldgq, int N, float scale,
                           const GatLayout L, const AttnSplit sp, const AttnRng rng) {
  constexpr int U = 3;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    // a hub row: its record here, its sums by the chunk + combine kernels
    const bool hub = !row_item<CHUNK>(rowptr, sp, item, row, start, end);
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float qi[VEC], go[VEC], acc[VEC];
      float shift = 0.f, dsum = 0.f;
      {
        float o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) qi[i] = go[i] = o[i] = acc[i] = 0.f;
        if (active) {
          load_vec<VEC>(qi, q + (int64_t)row * ldq + cofs);
          load_vec<VEC>(go, gout + (int64_t)row * ldg + cofs);
          load_vec<VEC>(o, out + (int64_t)row * ldo + cofs);
          shift = softmax_shift(m_in[(int64_t)row * L.H + head], rden_in[(int64_t)row * L.H + head]);
        }
        dsum = head_sum(dot_vec<VEC>(go, o), L.LPH);
      }
      if constexpr (!CHUNK) {
        if (g == 0 && active && ch == 0) nodeq[(int64_t)row * L.H + head] = make_float2(shift, dsum);
        if (hub) continue;
      }

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float kv[U][VEC], vv[U][VEC];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
#pragma unroll
            for (int i = 0; i < VEC; ++i) kv[u][i] = vv[u][i] = 0.f;
            if (ok[u]) {
              load_vec<VEC>(kv[u], kx + (int64_t)src * ldk + cofs);
              load_vec<VEC>(vv[u], vx + (int64_t)src * ldv + cofs);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float e = head_sum(dot_vec<VEC>(qi, kv[u]), L.LPH) * scale;
            const float dal = head_sum(dot_vec<VEC>(vv[u], go), L.LPH);
            float kappa = 1.f;
            if constexpr (TRAIN)
              kappa = drop_keep<kStreamAttnDrop>(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - shift) : 0.f;
            const float de = alpha * (kappa * dal - dsum);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(de, kv[u][i], acc[i]);
          }
        }
      }
      groups_sum<VEC>(acc, L.G);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] *= scale;
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_q + (int64_t)row * ldgq + cofs, acc);  // rows without slots: zeros, written
      }
    }
  }
}

// Source side, over the TRANSPOSED CSR (row = source j, col_t[p] = target i, t2f[p] = the forward slot of the same
// edge, which keys its dropout decision): g_k[j,h,:] = scale sum_p de q_i, g_v[j,h,:] = sum_p alpha kappa gout_i. The
// source's own k and v rows stay in registers; two rows (q_i, gout_i) and the record of i are gathered per slot. A
// source without out-edges stores zeros.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
transformer_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                           const int* __restrict__ t2f, const float* __restrict__ q, int64_t ldq,
                           const float* __restrict__ kx, int64_t ldk, const float* __restrict__ vx, int64_t ldv,
                           const float2* __restrict__ nodeq, const float* __restrict__ gout, int64_t ldg,
                           float* __restrict__ g_k, int64_t ldgk, float* __restrict__ g_v, int64_t ldgv, int N,
                           float scale, const GatLayout L, const AttnSplit sp, const AttnRng rng) {
  constexpr int U = 2;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float kj[VEC], vj[VEC], ak[VEC], av[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) kj[i] = vj[i] = ak[i] = av[i] = 0.f;
      if (active) {
        load_vec<VEC>(kj, kx + (int64_t)row * ldk + cofs);
        load_vec<VEC>(vj, vx + (int64_t)row * ldv + cofs);
      }

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col_t[base + lane] : 0;
        int myslot = 0;
        if constexpr (TRAIN) myslot = lane < n ? t2f[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float qi[U][VEC], go[U][VEC];
          float sh[U], dsm[U];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int tgt = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
            sh[u] = dsm[u] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) qi[u][i] = go[u][i] = 0.f;
            if (ok[u]) {
              const float2 rec = nodeq[(int64_t)tgt * L.H + head];
              sh[u] = rec.x;
              dsm[u] = rec.y;
              load_vec<VEC>(qi[u], q + (int64_t)tgt * ldq + cofs);
              load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + cofs);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float e = head_sum(dot_vec<VEC>(qi[u], kj), L.LPH) * scale;
            const float dal = head_sum(dot_vec<VEC>(vj, go[u]), L.LPH);
            float kappa = 1.f;
            if constexpr (TRAIN)
              kappa = drop_keep<kStreamAttnDrop>(s0, s1, __shfl(myslot, idx & 63), head, rng.p_drop)
                          ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - sh[u]) : 0.f;
            const float de = alpha * (kappa * dal - dsm[u]);
            const float akp = alpha * kappa;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              ak[i] = fmaf(de, qi[u][i], ak[i]);
              av[i] = fmaf(akp, go[u][i], av[i]);
            }
          }
        }
      }
      for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          ak[i] += __shfl_xor(ak[i], off);
          av[i] += __shfl_xor(av[i], off);
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) ak[i] *= scale;
      if (g == 0 && active) {
        if constexpr (CHUNK) {
          store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + cofs, ak);
          store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + F + cofs, av);
        } else {
          store_vec<VEC>(g_k + (int64_t)row * ldgk + cofs, ak);
          store_vec<VEC>(g_v + (int64_t)row * ldgv + cofs, av);
        }
      }
    }
  }
}

int check_scale(float scale, const char* name) {
  if (!(scale > 0.f) || !std::isfinite(scale)) return fail(RGBX_E_ARG, "%s: scale must be positive and finite", name);
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_transformer_supported(int H, int C) {
  return H > 0 && head_width_supported(C);
}

extern "C" int rgbx_transformer_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* q, int64_t ldq,
                                        const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                                        int64_t ldo, float* m, float* rden, int64_t N, int H, int C, float scale,
                                        const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                                        rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "transformer_fwd")) return rc;
  if (!head_width_supported(C)) return fail_head_width("transformer_fwd", C);
  if (int rc = check_scale(scale, "transformer_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !q || !k || !v || !out) return fail(RGBX_E_ARG, "transformer_fwd: null pointer");
  if ((m == nullptr) != (rden == nullptr)) return fail(RGBX_E_ARG, "transformer_fwd: m and rden go together");
  if (seed && !m) return fail(RGBX_E_ARG, "transformer_fwd: training mode saves m and rden");
  const int64_t F = (int64_t)H * C;
  if (ldq < F || ldk < F || ldv < F || ldo < F) return fail(RGBX_E_ARG, "transformer_fwd: leading dimension < H*C");
  if (!aligned_to({q, k, v, out, m, rden}, 4))
    return fail(RGBX_E_ALIGN, "transformer_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 2, &sd, "transformer_fwd")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_fwd")) return rc;
  const int vec = pick_vec(C, {q, k, v, out, sd.pacc}, {ldq, ldk, ldv, ldo});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_ATTN_DISPATCH(transformer_fwd_kernel, row_grid, N, rowptr, col, q, ldq, k, ldk, v, ldv, out, ldo, m, rden,
                     n_items, scale, L, sd, rng);
  if (sd.threshold > 0) RGBX_ATTN_FWD_COMBINE(false, nullptr, out, ldo, m, rden);
  RGBX_CHECK_LAUNCH("transformer_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_transformer_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* q, int64_t ldq,
                                            const float* k, int64_t ldk, const float* v, int64_t ldv, const float* m,
                                            const float* rden, const float* out, int64_t ldo, const float* gout,
                                            int64_t ldg, float* nodeq, float* g_q, int64_t ldgq, int64_t N, int H,
                                            int C, float scale, const uint32_t* seed, float p_drop,
                                            const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "transformer_bwd_dst")) return rc;
  if (!head_width_supported(C)) return fail_head_width("transformer_bwd_dst", C);
  if (int rc = check_scale(scale, "transformer_bwd_dst")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !q || !k || !v || !m || !rden || !out || !gout || !nodeq || !g_q)
    return fail(RGBX_E_ARG, "transformer_bwd_dst: null pointer");
  const int64_t F = (int64_t)H * C;
  if (ldq < F || ldk < F || ldv < F || ldo < F || ldg < F || ldgq < F)
    return fail(RGBX_E_ARG, "transformer_bwd_dst: leading dimension < H*C");
  if (!aligned_to({nodeq}, 8)) return fail(RGBX_E_ALIGN, "transformer_bwd_dst: nodeq must be 8-byte aligned");
  if (!aligned_to({q, k, v, m, rden, out, gout, g_q}, 4))
    return fail(RGBX_E_ALIGN, "transformer_bwd_dst: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 0, &sd, "transformer_bwd_dst")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_bwd_dst")) return rc;
  const int vec = pick_vec(C, {q, k, v, out, gout, g_q, sd.pacc}, {ldq, ldk, ldv, ldo, ldg, ldgq});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_bwd_dst")) return rc;
  hipStream_t s = (hipStream_t)stream;
  float2* nq = reinterpret_cast<float2*>(nodeq);
  RGBX_ATTN_DISPATCH(transformer_bwd_dst_kernel, row_grid, N, rowptr, col, q, ldq, k, ldk, v, ldv, m, rden, out, ldo,
                     gout, ldg, nq, g_q, ldgq, n_items, scale, L, sd, rng);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_q, ldgq, F, 0);
  RGBX_CHECK_LAUNCH("transformer_bwd_dst_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_transformer_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                            const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                            int64_t ldv, const float* nodeq, const float* gout, int64_t ldg,
                                            float* g_k, int64_t ldgk, float* g_v, int64_t ldgv, int64_t N, int H,
                                            int C, float scale, const uint32_t* seed, float p_drop,
                                            const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "transformer_bwd_src")) return rc;
  if (!head_width_supported(C)) return fail_head_width("transformer_bwd_src", C);
  if (int rc = check_scale(scale, "transformer_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !q || !k || !v || !nodeq || !gout || !g_k || !g_v)
    return fail(RGBX_E_ARG, "transformer_bwd_src: null pointer");
  if (seed && !t2f) return fail(RGBX_E_ARG, "transformer_bwd_src: training mode needs the slot map");
  const int64_t F = (int64_t)H * C;
  if (ldq < F || ldk < F || ldv < F || ldg < F || ldgk < F || ldgv < F)
    return fail(RGBX_E_ARG, "transformer_bwd_src: leading dimension < H*C");
  if (!aligned_to({nodeq}, 8)) return fail(RGBX_E_ALIGN, "transformer_bwd_src: nodeq must be 8-byte aligned");
  if (!aligned_to({q, k, v, gout, g_k, g_v}, 4))
    return fail(RGBX_E_ALIGN, "transformer_bwd_src: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 0, &sd, "transformer_bwd_src")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_bwd_src")) return rc;
  const int vec = pick_vec(C, {q, k, v, gout, g_k, g_v, sd.pacc}, {ldq, ldk, ldv, ldg, ldgk, ldgv});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float2* nq = reinterpret_cast<const float2*>(nodeq);
  RGBX_ATTN_DISPATCH(transformer_bwd_src_kernel, row_grid, N, rowptr_t, col_t, t2f, q, ldq, k, ldk, v, ldv, nq, gout,
                     ldg, g_k, ldgk, g_v, ldgv, n_items, scale, L, sd, rng);
  if (sd.threshold > 0) {  // a chunk's record is (g_k | g_v)
    RGBX_ATTN_BWD_COMBINE(g_k, ldgk, 2 * F, 0);
    RGBX_ATTN_BWD_COMBINE(g_v, ldgv, 2 * F, F);
  }
  RGBX_CHECK_LAUNCH("transformer_bwd_src_kernel");
  return RGBX_OK;
}
