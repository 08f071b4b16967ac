// GATv2 (dynamic attention): fused per-edge score + edge-softmax + aggregation and its backward, for gfx950. Stands in
// for GATv2Conv.forward / edge_update / message [PyG] (Brody et al., "How Attentive are Graph Attention Networks?").
//
// For an edge j -> i and head h (lane layout as in gat.hip / supergat.hip, one wave per CSR row):
//   s_c = xl[j,h,c] + xr[i,h,c],  e = sum_c att[h,c] leaky_relu(s_c),  alpha = softmax_i(e),
//   out[i,h,:] = sum_j alpha kappa xl[j,h,:]
// The non-linearity sits in front of the attention vector, so the score is no sum of two per-node scalars: the
// target's xr row and att stay in registers and every gathered xl row is scored against them by a cross-lane reduction
// over the head's lanes. The gathered row is also the message: one row per slot is moved, as in GAT's aggregation.
//
// The attention dropout keep of (forward CSR slot, head) is a hash of a 64-bit seed that lives on the device; the
// backward recomputes it and every score. No [E', H] tensor is ever written, there are no float atomics, and every sum
// runs in a fixed order.
#include "attn_common.h"

namespace rgbx {
namespace {

// This lane's share of the score: sum_v att_v lrelu(xl_v + xr_v); lr receives lrelu(s), s the pre-activation.
template <int VEC>
__device__ __forceinline__ float score_part(const float (&xl)[VEC], const float (&xr)[VEC], const float (&att)[VEC],
                                            float slope, float (&s)[VEC], float (&lr)[VEC]) {
  float e = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    s[i] = xl[i] + xr[i];
    lr[i] = s[i] > 0.f ? s[i] : slope * s[i];
    e = fmaf(att[i], lr[i], e);
  }
  return e;
}

// ------------------------------------------------------------------------------------------
// Forward: online softmax (running max, denominator, rescaled accumulator) over the slots of a row, read once.
// TRAIN: attention dropout in the accumulation (the normaliser stays that of the undropped softmax).
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
gatv2_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ xl, int64_t ldl,
                 const float* __restrict__ xr, int64_t ldr, const float* __restrict__ att,
                 const float* __restrict__ bias, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                 float* __restrict__ rden_out, int N, float slope, const GatLayout L, const AttnSplit sp,
                 const AttnRng rng) {
  constexpr int U = 4;  // neighbour rows in flight per lane group
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
      float xri[VEC], av[VEC], acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) xri[i] = av[i] = acc[i] = 0.f;
      if (active) {
        load_vec<VEC>(xri, xr + (int64_t)row * ldr + cofs);
        load_vec<VEC>(av, att + cofs);
      }
      float m = kNegBig, l = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float v[U][VEC];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
            if (ok[u]) load_vec<VEC>(v[u], xl + (int64_t)src * ldl + cofs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            float s[VEC], lr[VEC];
            const float e = head_sum(score_part<VEC>(v[u], xri, av, slope, s, lr), L.LPH);
            const float mn = ok[u] ? fmaxf(m, e) : m;
            const float sc = expf(m - mn);
            const float p = ok[u] ? expf(e - mn) : 0.f;
            l = fmaf(l, sc, p);
            float pk = p;
            if constexpr (TRAIN)
              pk = drop_keep<kStreamAttnDrop>(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? p * rng.inv_keep : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc[i], sc, pk * v[u][i]);
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
          const float rd = l > 0.f ? 1.0f / (l + 1e-16f) : 0.f;
          float r[VEC], bv[VEC];
#pragma unroll
          for (int i = 0; i < VEC; ++i) bv[i] = 0.f;
          if (bias) load_vec<VEC>(bv, bias + cofs);
#pragma unroll
          for (int i = 0; i < VEC; ++i) r[i] = acc[i] * rd + bv[i];
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
// Backward. With kappa = keep / (1 - p) (1 without dropout), D_i = <gout_i, out_i - bias> per head:
//   de = alpha (kappa <gout_i, xl_j> - D_i),  ds_c = de att_c lrelu'(s_c)
//   g_xr[i] = sum_j ds,  g_xl[j] = sum_i (kappa alpha gout_i + ds),  g_att[h,c] = sum_edges de lrelu(s_c)
//
// Target side, over the forward CSR (row = target i): g_xr, the per-(target, head) record nodeq = (m - log(rden), D)
// of the source pass, and this workgroup's share of g_att. The head chunks are the OUTER loop so that a lane keeps one
// g_att accumulator over all the rows of its wave; at the end of a chunk the four waves' sums are added in wave order
// and stored as record blockIdx.x of att_part [gridDim.x, H*C].
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
gatv2_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ xl,
                     int64_t ldl, const float* __restrict__ xr, int64_t ldr, const float* __restrict__ att,
                     const float* __restrict__ m_in, const float* __restrict__ rden_in, const float* __restrict__ out,
                     int64_t ldo, const float* __restrict__ bias, const float* __restrict__ gout, int64_t ldg,
                     float2* __restrict__ nodeq, float* __restrict__ g_xr, int64_t ldgr, float* __restrict__ att_part,
                     int N, float slope, const GatLayout L, const AttnSplit sp, const AttnRng rng) {
  constexpr int U = 3;
  __shared__ float red[4][kWave * 4];
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const int wave = threadIdx.x >> 6;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
    const int head = hbase + hl;
    const bool active = hl < L.HPC && head < L.H && ch < L.C;
    const int cofs = head * L.C + ch;
    float av[VEC], ga[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) av[i] = ga[i] = 0.f;
    if (active) load_vec<VEC>(av, att + cofs);

    for (int item = blockIdx.x * wpb + wave; item < N; item += gridDim.x * wpb) {
      int row, start, end;
      // a hub row: its record here, its sums by the chunk + combine kernels
      const bool hub = !row_item<CHUNK>(rowptr, sp, item, row, start, end);
      float xri[VEC], go[VEC], acc[VEC];
      float shift = 0.f, dsum = 0.f;
      {
        float o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) xri[i] = go[i] = o[i] = acc[i] = 0.f;
        if (active) {
          load_vec<VEC>(xri, xr + (int64_t)row * ldr + cofs);
          load_vec<VEC>(go, gout + (int64_t)row * ldg + cofs);
          load_vec<VEC>(o, out + (int64_t)row * ldo + cofs);
          if (bias) {  // `out` was stored with the bias added: the softmax Jacobian needs the bare aggregate
            float bv[VEC];
            load_vec<VEC>(bv, bias + cofs);
#pragma unroll
            for (int i = 0; i < VEC; ++i) o[i] -= bv[i];
          }
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
          float v[U][VEC];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
            if (ok[u]) load_vec<VEC>(v[u], xl + (int64_t)src * ldl + cofs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            float s[VEC], lr[VEC];
            const float e = head_sum(score_part<VEC>(v[u], xri, av, slope, s, lr), L.LPH);
            const float dal = head_sum(dot_vec<VEC>(v[u], go), L.LPH);
            float kappa = 1.f;
            if constexpr (TRAIN)
              kappa = drop_keep<kStreamAttnDrop>(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - shift) : 0.f;
            const float de = alpha * (kappa * dal - dsum);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              acc[i] = fmaf(de * av[i], s[i] > 0.f ? 1.f : slope, acc[i]);
              ga[i] = fmaf(de, lr[i], ga[i]);
            }
          }
        }
      }
      groups_sum<VEC>(acc, L.G);
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_xr + (int64_t)row * ldgr + cofs, acc);
      }
    }

    // this workgroup's g_att record for the chunk: lane groups, then waves, in a fixed order
    groups_sum<VEC>(ga, L.G);
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) red[wave][t * VEC + i] = ga[i];
    }
    __syncthreads();
    if (wave == 0 && g == 0 && active) {
      float r[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        r[i] = red[0][t * VEC + i];
        for (int w = 1; w < wpb; ++w) r[i] += red[w][t * VEC + i];
      }
      store_vec<VEC>(att_part + (int64_t)blockIdx.x * F + cofs, r);
    }
    __syncthreads();
  }
}

// Source side, over the TRANSPOSED CSR (row = source j, col_t[p] = target i, t2f[p] = the forward slot of the same
// edge, which keys its dropout decision): g_xl[j,h,:] = sum_p (kappa alpha gout_i + ds). Two rows (xr_i, gout_i) and
// the record of i are gathered per slot.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
gatv2_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ t2f,
                     const float* __restrict__ xl, int64_t ldl, const float* __restrict__ xr, int64_t ldr,
                     const float* __restrict__ att, const float2* __restrict__ nodeq, const float* __restrict__ gout,
                     int64_t ldg, float* __restrict__ g_xl, int64_t ldgl, int N, float slope, const GatLayout L,
                     const AttnSplit sp, const AttnRng rng) {
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
      float xlj[VEC], av[VEC], acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) xlj[i] = av[i] = acc[i] = 0.f;
      if (active) {
        load_vec<VEC>(xlj, xl + (int64_t)row * ldl + cofs);
        load_vec<VEC>(av, att + cofs);
      }

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col_t[base + lane] : 0;
        int myslot = 0;
        if constexpr (TRAIN) myslot = lane < n ? t2f[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float xi[U][VEC], go[U][VEC];
          float sh[U], dsm[U];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int tgt = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
            sh[u] = dsm[u] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) xi[u][i] = go[u][i] = 0.f;
            if (ok[u]) {
              const float2 q = nodeq[(int64_t)tgt * L.H + head];
              sh[u] = q.x;
              dsm[u] = q.y;
              load_vec<VEC>(xi[u], xr + (int64_t)tgt * ldr + cofs);
              load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + cofs);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            float s[VEC], lr[VEC];
            const float e = head_sum(score_part<VEC>(xlj, xi[u], av, slope, s, lr), L.LPH);
            const float dal = head_sum(dot_vec<VEC>(go[u], xlj), L.LPH);
            float kappa = 1.f;
            if constexpr (TRAIN)
              kappa = drop_keep<kStreamAttnDrop>(s0, s1, __shfl(myslot, idx & 63), head, rng.p_drop)
                          ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - sh[u]) : 0.f;
            const float de = alpha * (kappa * dal - dsm[u]);
            const float ak = alpha * kappa;
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              acc[i] = fmaf(ak, go[u][i], fmaf(de * av[i], s[i] > 0.f ? 1.f : slope, acc[i]));
          }
        }
      }
      groups_sum<VEC>(acc, L.G);
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_xl + (int64_t)row * ldgl + cofs, acc);
      }
    }
  }
}

// g_att[f] = sum of the per-workgroup records part[b, f], b = 0 .. n_rec - 1. A block owns 16 columns; its 16 x 16
// threads add the records b = r, r + 16, ... of a column, then the 16 sums in a fixed tree.
__global__ void __launch_bounds__(256)
gatv2_att_reduce_kernel(const float* __restrict__ part, int64_t n_rec, int F, float* __restrict__ g_att) {
  __shared__ float sh[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int f = blockIdx.x * 16 + c;
  float s = 0.f;
  if (f < F)
    for (int64_t b = r; b < n_rec; b += 16) s += part[b * F + f];
  sh[r][c] = s;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (r < w) sh[r][c] += sh[r + w][c];
    __syncthreads();
  }
  if (r == 0 && f < F) g_att[f] = sh[0][c];
}

// The dropout decisions of a training forward, written out for inspection (tests): keep[p, h] in forward CSR slot order.
__global__ void __launch_bounds__(256)
gatv2_draws_kernel(const uint32_t* __restrict__ seed, int64_t nnz, int H, float p_drop, uint8_t* __restrict__ keep) {
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x)
    for (int h = 0; h < H; ++h) keep[p * H + h] = drop_keep<kStreamAttnDrop>(s0, s1, (int)p, h, p_drop) ? 1 : 0;
}

// The target-side backward leaves one g_att record per workgroup, so its grid is capped and the waves stride over the
// rows.
int att_grid(int64_t N) { return capped_grid(N, 4); }

int64_t att_records(int64_t N, const rgbx_row_split_t* split) {
  return att_grid(N) + (split && split->threshold > 0 && split->n_chunks > 0 ? att_grid(split->n_chunks) : 0);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gatv2_supported(int H, int C) {
  return H > 0 && head_width_supported(C);
}

extern "C" int rgbx_gatv2_att_partial_floats(int64_t N, int H, int C, const rgbx_row_split_t* split, int64_t* count) {
  if (!count) return fail(RGBX_E_ARG, "gatv2_att_partial_floats: null pointer");
  if (int rc = check_common(N, H, C, "gatv2_att_partial_floats")) return rc;
  *count = att_records(N, split) * (int64_t)H * C;
  return RGBX_OK;
}

extern "C" int rgbx_gatv2_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldl,
                                  const float* xr, int64_t ldr, const float* att, const float* bias, float* out,
                                  int64_t ldo, float* m, float* rden, int64_t N, int H, int C, float slope,
                                  const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                                  rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "gatv2_fwd")) return rc;
  if (!head_width_supported(C)) return fail_head_width("gatv2_fwd", C);
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !xl || !xr || !att || !out) return fail(RGBX_E_ARG, "gatv2_fwd: null pointer");
  if ((m == nullptr) != (rden == nullptr)) return fail(RGBX_E_ARG, "gatv2_fwd: m and rden go together");
  if (seed && !m) return fail(RGBX_E_ARG, "gatv2_fwd: training mode saves m and rden");
  const int64_t F = (int64_t)H * C;
  if (ldl < F || ldr < F || ldo < F) return fail(RGBX_E_ARG, "gatv2_fwd: leading dimension < H*C");
  if (!aligned_to({xl, xr, att, bias, out, m, rden}, 4))
    return fail(RGBX_E_ALIGN, "gatv2_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 2, &sd, "gatv2_fwd")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "gatv2_fwd")) return rc;
  const int vec = pick_vec(C, {xl, xr, att, bias, out, sd.pacc}, {ldl, ldr, ldo});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "gatv2_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_ATTN_DISPATCH(gatv2_fwd_kernel, row_grid, N, rowptr, col, xl, ldl, xr, ldr, att, bias, out, ldo, m, rden,
                     n_items, slope, L, sd, rng);
  if (sd.threshold > 0) RGBX_ATTN_FWD_COMBINE(true, bias, out, ldo, m, rden);
  RGBX_CHECK_LAUNCH("gatv2_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gatv2_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* xl, int64_t ldl,
                                      const float* xr, int64_t ldr, const float* att, const float* m,
                                      const float* rden, const float* out, int64_t ldo, const float* bias,
                                      const float* gout, int64_t ldg, float* nodeq, float* g_xr, int64_t ldgr,
                                      float* g_att, float* att_partial, int64_t n_att_partial, int64_t N, int H, int C,
                                      float slope, const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                                      rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "gatv2_bwd_dst")) return rc;
  if (!head_width_supported(C)) return fail_head_width("gatv2_bwd_dst", C);
  if (!g_att) return fail(RGBX_E_ARG, "gatv2_bwd_dst: null pointer");
  const int64_t F = (int64_t)H * C;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    RGBX_HIP(hipMemsetAsync(g_att, 0, F * sizeof(float), s));
    return RGBX_OK;
  }
  if (!rowptr || !col || !xl || !xr || !att || !m || !rden || !out || !gout || !nodeq || !g_xr || !att_partial)
    return fail(RGBX_E_ARG, "gatv2_bwd_dst: null pointer");
  if (ldl < F || ldr < F || ldo < F || ldg < F || ldgr < F)
    return fail(RGBX_E_ARG, "gatv2_bwd_dst: leading dimension < H*C");
  if (!aligned_to({nodeq}, 8)) return fail(RGBX_E_ALIGN, "gatv2_bwd_dst: nodeq must be 8-byte aligned");
  if (!aligned_to({xl, xr, att, m, rden, out, bias, gout, g_xr, g_att, att_partial}, 4))
    return fail(RGBX_E_ALIGN, "gatv2_bwd_dst: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 0, &sd, "gatv2_bwd_dst")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "gatv2_bwd_dst")) return rc;
  const int64_t n_rec = att_records(N, split);
  if (n_att_partial < n_rec * F)
    return fail(RGBX_E_WS, "gatv2_bwd_dst: %lld partial floats < %lld", (long long)n_att_partial,
                (long long)(n_rec * F));
  const int vec = pick_vec(C, {xl, xr, att, out, bias, gout, g_xr, att_partial, sd.pacc}, {ldl, ldr, ldo, ldg, ldgr});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "gatv2_bwd_dst")) return rc;
  const int grid = att_grid(N);
  float2* nq = reinterpret_cast<float2*>(nodeq);
  RGBX_ATTN_DISPATCH(gatv2_bwd_dst_kernel, att_grid, N, rowptr, col, xl, ldl, xr, ldr, att, m, rden, out, ldo, bias,
                     gout, ldg, nq, g_xr, ldgr, att_partial + (chunk_pass ? (int64_t)grid * F : 0), n_items, slope, L,
                     sd, rng);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_xr, ldgr, F, 0);
  RGBX_CHECK_LAUNCH("gatv2_bwd_dst_kernel");
  gatv2_att_reduce_kernel<<<(int)cdiv(F, 16), 256, 0, s>>>(att_partial, n_rec, (int)F, g_att);
  RGBX_CHECK_LAUNCH("gatv2_att_reduce_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gatv2_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                      const float* xl, int64_t ldl, const float* xr, int64_t ldr, const float* att,
                                      const float* nodeq, const float* gout, int64_t ldg, float* g_xl, int64_t ldgl,
                                      int64_t N, int H, int C, float slope, const uint32_t* seed, float p_drop,
                                      const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "gatv2_bwd_src")) return rc;
  if (!head_width_supported(C)) return fail_head_width("gatv2_bwd_src", C);
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !xl || !xr || !att || !nodeq || !gout || !g_xl)
    return fail(RGBX_E_ARG, "gatv2_bwd_src: null pointer");
  if (seed && !t2f) return fail(RGBX_E_ARG, "gatv2_bwd_src: training mode needs the slot map");
  const int64_t F = (int64_t)H * C;
  if (ldl < F || ldr < F || ldg < F || ldgl < F) return fail(RGBX_E_ARG, "gatv2_bwd_src: leading dimension < H*C");
  if (!aligned_to({nodeq}, 8)) return fail(RGBX_E_ALIGN, "gatv2_bwd_src: nodeq must be 8-byte aligned");
  if (!aligned_to({xl, xr, att, gout, g_xl}, 4))
    return fail(RGBX_E_ALIGN, "gatv2_bwd_src: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 0, &sd, "gatv2_bwd_src")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "gatv2_bwd_src")) return rc;
  const int vec = pick_vec(C, {xl, xr, att, gout, g_xl, sd.pacc}, {ldl, ldr, ldg, ldgl});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "gatv2_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float2* nq = reinterpret_cast<const float2*>(nodeq);
  RGBX_ATTN_DISPATCH(gatv2_bwd_src_kernel, row_grid, N, rowptr_t, col_t, t2f, xl, ldl, xr, ldr, att, nq, gout, ldg,
                     g_xl, ldgl, n_items, slope, L, sd, rng);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_xl, ldgl, F, 0);
  RGBX_CHECK_LAUNCH("gatv2_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gatv2_draws_u8(const uint32_t* seed, int64_t nnz, int H, float p_drop, uint8_t* keep,
                                   rgbx_stream_t stream) {
  if (nnz < 0 || H <= 0) return fail(RGBX_E_ARG, "gatv2_draws: bad size");
  if (nnz == 0) return RGBX_OK;
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "gatv2_draws: E' exceeds int32");
  if (!seed || !keep) return fail(RGBX_E_ARG, "gatv2_draws: null pointer");
  gatv2_draws_kernel<<<capped_grid(nnz, 256), 256, 0, (hipStream_t)stream>>>(seed, nnz, H, p_drop, keep);
  RGBX_CHECK_LAUNCH("gatv2_draws_kernel");
  return RGBX_OK;
}
