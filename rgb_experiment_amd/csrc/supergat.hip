// SuperGAT ("MX" attention): fused per-edge dot product + edge-softmax + aggregation, the self-supervised
// link-prediction loss over sampled edges and sampled non-edges, and their backward, for gfx950. Stands in for
// SuperGATConv.forward / message / get_attention / negative_sampling [PyG] behind reference models/supergat.py.
//
// For an edge j -> i and head h (lane layout as in gat.hip, one wave per CSR row):
//   d = <h_i, h_j>,  s = (<h_j, att_l> + <h_i, att_r>) * sigmoid(d),  e = leaky_relu(s),  alpha = softmax_i(e)
// Unlike GAT's the score is no sum of two per-node scalars: every gathered row is multiplied with the target's row,
// which stays in registers, by a cross-lane reduction over the head's lanes. The same products are the logits of the
// link-prediction loss, mean_h d, so the positive half of that loss is formed in the aggregation pass itself.
//
// Randomness is counter-based: the attention-dropout keep of (forward CSR slot, head), the positive keep of a slot
// and the negative pairs are hashes of a 64-bit seed that lives on the device. The backward recomputes them; no
// [E', H] tensor is ever written.
#include "attn_common.h"

namespace rgbx {
namespace {

// Training-mode state of one forward: the attention dropout's, and edge_sample_ratio beside it.
struct SgatRng : AttnRng {
  float pos_ratio;
};

constexpr uint32_t kStreamDrop = 0x243F6A88u, kStreamPos = 0x85A308D3u, kStreamNegU = 0x13198A2Eu,
                   kStreamNegV = 0x03707344u;

// mix32 / draw32 / unit24: rgbx_rng.h; drop_keep<kStreamDrop>: attn_common.h

__device__ __forceinline__ bool pos_keep(uint32_t s0, uint32_t s1, int slot, float ratio) {
  return unit24(draw32(s0, s1, kStreamPos, (uint32_t)slot, 0u)) < ratio;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// Sum over the G lanes of a neighbour group; every lane of the group ends with the total.
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// This lane's share of <a, b> over the head chunks OTHER than `hbase`: layouts whose heads do not fit one lane group
// (H > HPC, e.g. 8 x 40) need it for the loss logit, which is the mean over ALL heads.
template <int VEC>
__device__ __forceinline__ float other_chunks_dot(const float* __restrict__ a, const float* __restrict__ b,
                                                  const GatLayout& L, int hbase, int hl, int ch) {
  float s = 0.f;
  for (int hb = 0; hb < L.H; hb += L.HPC) {
    const int head = hb + hl;
    if (hb == hbase || hl >= L.HPC || head >= L.H || ch >= L.C) continue;
    float x[VEC], y[VEC];
    load_vec<VEC>(x, a + head * L.C + ch);
    load_vec<VEC>(y, b + head * L.C + ch);
    s += dot_vec<VEC>(x, y);
  }
  return s;
}

// Block-wide (sum, count) of the loss terms -> one record per workgroup; every thread of the block calls it.
__device__ __forceinline__ void block_loss_store(float lsum, float lcnt, float2* __restrict__ part) {
  __shared__ float red[2][4];
  for (int off = 32; off > 0; off >>= 1) {
    lsum += __shfl_xor(lsum, off);
    lcnt += __shfl_xor(lcnt, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = lsum;
    red[1][wave] = lcnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f, c = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      s += red[0][w];
      c += red[1][w];
    }
    part[blockIdx.x] = make_float2(s, c);
  }
}

// ------------------------------------------------------------------------------------------
// Forward. TRAIN: attention dropout in the accumulation (the normaliser stays that of the undropped softmax) and
// the positive half of the link-prediction loss: softplus(-mean_h d) of every kept slot, summed per workgroup.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
sgat_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ hfeat,
                int64_t ldh, const float* __restrict__ att_l, const float* __restrict__ att_r,
                const float* __restrict__ bias, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                float* __restrict__ rden_out, int N, float slope, const GatLayout L, const AttnSplit sp,
                const SgatRng rng, float2* __restrict__ loss_part) {
  constexpr int U = TRAIN ? 3 : 4;  // neighbour rows in flight per lane group
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool multi = L.H > L.HPC;
  const float inv_h = 1.0f / (float)L.H;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }
  float lsum = 0.f, lcnt = 0.f;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    const float* hrow = hfeat + (int64_t)row * ldh;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float hi[VEC], atl[VEC];
      float ar = 0.f;
      {
        float atr[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) hi[i] = atl[i] = atr[i] = 0.f;
        if (active) {
          load_vec<VEC>(hi, hrow + cofs);
          load_vec<VEC>(atl, att_l + cofs);
          load_vec<VEC>(atr, att_r + cofs);
        }
        ar = head_sum(dot_vec<VEC>(hi, atr), L.LPH);
      }
      float m = kNegBig, l = 0.f;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

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
            if (ok[u]) load_vec<VEC>(v[u], hfeat + (int64_t)src * ldh + cofs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float dl = dot_vec<VEC>(v[u], hi);  // this lane's share of <h_i, h_j>
            const float d = head_sum(dl, L.LPH);
            const float al = head_sum(dot_vec<VEC>(v[u], atl), L.LPH);
            const float s = (al + ar) * sigmoidf_(d);
            const float e = s > 0.f ? s : slope * s;
            const float mn = ok[u] ? fmaxf(m, e) : m;
            const float sc = expf(m - mn);
            const float p = ok[u] ? expf(e - mn) : 0.f;
            l = fmaf(l, sc, p);
            float pk = p;
            if constexpr (TRAIN)
              pk = drop_keep<kStreamDrop>(s0, s1, base + idx, head, rng.p_drop) ? p * rng.inv_keep : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc[i], sc, pk * v[u][i]);
            m = mn;
            if constexpr (TRAIN) {
              if (hbase == 0) {  // the loss logit of the slot, once: mean over ALL heads of d
                float zl = dl;
                if (multi && idx < n)
                  zl += other_chunks_dot<VEC>(hrow, hfeat + (int64_t)__shfl(mycol, idx & 63) * ldh, L, hbase, hl, ch);
                const float z = group_sum(zl, L.G) * inv_h;
                if (t == 0 && idx < n && pos_keep(s0, s1, base + idx, rng.pos_ratio)) {
                  lsum += softplusf_(-z);
                  lcnt += 1.f;
                }
              }
            }
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
          if (ch == 0) {
            m_out[(int64_t)row * L.H + head] = l > 0.f ? m : 0.f;
            rden_out[(int64_t)row * L.H + head] = rd;
          }
        }
      }
    }
  }
  if constexpr (TRAIN) block_loss_store(lsum, lcnt, loss_part);
}

// Per-workgroup (sum, count) records added in record order, in double: stats[0] = sum, stats[1] = count.
__global__ void __launch_bounds__(256)
sgat_loss_finish_kernel(const float2* __restrict__ part, int n, double* __restrict__ stats) {
  __shared__ double sh[2][256];
  const int t = threadIdx.x;
  double s = 0.0, c = 0.0;
  for (int b = t; b < n; b += 256) {
    const float2 r = part[b];
    s += (double)r.x;
    c += (double)r.y;
  }
  sh[0][t] = s;
  sh[1][t] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    stats[0] = sh[0][0];
    stats[1] = sh[1][0];
  }
}

// ------------------------------------------------------------------------------------------
// Per-edge gradient terms shared by the two backward passes. With kappa = keep / (1 - p) (1 in eval mode):
//   g_e = alpha (kappa <gout_i, h_j> - <gout_i, out_i>),  g_s = g_e lrelu'(s),  g_t = g_s sigma(d),
//   g_d = g_s t sigma (1 - sigma)  [+ (sigma(z) - 1) / H * gl for a kept positive slot, z = mean_h d]
struct EdgeGrad {
  float alpha_k;  // alpha * kappa: the weight of gout_i in g_h_j
  float g_t;
  float g_d;
};

__device__ __forceinline__ EdgeGrad edge_grad(float d, float t, float dal, float shift, float dsum, float kappa,
                                              float slope, bool ok) {
  const float sg = sigmoidf_(d);
  const float s = t * sg;
  const float e = s > 0.f ? s : slope * s;
  const float alpha = ok ? expf(e - shift) : 0.f;
  const float g_s = alpha * (kappa * dal - dsum) * (s > 0.f ? 1.f : slope);
  EdgeGrad r;
  r.alpha_k = alpha * kappa;
  r.g_t = g_s * sg;
  r.g_d = g_s * t * sg * (1.f - sg);
  return r;
}

// Backward, target side, over the forward CSR (row = target i):
//   g_hfeat[i,h,:] = sum_p g_d_p h_j + (sum_p g_t_p) att_r[h,:],   g_ar[i,h] = sum_p g_t_p
// and the per-(target, head) record nodeq = (<h_i, att_r>, m - log(rden), <gout_i, out_i - bias>, 0) of the source pass.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
sgat_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ hfeat,
                    int64_t ldh, const float* __restrict__ att_l, const float* __restrict__ att_r,
                    const float* __restrict__ m_in, const float* __restrict__ rden_in, const float* __restrict__ out,
                    int64_t ldo, const float* __restrict__ bias, const float* __restrict__ gout, int64_t ldg,
                    float4* __restrict__ nodeq, float* __restrict__ g_hfeat, int64_t ldgh, float* __restrict__ g_ar,
                    int N, float slope, const GatLayout L, const AttnSplit sp, const SgatRng rng,
                    const float* __restrict__ gl) {
  constexpr int U = 3;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool multi = L.H > L.HPC;
  const float inv_h = 1.0f / (float)L.H;
  uint32_t s0 = 0, s1 = 0;
  float glv = 0.f;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
    glv = gl[0] * inv_h;
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    // a hub row: its record here, its sums by the chunk + combine kernels
    const bool hub = !row_item<CHUNK>(rowptr, sp, item, row, start, end);
    const float* hrow = hfeat + (int64_t)row * ldh;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float hi[VEC], go[VEC], atl[VEC];
      float ar = 0.f, shift = 0.f, dsum = 0.f;
      {
        float atr[VEC], o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) hi[i] = go[i] = atl[i] = atr[i] = o[i] = 0.f;
        if (active) {
          load_vec<VEC>(hi, hrow + cofs);
          load_vec<VEC>(go, gout + (int64_t)row * ldg + cofs);
          load_vec<VEC>(o, out + (int64_t)row * ldo + cofs);
          load_vec<VEC>(atl, att_l + cofs);
          load_vec<VEC>(atr, att_r + cofs);
          if (bias) {  // `out` was stored with the bias added: the softmax Jacobian needs the bare aggregate
            float bv[VEC];
            load_vec<VEC>(bv, bias + cofs);
#pragma unroll
            for (int i = 0; i < VEC; ++i) o[i] -= bv[i];
          }
          shift = softmax_shift(m_in[(int64_t)row * L.H + head], rden_in[(int64_t)row * L.H + head]);
        }
        ar = head_sum(dot_vec<VEC>(hi, atr), L.LPH);
        dsum = head_sum(dot_vec<VEC>(go, o), L.LPH);
      }
      if constexpr (!CHUNK) {
        if (g == 0 && active && ch == 0) nodeq[(int64_t)row * L.H + head] = make_float4(ar, shift, dsum, 0.f);
        if (hub) continue;
      }
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      float acc_t = 0.f;

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
            if (ok[u]) load_vec<VEC>(v[u], hfeat + (int64_t)src * ldh + cofs);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float dl = dot_vec<VEC>(v[u], hi);
            const float d = head_sum(dl, L.LPH);
            const float al = head_sum(dot_vec<VEC>(v[u], atl), L.LPH);
            const float dal = head_sum(dot_vec<VEC>(v[u], go), L.LPH);
            float kappa = 1.f;
            if constexpr (TRAIN)
              kappa = drop_keep<kStreamDrop>(s0, s1, base + idx, head, rng.p_drop) ? rng.inv_keep : 0.f;
            const EdgeGrad eg = edge_grad(d, al + ar, dal, shift, dsum, kappa, slope, ok[u]);
            float g_d = eg.g_d;
            if constexpr (TRAIN) {
              float zl = dl;
              if (multi && idx < n)
                zl += other_chunks_dot<VEC>(hrow, hfeat + (int64_t)__shfl(mycol, idx & 63) * ldh, L, hbase, hl, ch);
              const float z = group_sum(zl, L.G) * inv_h;
              if (ok[u] && pos_keep(s0, s1, base + idx, rng.pos_ratio)) g_d += (sigmoidf_(z) - 1.f) * glv;
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(g_d, v[u][i], acc[i]);
            acc_t += eg.g_t;
          }
        }
      }
      for (int off = 32; off >= L.G; off >>= 1) {
        acc_t += __shfl_xor(acc_t, off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
      if (g == 0 && active) {
        if constexpr (CHUNK) {
          store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
          if (ch == 0) sp.p0[(int64_t)item * L.H + head] = acc_t;
        } else {
          float atr[VEC];
          load_vec<VEC>(atr, att_r + cofs);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc_t, atr[i], acc[i]);
          store_vec<VEC>(g_hfeat + (int64_t)row * ldgh + cofs, acc);
          if (ch == 0) g_ar[(int64_t)row * L.H + head] = acc_t;
        }
      }
    }
  }
}

// Backward, source side, over the TRANSPOSED CSR (row = source j, col_t[p] = target i, t2f[p] = the forward slot of
// the same edge, which keys its random decisions):
//   g_hfeat[j,h,:] += sum_p (alpha~_p gout_i + g_d_p h_i) + (sum_p g_t_p) att_l[h,:],   g_al[j,h] = sum_p g_t_p
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
sgat_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ t2f,
                    const float* __restrict__ hfeat, int64_t ldh, const float* __restrict__ att_l,
                    const float4* __restrict__ nodeq, const float* __restrict__ gout, int64_t ldg,
                    float* __restrict__ g_hfeat, int64_t ldgh, float* __restrict__ g_al, int N, float slope,
                    const GatLayout L, const AttnSplit sp, const SgatRng rng, const float* __restrict__ gl) {
  constexpr int U = 2;  // two rows (h_i, gout_i) are gathered per edge
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool multi = L.H > L.HPC;
  const float inv_h = 1.0f / (float)L.H;
  uint32_t s0 = 0, s1 = 0;
  float glv = 0.f;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
    glv = gl[0] * inv_h;
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    const float* hrow = hfeat + (int64_t)row * ldh;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      float hj[VEC], atl[VEC], acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) hj[i] = atl[i] = acc[i] = 0.f;
      if (active) {
        load_vec<VEC>(hj, hrow + cofs);
        load_vec<VEC>(atl, att_l + cofs);
      }
      const float al = head_sum(dot_vec<VEC>(hj, atl), L.LPH);
      float acc_t = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col_t[base + lane] : 0;
        int myslot = 0;
        if constexpr (TRAIN) myslot = lane < n ? t2f[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float hi[U][VEC], go[U][VEC];
          float ar[U], sh[U], dsm[U];
          bool ok[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int tgt = __shfl(mycol, idx & 63);
            ok[u] = active && idx < n;
            ar[u] = sh[u] = dsm[u] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) hi[u][i] = go[u][i] = 0.f;
            if (ok[u]) {
              const float4 q = nodeq[(int64_t)tgt * L.H + head];
              ar[u] = q.x;
              sh[u] = q.y;
              dsm[u] = q.z;
              load_vec<VEC>(hi[u], hfeat + (int64_t)tgt * ldh + cofs);
              load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + cofs);
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float dl = dot_vec<VEC>(hi[u], hj);
            const float d = head_sum(dl, L.LPH);
            const float dal = head_sum(dot_vec<VEC>(go[u], hj), L.LPH);
            float kappa = 1.f;
            int slot = 0;
            if constexpr (TRAIN) {
              slot = __shfl(myslot, idx & 63);
              kappa = drop_keep<kStreamDrop>(s0, s1, slot, head, rng.p_drop) ? rng.inv_keep : 0.f;
            }
            const EdgeGrad eg = edge_grad(d, al + ar[u], dal, sh[u], dsm[u], kappa, slope, ok[u]);
            float g_d = eg.g_d;
            if constexpr (TRAIN) {
              float zl = dl;
              if (multi && idx < n)
                zl += other_chunks_dot<VEC>(hrow, hfeat + (int64_t)__shfl(mycol, idx & 63) * ldh, L, hbase, hl, ch);
              const float z = group_sum(zl, L.G) * inv_h;
              if (ok[u] && pos_keep(s0, s1, slot, rng.pos_ratio)) g_d += (sigmoidf_(z) - 1.f) * glv;
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(eg.alpha_k, go[u][i], fmaf(g_d, hi[u][i], acc[i]));
            acc_t += eg.g_t;
          }
        }
      }
      for (int off = 32; off >= L.G; off >>= 1) {
        acc_t += __shfl_xor(acc_t, off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
      if (g == 0 && active) {
        if constexpr (CHUNK) {
          store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
          if (ch == 0) sp.p0[(int64_t)item * L.H + head] = acc_t;
        } else {
          float prev[VEC];
          load_vec<VEC>(prev, g_hfeat + (int64_t)row * ldgh + cofs);  // the target-side pass's share
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = prev[i] + fmaf(acc_t, atl[i], acc[i]);
          store_vec<VEC>(g_hfeat + (int64_t)row * ldgh + cofs, acc);
          if (ch == 0) g_al[(int64_t)row * L.H + head] = acc_t;
        }
      }
    }
  }
}

// One wave per hub row of either backward pass: chunk sums added in chunk order, then the score term
// (sum g_t) att[h,:]; `accumulate`: on top of what g_hfeat holds (the source pass runs second).
template <int VEC>
__global__ void __launch_bounds__(256)
sgat_bwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                        const float* __restrict__ att, float* __restrict__ g_hfeat, int64_t ldgh,
                        float* __restrict__ g_a, int accumulate, const GatLayout L, const AttnSplit sp) {
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      if (!(g == 0 && hl < L.HPC && head < L.H && ch < L.C)) continue;
      const int cofs = head * L.C + ch;
      float acc[VEC], av[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      float as = 0.f;
      for (int c = c0; c < c1; ++c) {
        float a2[VEC];
        load_vec<VEC>(a2, sp.pacc + (int64_t)c * F + cofs);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += a2[i];
        as += sp.p0[(int64_t)c * L.H + head];
      }
      load_vec<VEC>(av, att + cofs);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(as, av[i], acc[i]);
      if (accumulate) {
        float prev[VEC];
        load_vec<VEC>(prev, g_hfeat + (int64_t)row * ldgh + cofs);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += prev[i];
      }
      store_vec<VEC>(g_hfeat + (int64_t)row * ldgh + cofs, acc);
      if (ch == 0) g_a[(int64_t)row * L.H + head] = as;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Negative sampler: slot k draws up to `redraws` candidate pairs (u, v) and keeps the first with u != v that is not in
// the sorted key array of the undirected edge set (keys u * N + v; both directions are in the array).
__global__ void __launch_bounds__(256)
sgat_sample_neg_kernel(const uint64_t* __restrict__ keys, int64_t n_keys, int64_t N, const uint32_t* __restrict__ seed,
                       int64_t n_neg, int redraws, int64_t* __restrict__ neg, uint8_t* __restrict__ valid) {
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_neg; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t u = 0, v = 0;
    bool found = false;
    for (int r = 0; r < redraws && !found; ++r) {
      u = (int64_t)(((uint64_t)draw32(s0, s1, kStreamNegU, (uint32_t)k, (uint32_t)r) * (uint64_t)N) >> 32);
      v = (int64_t)(((uint64_t)draw32(s0, s1, kStreamNegV, (uint32_t)k, (uint32_t)r) * (uint64_t)N) >> 32);
      if (u == v) continue;
      const uint64_t key = (uint64_t)u * (uint64_t)N + (uint64_t)v;
      int64_t lo = 0, hi = n_keys;  // first index with keys[idx] >= key
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
      }
      found = !(lo < n_keys && keys[lo] == key);
    }
    neg[k] = found ? u : 0;
    neg[n_neg + k] = found ? v : 0;
    valid[k] = found ? 1 : 0;
  }
}

// Negative half of the loss: logit z = <h_u, h_v> / H over the whole row, term softplus(z). LP lanes per pair.
// BWD: g_h_u += g_z h_v, g_h_v += g_z h_u with g_z = sigmoid(z) gl / H, by float atomics (pairs share rows).
template <int VEC, bool BWD>
__global__ void __launch_bounds__(256)
sgat_neg_kernel(const float* __restrict__ hfeat, int64_t ldh, const int64_t* __restrict__ neg,
                const uint8_t* __restrict__ valid, int64_t n_neg, int F, int LP, float inv_h,
                float2* __restrict__ part, const float* __restrict__ gl, float* __restrict__ g_hfeat, int64_t ldgh) {
  const int lane = threadIdx.x & 63;
  const int PP = kWave / LP;
  const int t = lane % LP;
  const int wpb = blockDim.x >> 6;
  float lsum = 0.f, lcnt = 0.f;
  for (int64_t p0 = ((int64_t)blockIdx.x * wpb + (threadIdx.x >> 6)) * PP; p0 < n_neg;
       p0 += (int64_t)gridDim.x * wpb * PP) {
    const int64_t pr = p0 + lane / LP;
    const bool ok = pr < n_neg && (!valid || valid[pr]);
    const int64_t u = ok ? neg[pr] : 0, v = ok ? neg[n_neg + pr] : 0;
    float zl = 0.f;
    if (ok) {
      for (int c = t * VEC; c < F; c += LP * VEC) {
        float a[VEC], b[VEC];
        load_vec<VEC>(a, hfeat + u * ldh + c);
        load_vec<VEC>(b, hfeat + v * ldh + c);
        zl += dot_vec<VEC>(a, b);
      }
    }
    const float z = group_sum(zl, LP) * inv_h;
    if constexpr (!BWD) {
      if (ok && t == 0) {
        lsum += softplusf_(z);
        lcnt += 1.f;
      }
    } else {
      if (ok) {
        const float gz = sigmoidf_(z) * gl[0] * inv_h;
        for (int c = t * VEC; c < F; c += LP * VEC) {
          float a[VEC], b[VEC];
          load_vec<VEC>(a, hfeat + u * ldh + c);
          load_vec<VEC>(b, hfeat + v * ldh + c);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            atomicAdd(g_hfeat + u * ldgh + c + i, gz * b[i]);
            atomicAdd(g_hfeat + v * ldgh + c + i, gz * a[i]);
          }
        }
      }
    }
  }
  if constexpr (!BWD) block_loss_store(lsum, lcnt, part);
}

// The random decisions of a training forward, written out for inspection (tests): pos[p] and drop[p, h] in forward
// CSR slot order.
__global__ void __launch_bounds__(256)
sgat_draws_kernel(const uint32_t* __restrict__ seed, int64_t nnz, int H, float p_drop, float pos_ratio,
                  uint8_t* __restrict__ pos, uint8_t* __restrict__ drop) {
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    pos[p] = pos_keep(s0, s1, (int)p, pos_ratio) ? 1 : 0;
    for (int h = 0; h < H; ++h) drop[p * H + h] = drop_keep<kStreamDrop>(s0, s1, (int)p, h, p_drop) ? 1 : 0;
  }
}

void launch_sgat_bwd_combine(int vec, const rgbx_row_split_t* split, const float* att, float* g_hfeat, int64_t ldgh,
                             float* g_a, int accumulate, const GatLayout& L, const AttnSplit& sd, hipStream_t s) {
  RGBX_VEC_SWITCH(vec, sgat_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(split->n_long,
                  split->long_row, split->long_chunk_ptr, att, g_hfeat, ldgh, g_a, accumulate, L, sd));
}

int sgat_rng(const uint32_t* seed, float p_drop, float pos_ratio, bool train, SgatRng* rng, const char* name) {
  *rng = SgatRng{{seed, p_drop, 1.0f}, pos_ratio};
  if (!train) return RGBX_OK;
  if (!(p_drop >= 0.f && p_drop < 1.f) || !(pos_ratio >= 0.f && pos_ratio <= 1.f))
    return fail(RGBX_E_ARG, "%s: dropout must be in [0, 1) and edge_sample_ratio in [0, 1]", name);
  rng->inv_keep = 1.0f / (1.0f - p_drop);
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_supergat_supported(int H, int C) {
  return H > 0 && head_width_supported(C);
}

extern "C" int rgbx_supergat_loss_records(int64_t N, const rgbx_row_split_t* split, int64_t* count) {
  if (!count || N < 0) return fail(RGBX_E_ARG, "supergat_loss_records: bad argument");
  *count = row_grid(N) + (split && split->threshold > 0 && split->n_chunks > 0 ? row_grid(split->n_chunks) : 0);
  return RGBX_OK;
}

extern "C" int rgbx_supergat_aggregate_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat,
                                               int64_t ldh, const float* att_l, const float* att_r,
                                               const float* bias, float* out, int64_t ldo, float* m, float* rden,
                                               int64_t N, int H, int C, float slope, const uint32_t* seed,
                                               float p_drop, float pos_ratio, float* loss_records,
                                               int64_t n_loss_records, double* pos_stats,
                                               const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "supergat_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !hfeat || !att_l || !att_r || !out || !m || !rden)
    return fail(RGBX_E_ARG, "supergat_fwd: null pointer");
  if (ldh < (int64_t)H * C || ldo < (int64_t)H * C) return fail(RGBX_E_ARG, "supergat_fwd: leading dimension < H*C");
  const bool train = seed != nullptr;
  if (train && (!loss_records || !pos_stats)) return fail(RGBX_E_ARG, "supergat_fwd: training mode needs loss buffers");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 2, &sd, "supergat_fwd")) return rc;
  SgatRng rng;
  if (int rc = sgat_rng(seed, p_drop, pos_ratio, train, &rng, "supergat_fwd")) return rc;
  const int grid = row_grid(N);
  const int grid_c = sd.threshold > 0 ? row_grid(split->n_chunks) : 0;
  if (train && n_loss_records < (int64_t)grid + grid_c)
    return fail(RGBX_E_WS, "supergat_fwd: %lld loss records < %lld", (long long)n_loss_records,
                (long long)grid + grid_c);
  if (train && !aligned16(loss_records)) return fail(RGBX_E_ALIGN, "supergat_fwd: loss records must be 16-byte aligned");
  const int vec = pick_vec(C, {hfeat, out, att_l, att_r, bias, sd.pacc}, {ldh, ldo});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "supergat_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  float2* part = reinterpret_cast<float2*>(loss_records);
  RGBX_ATTN_DISPATCH(sgat_fwd_kernel, row_grid, N, rowptr, col, hfeat, ldh, att_l, att_r, bias, out, ldo, m, rden,
                     n_items, slope, L, sd, rng, part + (chunk_pass && train ? grid : 0));
  if (sd.threshold > 0) RGBX_ATTN_FWD_COMBINE(true, bias, out, ldo, m, rden);
  RGBX_CHECK_LAUNCH("sgat_fwd_kernel");
  if (train) {
    sgat_loss_finish_kernel<<<1, 256, 0, s>>>(part, grid + grid_c, pos_stats);
    RGBX_CHECK_LAUNCH("sgat_loss_finish_kernel");
  }
  return RGBX_OK;
}

extern "C" int rgbx_supergat_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* hfeat, int64_t ldh,
                                         const float* att_l, const float* att_r, const float* m, const float* rden,
                                         const float* out, int64_t ldo, const float* bias, const float* gout,
                                         int64_t ldg, float* nodeq, float* g_hfeat, int64_t ldgh, float* g_ar,
                                         int64_t N, int H, int C, float slope, const uint32_t* seed, float p_drop,
                                         float pos_ratio, const float* gl, const rgbx_row_split_t* split,
                                         rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "supergat_bwd_dst")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !hfeat || !att_l || !att_r || !m || !rden || !out || !gout || !nodeq || !g_hfeat || !g_ar)
    return fail(RGBX_E_ARG, "supergat_bwd_dst: null pointer");
  const int64_t F = (int64_t)H * C;
  if (ldh < F || ldo < F || ldg < F || ldgh < F) return fail(RGBX_E_ARG, "supergat_bwd_dst: leading dimension < H*C");
  if (!aligned16(nodeq)) return fail(RGBX_E_ALIGN, "supergat_bwd_dst: nodeq must be 16-byte aligned");
  const bool train = seed != nullptr;
  if (train && !gl) return fail(RGBX_E_ARG, "supergat_bwd_dst: training mode needs the loss gradient scalar");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 1, &sd, "supergat_bwd_dst")) return rc;
  SgatRng rng;
  if (int rc = sgat_rng(seed, p_drop, pos_ratio, train, &rng, "supergat_bwd_dst")) return rc;
  const int vec = pick_vec(C, {hfeat, out, gout, g_hfeat, att_l, att_r, bias, sd.pacc}, {ldh, ldo, ldg, ldgh});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "supergat_bwd_dst")) return rc;
  hipStream_t s = (hipStream_t)stream;
  float4* nq = reinterpret_cast<float4*>(nodeq);
  RGBX_ATTN_DISPATCH(sgat_bwd_dst_kernel, row_grid, N, rowptr, col, hfeat, ldh, att_l, att_r, m, rden, out, ldo, bias,
                     gout, ldg, nq, g_hfeat, ldgh, g_ar, n_items, slope, L, sd, rng, gl);
  if (sd.threshold > 0) launch_sgat_bwd_combine(vec, split, att_r, g_hfeat, ldgh, g_ar, 0, L, sd, s);
  RGBX_CHECK_LAUNCH("sgat_bwd_dst_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_supergat_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                         const float* hfeat, int64_t ldh, const float* att_l, const float* nodeq,
                                         const float* gout, int64_t ldg, float* g_hfeat, int64_t ldgh, float* g_al,
                                         int64_t N, int H, int C, float slope, const uint32_t* seed, float p_drop,
                                         float pos_ratio, const float* gl, const rgbx_row_split_t* split,
                                         rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "supergat_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !hfeat || !att_l || !nodeq || !gout || !g_hfeat || !g_al)
    return fail(RGBX_E_ARG, "supergat_bwd_src: null pointer");
  const int64_t F = (int64_t)H * C;
  if (ldh < F || ldg < F || ldgh < F) return fail(RGBX_E_ARG, "supergat_bwd_src: leading dimension < H*C");
  if (!aligned16(nodeq)) return fail(RGBX_E_ALIGN, "supergat_bwd_src: nodeq must be 16-byte aligned");
  const bool train = seed != nullptr;
  if (train && (!gl || !t2f)) return fail(RGBX_E_ARG, "supergat_bwd_src: training mode needs gl and the slot map");
  AttnSplit sd;
  if (int rc = split_view(split, H, C, 1, &sd, "supergat_bwd_src")) return rc;
  SgatRng rng;
  if (int rc = sgat_rng(seed, p_drop, pos_ratio, train, &rng, "supergat_bwd_src")) return rc;
  const int vec = pick_vec(C, {hfeat, gout, g_hfeat, att_l, sd.pacc}, {ldh, ldg, ldgh});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "supergat_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float4* nq = reinterpret_cast<const float4*>(nodeq);
  RGBX_ATTN_DISPATCH(sgat_bwd_src_kernel, row_grid, N, rowptr_t, col_t, t2f, hfeat, ldh, att_l, nq, gout, ldg, g_hfeat,
                     ldgh, g_al, n_items, slope, L, sd, rng, gl);
  if (sd.threshold > 0) launch_sgat_bwd_combine(vec, split, att_l, g_hfeat, ldgh, g_al, 1, L, sd, s);
  RGBX_CHECK_LAUNCH("sgat_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_supergat_sample_negatives(const uint64_t* keys, int64_t n_keys, int64_t N, const uint32_t* seed,
                                              int64_t n_neg, int redraws, int64_t* neg, uint8_t* valid,
                                              rgbx_stream_t stream) {
  if (n_neg < 0 || n_keys < 0 || N < 0 || redraws <= 0) return fail(RGBX_E_ARG, "supergat_sample_negatives: bad size");
  if (n_neg == 0) return RGBX_OK;
  if (N < 2) return fail(RGBX_E_ARG, "supergat_sample_negatives: a pair needs two nodes");
  if (N >= INT32_MAX || n_neg >= INT32_MAX) return fail(RGBX_E_RANGE, "supergat_sample_negatives: size exceeds int32");
  if ((n_keys > 0 && !keys) || !seed || !neg || !valid) return fail(RGBX_E_ARG, "supergat_sample_negatives: null pointer");
  sgat_sample_neg_kernel<<<capped_grid(n_neg, 256), 256, 0, (hipStream_t)stream>>>(keys, n_keys, N, seed, n_neg,
                                                                                   redraws, neg, valid);
  RGBX_CHECK_LAUNCH("sgat_sample_neg_kernel");
  return RGBX_OK;
}

namespace {
int neg_layout(const float* hfeat, int64_t ldh, float* g_hfeat, int64_t ldgh, int64_t F, int* vec, int* lp) {
  *vec = pick_vec((int)F, {hfeat, g_hfeat}, {ldh, ldgh});
  *lp = std::min(kWave, pow2ceil((int)cdiv(F, *vec)));
  return RGBX_OK;
}
}  // namespace

extern "C" int rgbx_supergat_neg_loss_fwd_f32(const float* hfeat, int64_t ldh, const int64_t* neg,
                                              const uint8_t* valid, int64_t n_neg, int H, int C, float* loss_records,
                                              int64_t n_loss_records, double* neg_stats, rgbx_stream_t stream) {
  if (int rc = check_common(n_neg, H, C, "supergat_neg_loss_fwd")) return rc;
  if (!neg_stats) return fail(RGBX_E_ARG, "supergat_neg_loss_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_neg == 0) {
    RGBX_HIP(hipMemsetAsync(neg_stats, 0, 2 * sizeof(double), s));
    return RGBX_OK;
  }
  if (!hfeat || !neg || !loss_records) return fail(RGBX_E_ARG, "supergat_neg_loss_fwd: null pointer");
  const int64_t F = (int64_t)H * C;
  if (ldh < F) return fail(RGBX_E_ARG, "supergat_neg_loss_fwd: leading dimension < H*C");
  int vec, lp;
  neg_layout(hfeat, ldh, nullptr, 0, F, &vec, &lp);
  const int grid = capped_grid(n_neg, 4 * (kWave / lp));
  if (n_loss_records < grid)
    return fail(RGBX_E_WS, "supergat_neg_loss_fwd: %lld loss records < %d", (long long)n_loss_records, grid);
  float2* part = reinterpret_cast<float2*>(loss_records);
  RGBX_VEC_SWITCH(vec, sgat_neg_kernel<V, false><<<grid, 256, 0, s>>>(hfeat, ldh, neg, valid, n_neg, (int)F, lp,
                  1.0f / H, part, nullptr, nullptr, 0));
  RGBX_CHECK_LAUNCH("sgat_neg_kernel");
  sgat_loss_finish_kernel<<<1, 256, 0, s>>>(part, grid, neg_stats);
  RGBX_CHECK_LAUNCH("sgat_loss_finish_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_supergat_neg_loss_bwd_f32(const float* hfeat, int64_t ldh, const int64_t* neg,
                                              const uint8_t* valid, int64_t n_neg, int H, int C, const float* gl,
                                              float* g_hfeat, int64_t ldgh, rgbx_stream_t stream) {
  if (int rc = check_common(n_neg, H, C, "supergat_neg_loss_bwd")) return rc;
  if (n_neg == 0) return RGBX_OK;
  if (!hfeat || !neg || !gl || !g_hfeat) return fail(RGBX_E_ARG, "supergat_neg_loss_bwd: null pointer");
  const int64_t F = (int64_t)H * C;
  if (ldh < F || ldgh < F) return fail(RGBX_E_ARG, "supergat_neg_loss_bwd: leading dimension < H*C");
  int vec, lp;
  neg_layout(hfeat, ldh, g_hfeat, ldgh, F, &vec, &lp);
  const int grid = capped_grid(n_neg, 4 * (kWave / lp));
  hipStream_t s = (hipStream_t)stream;
  RGBX_VEC_SWITCH(vec, sgat_neg_kernel<V, true><<<grid, 256, 0, s>>>(hfeat, ldh, neg, valid, n_neg, (int)F, lp,
                  1.0f / H, nullptr, gl, g_hfeat, ldgh));
  RGBX_CHECK_LAUNCH("sgat_neg_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_supergat_draws_u8(const uint32_t* seed, int64_t nnz, int H, float p_drop, float pos_ratio,
                                      uint8_t* pos, uint8_t* drop, rgbx_stream_t stream) {
  if (nnz < 0 || H <= 0) return fail(RGBX_E_ARG, "supergat_draws: bad size");
  if (nnz == 0) return RGBX_OK;
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "supergat_draws: E' exceeds int32");
  if (!seed || !pos || !drop) return fail(RGBX_E_ARG, "supergat_draws: null pointer");
  sgat_draws_kernel<<<capped_grid(nnz, 256), 256, 0, (hipStream_t)stream>>>(seed, nnz, H, p_drop, pos_ratio, pos, drop);
  RGBX_CHECK_LAUNCH("sgat_draws_kernel");
  return RGBX_OK;
}
