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

#include "rgbx_common.h"
#include "rgbx_rng.h"

namespace rgbx {
namespace {

// Lane layout and host helpers: the same as gat.hip's, supergat.hip's and gatv2.hip's (a head occupies
// LPH = pow2ceil(C / VEC) consecutive lanes of VEC channels, HPC heads side by side in a group of G lanes that reads one
// neighbour row per step, NG = 64 / G rows per wave-instruction). Copied rather than shared, as gatv2.hip did: the text
// of gat.hip keys the recorded counter measurements of its kernels (bench.py KERNEL_SOURCES).
struct GatLayout {
  int H, C;
  int LPH;  // lanes per head (power of two)
  int HPC;  // heads per chunk
  int G;    // lanes per neighbour row (power of two, >= HPC * LPH)
};

constexpr float kNegBig = -1.0e30f;

template <int VEC>
__device__ __forceinline__ float dot_vec(const float (&a)[VEC], const float (&b)[VEC]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// Sum over the LPH lanes of a head; every lane of the head ends with the total.
__device__ __forceinline__ float head_sum(float v, int LPH) {
  for (int off = LPH >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

int pow2ceil(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// VEC must divide C so that a lane's channels stay inside one head.
int pick_vec(int C, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
  for (int v : {4, 2}) {
    bool ok = C % v == 0;
    for (const void* p : ptrs) ok = ok && (reinterpret_cast<uintptr_t>(p) % (v * 4) == 0);
    for (int64_t ld : lds) ok = ok && (ld % v == 0);
    if (ok) return v;
  }
  return 1;
}

int make_layout(int H, int C, int vec, GatLayout* L, const char* name) {
  const int lph = pow2ceil((C + vec - 1) / vec);
  if (lph > kWave)
    return fail(RGBX_E_SHAPE, "%s: C=%d needs %d lanes per head (> 64) at vector width %d", name, C, lph, vec);
  L->H = H;
  L->C = C;
  L->LPH = lph;
  L->HPC = std::min(H, kWave / lph);
  L->G = pow2ceil(L->HPC * lph);
  return RGBX_OK;
}

int row_grid(int64_t N) {  // one row per wave, no cap (see spmm.hip: uncapped grids balance ragged rows better)
  return (int)cdiv(N, 4);
}

int check_common(int64_t N, int H, int C, const char* name) {
  if (N < 0 || H <= 0 || C <= 0) return fail(RGBX_E_ARG, "%s: bad size", name);
  if (N >= INT32_MAX || (int64_t)H * C >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: size exceeds int32", name);
  return RGBX_OK;
}

bool aligned_to(std::initializer_list<const void*> ptrs, unsigned bytes) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % bytes) return false;
  return true;
}

struct TfSplit {
  int threshold;
  const int* chunk_row;
  const int* chunk_begin;
  const int* chunk_end;
  float* pacc;  // [n_chunks, F] (forward, target side) or [n_chunks, 2F] (source side: g_k | g_v)
  float* p0;    // [n_chunks, H]  (forward only: running max)
  float* p1;    // [n_chunks, H]  (forward only: denominator)
};

// Training-mode state of one forward: `seed` = two 32-bit words on the device (NULL: no dropout).
struct TfRng {
  const uint32_t* seed;
  float p_drop;
  float inv_keep;  // 1 / (1 - p_drop)
};

constexpr uint32_t kStreamDrop = 0xA4093822u;  // gatv2.hip's: one keep function, one inspection entry point

// mix32 / draw32 / unit24: rgbx_rng.h
__device__ __forceinline__ bool drop_keep(uint32_t s0, uint32_t s1, int slot, int head, float p) {
  return unit24(draw32(s0, s1, kStreamDrop, (uint32_t)slot, (uint32_t)head)) >= p;
}

// (m, rden) = (0, 0) is the saved state of a row without slots: shift 0, and no slot to apply it to.
__device__ __forceinline__ float softmax_shift(float m, float rden) { return rden > 0.f ? m - logf(rden) : 0.f; }

// ------------------------------------------------------------------------------------------
// Forward: online softmax (running max, denominator, rescaled accumulator) over the slots of a row, read once; per
// slot the k row is scored against the target's q row in registers and the v row is accumulated.
// TRAIN: attention dropout in the accumulation (the normaliser stays that of the undropped softmax).
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
transformer_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ q,
                       int64_t ldq, const float* __restrict__ kx, int64_t ldk, const float* __restrict__ vx,
                       int64_t ldv, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                       float* __restrict__ rden_out, int N, float scale, const GatLayout L, const TfSplit sp,
                       const TfRng rng) {
  constexpr int U = 4;  // neighbour rows in flight per lane group (k and v each)
  const int lane = threadIdx.x & 63;
  const int NG = kWave / L.G;
  const int g = lane / L.G;
  const int t = lane % L.G;
  const int hl = t / L.LPH;
  const int ch = (t % L.LPH) * VEC;
  const int wpb = blockDim.x >> 6;
  const int F = L.H * L.C;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if constexpr (CHUNK) {
      row = __builtin_amdgcn_readfirstlane(sp.chunk_row[item]);
      start = __builtin_amdgcn_readfirstlane(sp.chunk_begin[item]);
      end = __builtin_amdgcn_readfirstlane(sp.chunk_end[item]);
    } else {
      row = item;
      start = __builtin_amdgcn_readfirstlane(rowptr[row]);
      end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
      if (sp.threshold > 0 && end - start > sp.threshold) continue;  // the chunk + combine kernels own it
    }
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
              pk = drop_keep(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? p * rng.inv_keep : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc[i], sc, pk * vv[u][i]);
            m = mn;
          }
        }
      }
      // merge the NG online-softmax states
      for (int off = 32; off >= L.G; off >>= 1) {
        const float m2 = __shfl_xor(m, off);
        const float l2 = __shfl_xor(l, off);
        const float mn = fmaxf(m, m2);
        const float s1m = expf(m - mn), s2m = expf(m2 - mn);
        l = l * s1m + l2 * s2m;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float a2 = __shfl_xor(acc[i], off);
          acc[i] = acc[i] * s1m + a2 * s2m;
        }
        m = mn;
      }
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

// One wave per hub row: merge the chunk states in chunk order, normalise, store.
template <int VEC>
__global__ void __launch_bounds__(256)
transformer_fwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                               float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                               float* __restrict__ rden_out, const GatLayout L, const TfSplit sp) {
  const int lane = threadIdx.x & 63;
  const int g = lane / L.G;
  const int t = lane % L.G;
  const int hl = t / L.LPH;
  const int ch = (t % L.LPH) * VEC;
  const int wpb = blockDim.x >> 6;
  const int F = L.H * L.C;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      if (!(g == 0 && hl < L.HPC && head < L.H && ch < L.C)) continue;
      const int cofs = head * L.C + ch;
      float m = kNegBig, l = 0.f;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (int c = c0; c < c1; ++c) {
        const float m2 = sp.p0[(int64_t)c * L.H + head];
        const float l2 = sp.p1[(int64_t)c * L.H + head];
        float a2[VEC];
        load_vec<VEC>(a2, sp.pacc + (int64_t)c * F + cofs);
        const float mn = fmaxf(m, m2);
        const float s1 = expf(m - mn), s2 = expf(m2 - mn);
        l = l * s1 + l2 * s2;
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = acc[i] * s1 + a2[i] * s2;
        m = mn;
      }
      const float rd = l > 0.f ? 1.0f / (l + 1e-16f) : 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] *= rd;
      store_vec<VEC>(out + (int64_t)row * ldo + cofs, acc);
      if (m_out && ch == 0) {
        m_out[(int64_t)row * L.H + head] = l > 0.f ? m : 0.f;
        rden_out[(int64_t)row * L.H + head] = rd;
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
                           const GatLayout L, const TfSplit sp, const TfRng rng) {
  constexpr int U = 3;
  const int lane = threadIdx.x & 63;
  const int NG = kWave / L.G;
  const int g = lane / L.G;
  const int t = lane % L.G;
  const int hl = t / L.LPH;
  const int ch = (t % L.LPH) * VEC;
  const int wpb = blockDim.x >> 6;
  const int F = L.H * L.C;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    bool hub = false;
    if constexpr (CHUNK) {
      row = __builtin_amdgcn_readfirstlane(sp.chunk_row[item]);
      start = __builtin_amdgcn_readfirstlane(sp.chunk_begin[item]);
      end = __builtin_amdgcn_readfirstlane(sp.chunk_end[item]);
    } else {
      row = item;
      start = __builtin_amdgcn_readfirstlane(rowptr[row]);
      end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
      hub = sp.threshold > 0 && end - start > sp.threshold;  // record here, sums by the chunk + combine kernels
    }
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
              kappa = drop_keep(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - shift) : 0.f;
            const float de = alpha * (kappa * dal - dsum);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(de, kv[u][i], acc[i]);
          }
        }
      }
      for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
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
                           float scale, const GatLayout L, const TfSplit sp, const TfRng rng) {
  constexpr int U = 2;
  const int lane = threadIdx.x & 63;
  const int NG = kWave / L.G;
  const int g = lane / L.G;
  const int t = lane % L.G;
  const int hl = t / L.LPH;
  const int ch = (t % L.LPH) * VEC;
  const int wpb = blockDim.x >> 6;
  const int F = L.H * L.C;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if constexpr (CHUNK) {
      row = __builtin_amdgcn_readfirstlane(sp.chunk_row[item]);
      start = __builtin_amdgcn_readfirstlane(sp.chunk_begin[item]);
      end = __builtin_amdgcn_readfirstlane(sp.chunk_end[item]);
    } else {
      row = item;
      start = __builtin_amdgcn_readfirstlane(rowptr_t[row]);
      end = __builtin_amdgcn_readfirstlane(rowptr_t[row + 1]);
      if (sp.threshold > 0 && end - start > sp.threshold) continue;
    }
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
              kappa = drop_keep(s0, s1, __shfl(myslot, idx & 63), head, rng.p_drop) ? rng.inv_keep : 0.f;
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

// One wave per hub row of either backward pass: chunk sums added in chunk order. A chunk's record is `stride` floats
// wide and this output's sums start `ofs` floats into it.
template <int VEC>
__global__ void __launch_bounds__(256)
transformer_bwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                               float* __restrict__ gx, int64_t ldgx, int64_t stride, int64_t ofs, const GatLayout L,
                               const TfSplit sp) {
  const int lane = threadIdx.x & 63;
  const int g = lane / L.G;
  const int t = lane % L.G;
  const int hl = t / L.LPH;
  const int ch = (t % L.LPH) * VEC;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      if (!(g == 0 && hl < L.HPC && head < L.H && ch < L.C)) continue;
      const int cofs = head * L.C + ch;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (int c = c0; c < c1; ++c) {
        float a2[VEC];
        load_vec<VEC>(a2, sp.pacc + (int64_t)c * stride + ofs + cofs);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += a2[i];
      }
      store_vec<VEC>(gx + (int64_t)row * ldgx + cofs, acc);
    }
  }
}

int split_view(const rgbx_row_split_t* split, int H, int C, bool fwd, TfSplit* sd, const char* name) {
  *sd = TfSplit{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!split || split->threshold <= 0 || split->n_chunks <= 0) return RGBX_OK;
  if (split->n_long <= 0 || !split->chunk_row || !split->chunk_begin || !split->chunk_end || !split->long_row ||
      !split->long_chunk_ptr || !split->partial)
    return fail(RGBX_E_ARG, "%s: incomplete row-split plan", name);
  const int64_t F = (int64_t)H * C;
  sd->threshold = split->threshold;
  sd->chunk_row = split->chunk_row;
  sd->chunk_begin = split->chunk_begin;
  sd->chunk_end = split->chunk_end;
  sd->pacc = split->partial;
  if (fwd) {
    sd->p0 = sd->pacc + (int64_t)split->n_chunks * F;  // [n_chunks, H]
    sd->p1 = sd->p0 + (int64_t)split->n_chunks * H;    // [n_chunks, H]
  }
  return RGBX_OK;
}

int make_rng(const uint32_t* seed, float p_drop, TfRng* rng, const char* name) {
  *rng = TfRng{seed, p_drop, 1.0f};
  if (!seed) return RGBX_OK;
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(RGBX_E_ARG, "%s: dropout must be in [0, 1)", name);
  rng->inv_keep = 1.0f / (1.0f - p_drop);
  return RGBX_OK;
}

int check_scale(float scale, const char* name) {
  if (!(scale > 0.f) || !std::isfinite(scale)) return fail(RGBX_E_ARG, "%s: scale must be positive and finite", name);
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_transformer_supported(int H, int C) {
  if (H <= 0 || C <= 0) return 0;
  return C <= 64 || (C % 2 == 0 && C <= 128) || (C % 4 == 0 && C <= 256);
}

extern "C" int rgbx_transformer_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* q, int64_t ldq,
                                        const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                                        int64_t ldo, float* m, float* rden, int64_t N, int H, int C, float scale,
                                        const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                                        rgbx_stream_t stream) {
  if (int rc = check_common(N, H, C, "transformer_fwd")) return rc;
  if (!rgbx_transformer_supported(H, C))
    return fail(RGBX_E_SHAPE, "transformer_fwd: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)",
                C);
  if (int rc = check_scale(scale, "transformer_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !q || !k || !v || !out) return fail(RGBX_E_ARG, "transformer_fwd: null pointer");
  if ((m == nullptr) != (rden == nullptr)) return fail(RGBX_E_ARG, "transformer_fwd: m and rden go together");
  if (seed && !m) return fail(RGBX_E_ARG, "transformer_fwd: training mode saves m and rden");
  const int64_t F = (int64_t)H * C;
  if (ldq < F || ldk < F || ldv < F || ldo < F) return fail(RGBX_E_ARG, "transformer_fwd: leading dimension < H*C");
  if (!aligned_to({q, k, v, out, m, rden}, 4))
    return fail(RGBX_E_ALIGN, "transformer_fwd: float pointers must be 4-byte aligned");
  TfSplit sd;
  if (int rc = split_view(split, H, C, true, &sd, "transformer_fwd")) return rc;
  TfRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_fwd")) return rc;
  const int vec = pick_vec(C, {q, k, v, out, sd.pacc}, {ldq, ldk, ldv, ldo});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = row_grid(N);
#define RGBX_TF_FWD(V, T)                                                                                            \
  do {                                                                                                               \
    transformer_fwd_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr, col, q, ldq, k, ldk, v, ldv, out, ldo, m, rden, \
                                                             (int)N, scale, L, sd, rng);                             \
    if (sd.threshold > 0) {                                                                                          \
      transformer_fwd_kernel<V, true, T><<<row_grid(split->n_chunks), 256, 0, s>>>(                                  \
          rowptr, col, q, ldq, k, ldk, v, ldv, out, ldo, m, rden, split->n_chunks, scale, L, sd, rng);               \
      transformer_fwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(                                     \
          split->n_long, split->long_row, split->long_chunk_ptr, out, ldo, m, rden, L, sd);                          \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_TF_FWD(4, true);
    else if (vec == 2) RGBX_TF_FWD(2, true);
    else RGBX_TF_FWD(1, true);
  } else {
    if (vec == 4) RGBX_TF_FWD(4, false);
    else if (vec == 2) RGBX_TF_FWD(2, false);
    else RGBX_TF_FWD(1, false);
  }
#undef RGBX_TF_FWD
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
  if (!rgbx_transformer_supported(H, C))
    return fail(RGBX_E_SHAPE,
                "transformer_bwd_dst: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)", C);
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
  TfSplit sd;
  if (int rc = split_view(split, H, C, false, &sd, "transformer_bwd_dst")) return rc;
  TfRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_bwd_dst")) return rc;
  const int vec = pick_vec(C, {q, k, v, out, gout, g_q, sd.pacc}, {ldq, ldk, ldv, ldo, ldg, ldgq});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_bwd_dst")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = row_grid(N);
  float2* nq = reinterpret_cast<float2*>(nodeq);
#define RGBX_TF_BD(V, T)                                                                                             \
  do {                                                                                                               \
    transformer_bwd_dst_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr, col, q, ldq, k, ldk, v, ldv, m, rden, out,  \
                                                                 ldo, gout, ldg, nq, g_q, ldgq, (int)N, scale, L,    \
                                                                 sd, rng);                                           \
    if (sd.threshold > 0) {                                                                                          \
      transformer_bwd_dst_kernel<V, true, T><<<row_grid(split->n_chunks), 256, 0, s>>>(                              \
          rowptr, col, q, ldq, k, ldk, v, ldv, m, rden, out, ldo, gout, ldg, nq, g_q, ldgq, split->n_chunks, scale,  \
          L, sd, rng);                                                                                               \
      transformer_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(                                     \
          split->n_long, split->long_row, split->long_chunk_ptr, g_q, ldgq, F, 0, L, sd);                            \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_TF_BD(4, true);
    else if (vec == 2) RGBX_TF_BD(2, true);
    else RGBX_TF_BD(1, true);
  } else {
    if (vec == 4) RGBX_TF_BD(4, false);
    else if (vec == 2) RGBX_TF_BD(2, false);
    else RGBX_TF_BD(1, false);
  }
#undef RGBX_TF_BD
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
  if (!rgbx_transformer_supported(H, C))
    return fail(RGBX_E_SHAPE,
                "transformer_bwd_src: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)", C);
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
  TfSplit sd;
  if (int rc = split_view(split, H, C, false, &sd, "transformer_bwd_src")) return rc;
  TfRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "transformer_bwd_src")) return rc;
  const int vec = pick_vec(C, {q, k, v, gout, g_k, g_v, sd.pacc}, {ldq, ldk, ldv, ldg, ldgk, ldgv});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "transformer_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = row_grid(N);
  const float2* nq = reinterpret_cast<const float2*>(nodeq);
#define RGBX_TF_BS(V, T)                                                                                             \
  do {                                                                                                               \
    transformer_bwd_src_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr_t, col_t, t2f, q, ldq, k, ldk, v, ldv, nq,   \
                                                                 gout, ldg, g_k, ldgk, g_v, ldgv, (int)N, scale, L,  \
                                                                 sd, rng);                                           \
    if (sd.threshold > 0) {                                                                                          \
      transformer_bwd_src_kernel<V, true, T><<<row_grid(split->n_chunks), 256, 0, s>>>(                              \
          rowptr_t, col_t, t2f, q, ldq, k, ldk, v, ldv, nq, gout, ldg, g_k, ldgk, g_v, ldgv, split->n_chunks, scale, \
          L, sd, rng);                                                                                               \
      transformer_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(                                     \
          split->n_long, split->long_row, split->long_chunk_ptr, g_k, ldgk, 2 * F, 0, L, sd);                        \
      transformer_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(                                     \
          split->n_long, split->long_row, split->long_chunk_ptr, g_v, ldgv, 2 * F, F, L, sd);                        \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_TF_BS(4, true);
    else if (vec == 2) RGBX_TF_BS(2, true);
    else RGBX_TF_BS(1, true);
  } else {
    if (vec == 4) RGBX_TF_BS(4, false);
    else if (vec == 2) RGBX_TF_BS(2, false);
    else RGBX_TF_BS(1, false);
  }
#undef RGBX_TF_BS
  RGBX_CHECK_LAUNCH("transformer_bwd_src_kernel");
  return RGBX_OK;
}
