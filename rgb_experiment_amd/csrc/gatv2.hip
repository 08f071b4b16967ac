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
#include "rgbx_common.h"
#include "rgbx_rng.h"

namespace rgbx {
namespace {

// Lane layout and host helpers: the same as gat.hip's and supergat.hip's (a head occupies LPH = pow2ceil(C / VEC)
// consecutive lanes of VEC channels, HPC heads side by side in a group of G lanes that reads one neighbour row per
// step, NG = 64 / G rows per wave-instruction). Copied rather than shared: the text of gat.hip and supergat.hip keys
// the recorded counter measurements of their kernels (bench.py KERNEL_SOURCES), which an edit would invalidate.
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

int gat_grid(int64_t N) {  // one row per wave, no cap (see spmm.hip: uncapped grids balance ragged rows better)
  return (int)cdiv(N, 4);
}

// The target-side backward leaves one g_att record per workgroup, so its grid is capped and the waves stride over the
// rows.
int att_grid(int64_t N) {
  const int64_t b = cdiv(N, 4);
  return (int)(b < 1 ? 1 : (b < kMaxGrid ? b : kMaxGrid));
}

int flat_grid(int64_t n, int per_block) {
  const int64_t b = cdiv(n, per_block);
  return (int)(b < 1 ? 1 : (b < kMaxGrid ? b : kMaxGrid));
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

struct V2Split {
  int threshold;
  const int* chunk_row;
  const int* chunk_begin;
  const int* chunk_end;
  float* pacc;  // [n_chunks, F]
  float* p0;    // [n_chunks, H]  (forward only: running max)
  float* p1;    // [n_chunks, H]  (forward only: denominator)
};

// Training-mode state of one forward: `seed` = two 32-bit words on the device (NULL: no dropout).
struct V2Rng {
  const uint32_t* seed;
  float p_drop;
  float inv_keep;  // 1 / (1 - p_drop)
};

constexpr uint32_t kStreamDrop = 0xA4093822u;

// mix32 / draw32 / unit24: rgbx_rng.h (shared with supergat.hip and faconv.hip)
__device__ __forceinline__ bool drop_keep(uint32_t s0, uint32_t s1, int slot, int head, float p) {
  return unit24(draw32(s0, s1, kStreamDrop, (uint32_t)slot, (uint32_t)head)) >= p;
}

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

__device__ __forceinline__ float softmax_shift(float m, float rden) { return rden > 0.f ? m - logf(rden) : 0.f; }

// ------------------------------------------------------------------------------------------
// Forward: online softmax (running max, denominator, rescaled accumulator) over the slots of a row, read once.
// TRAIN: attention dropout in the accumulation (the normaliser stays that of the undropped softmax).
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
gatv2_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ xl, int64_t ldl,
                 const float* __restrict__ xr, int64_t ldr, const float* __restrict__ att,
                 const float* __restrict__ bias, float* __restrict__ out, int64_t ldo, float* __restrict__ m_out,
                 float* __restrict__ rden_out, int N, float slope, const GatLayout L, const V2Split sp,
                 const V2Rng rng) {
  constexpr int U = 4;  // neighbour rows in flight per lane group
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
              pk = drop_keep(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? p * rng.inv_keep : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc[i], sc, pk * v[u][i]);
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

// One wave per hub row: merge the chunk states in chunk order, normalise, store.
template <int VEC>
__global__ void __launch_bounds__(256)
gatv2_fwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                         const float* __restrict__ bias, float* __restrict__ out, int64_t ldo,
                         float* __restrict__ m_out, float* __restrict__ rden_out, const GatLayout L,
                         const V2Split sp) {
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
      float bv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) bv[i] = 0.f;
      if (bias) load_vec<VEC>(bv, bias + cofs);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = acc[i] * rd + bv[i];
      store_vec<VEC>(out + (int64_t)row * ldo + cofs, acc);
      if (m_out && ch == 0) {
        m_out[(int64_t)row * L.H + head] = l > 0.f ? m : 0.f;
        rden_out[(int64_t)row * L.H + head] = rd;
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
                     int N, float slope, const GatLayout L, const V2Split sp, const V2Rng rng) {
  constexpr int U = 3;
  __shared__ float red[4][kWave * 4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
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
              kappa = drop_keep(s0, s1, base + k + u * NG + g, head, rng.p_drop) ? rng.inv_keep : 0.f;
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
      for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_xr + (int64_t)row * ldgr + cofs, acc);
      }
    }

    // this workgroup's g_att record for the chunk: lane groups, then waves, in a fixed order
    for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) ga[i] += __shfl_xor(ga[i], off);
    }
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
                     const V2Split sp, const V2Rng rng) {
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
              kappa = drop_keep(s0, s1, __shfl(myslot, idx & 63), head, rng.p_drop) ? rng.inv_keep : 0.f;
            const float alpha = ok[u] ? expf(e - sh[u]) : 0.f;
            const float de = alpha * (kappa * dal - dsm[u]);
            const float ak = alpha * kappa;
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              acc[i] = fmaf(ak, go[u][i], fmaf(de * av[i], s[i] > 0.f ? 1.f : slope, acc[i]));
          }
        }
      }
      for (int off = 32; off >= L.G; off >>= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
      }
      if (g == 0 && active) {
        if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + cofs, acc);
        else store_vec<VEC>(g_xl + (int64_t)row * ldgl + cofs, acc);
      }
    }
  }
}

// One wave per hub row of either backward pass: chunk sums added in chunk order.
template <int VEC>
__global__ void __launch_bounds__(256)
gatv2_bwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                         float* __restrict__ gx, int64_t ldgx, const GatLayout L, const V2Split sp) {
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
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (int c = c0; c < c1; ++c) {
        float a2[VEC];
        load_vec<VEC>(a2, sp.pacc + (int64_t)c * F + cofs);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += a2[i];
      }
      store_vec<VEC>(gx + (int64_t)row * ldgx + cofs, acc);
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
    for (int h = 0; h < H; ++h) keep[p * H + h] = drop_keep(s0, s1, (int)p, h, p_drop) ? 1 : 0;
}

int split_view(const rgbx_row_split_t* split, int H, int C, bool fwd, V2Split* sd, const char* name) {
  *sd = V2Split{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!split || split->threshold <= 0 || split->n_chunks <= 0) return RGBX_OK;
  if (split->n_long <= 0 || !split->chunk_row || !split->chunk_begin || !split->chunk_end || !split->long_row ||
      !split->long_chunk_ptr || !split->partial)
    return fail(RGBX_E_ARG, "%s: incomplete row-split plan", name);
  const int64_t F = (int64_t)H * C;
  sd->threshold = split->threshold;
  sd->chunk_row = split->chunk_row;
  sd->chunk_begin = split->chunk_begin;
  sd->chunk_end = split->chunk_end;
  sd->pacc = split->partial;  // [n_chunks, F]
  if (fwd) {
    sd->p0 = sd->pacc + (int64_t)split->n_chunks * F;  // [n_chunks, H]
    sd->p1 = sd->p0 + (int64_t)split->n_chunks * H;    // [n_chunks, H]
  }
  return RGBX_OK;
}

int make_rng(const uint32_t* seed, float p_drop, V2Rng* rng, const char* name) {
  *rng = V2Rng{seed, p_drop, 1.0f};
  if (!seed) return RGBX_OK;
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(RGBX_E_ARG, "%s: dropout must be in [0, 1)", name);
  rng->inv_keep = 1.0f / (1.0f - p_drop);
  return RGBX_OK;
}

int64_t att_records(int64_t N, const rgbx_row_split_t* split) {
  return att_grid(N) + (split && split->threshold > 0 && split->n_chunks > 0 ? att_grid(split->n_chunks) : 0);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gatv2_supported(int H, int C) {
  if (H <= 0 || C <= 0) return 0;
  return C <= 64 || (C % 2 == 0 && C <= 128) || (C % 4 == 0 && C <= 256);
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
  if (!rgbx_gatv2_supported(H, C))
    return fail(RGBX_E_SHAPE, "gatv2_fwd: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)", C);
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !xl || !xr || !att || !out) return fail(RGBX_E_ARG, "gatv2_fwd: null pointer");
  if ((m == nullptr) != (rden == nullptr)) return fail(RGBX_E_ARG, "gatv2_fwd: m and rden go together");
  if (seed && !m) return fail(RGBX_E_ARG, "gatv2_fwd: training mode saves m and rden");
  const int64_t F = (int64_t)H * C;
  if (ldl < F || ldr < F || ldo < F) return fail(RGBX_E_ARG, "gatv2_fwd: leading dimension < H*C");
  if (!aligned_to({xl, xr, att, bias, out, m, rden}, 4))
    return fail(RGBX_E_ALIGN, "gatv2_fwd: float pointers must be 4-byte aligned");
  V2Split sd;
  if (int rc = split_view(split, H, C, true, &sd, "gatv2_fwd")) return rc;
  V2Rng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "gatv2_fwd")) return rc;
  const int vec = pick_vec(C, {xl, xr, att, bias, out, sd.pacc}, {ldl, ldr, ldo});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "gatv2_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = gat_grid(N);
#define RGBX_GATV2_FWD(V, T)                                                                                         \
  do {                                                                                                               \
    gatv2_fwd_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr, col, xl, ldl, xr, ldr, att, bias, out, ldo, m, rden,  \
                                                       (int)N, slope, L, sd, rng);                                   \
    if (sd.threshold > 0) {                                                                                          \
      gatv2_fwd_kernel<V, true, T><<<gat_grid(split->n_chunks), 256, 0, s>>>(                                        \
          rowptr, col, xl, ldl, xr, ldr, att, bias, out, ldo, m, rden, split->n_chunks, slope, L, sd, rng);          \
      gatv2_fwd_combine_kernel<V><<<gat_grid(split->n_long), 256, 0, s>>>(                                           \
          split->n_long, split->long_row, split->long_chunk_ptr, bias, out, ldo, m, rden, L, sd);                    \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_GATV2_FWD(4, true);
    else if (vec == 2) RGBX_GATV2_FWD(2, true);
    else RGBX_GATV2_FWD(1, true);
  } else {
    if (vec == 4) RGBX_GATV2_FWD(4, false);
    else if (vec == 2) RGBX_GATV2_FWD(2, false);
    else RGBX_GATV2_FWD(1, false);
  }
#undef RGBX_GATV2_FWD
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
  if (!rgbx_gatv2_supported(H, C))
    return fail(RGBX_E_SHAPE, "gatv2_bwd_dst: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)",
                C);
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
  V2Split sd;
  if (int rc = split_view(split, H, C, false, &sd, "gatv2_bwd_dst")) return rc;
  V2Rng rng;
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
#define RGBX_GATV2_BD(V, T)                                                                                          \
  do {                                                                                                               \
    gatv2_bwd_dst_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr, col, xl, ldl, xr, ldr, att, m, rden, out, ldo,    \
                                                           bias, gout, ldg, nq, g_xr, ldgr, att_partial, (int)N,     \
                                                           slope, L, sd, rng);                                       \
    if (sd.threshold > 0) {                                                                                          \
      gatv2_bwd_dst_kernel<V, true, T><<<att_grid(split->n_chunks), 256, 0, s>>>(                                    \
          rowptr, col, xl, ldl, xr, ldr, att, m, rden, out, ldo, bias, gout, ldg, nq, g_xr, ldgr,                    \
          att_partial + (int64_t)grid * F, split->n_chunks, slope, L, sd, rng);                                      \
      gatv2_bwd_combine_kernel<V><<<gat_grid(split->n_long), 256, 0, s>>>(                                           \
          split->n_long, split->long_row, split->long_chunk_ptr, g_xr, ldgr, L, sd);                                 \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_GATV2_BD(4, true);
    else if (vec == 2) RGBX_GATV2_BD(2, true);
    else RGBX_GATV2_BD(1, true);
  } else {
    if (vec == 4) RGBX_GATV2_BD(4, false);
    else if (vec == 2) RGBX_GATV2_BD(2, false);
    else RGBX_GATV2_BD(1, false);
  }
#undef RGBX_GATV2_BD
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
  if (!rgbx_gatv2_supported(H, C))
    return fail(RGBX_E_SHAPE, "gatv2_bwd_src: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)",
                C);
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !xl || !xr || !att || !nodeq || !gout || !g_xl)
    return fail(RGBX_E_ARG, "gatv2_bwd_src: null pointer");
  if (seed && !t2f) return fail(RGBX_E_ARG, "gatv2_bwd_src: training mode needs the slot map");
  const int64_t F = (int64_t)H * C;
  if (ldl < F || ldr < F || ldg < F || ldgl < F) return fail(RGBX_E_ARG, "gatv2_bwd_src: leading dimension < H*C");
  if (!aligned_to({nodeq}, 8)) return fail(RGBX_E_ALIGN, "gatv2_bwd_src: nodeq must be 8-byte aligned");
  if (!aligned_to({xl, xr, att, gout, g_xl}, 4))
    return fail(RGBX_E_ALIGN, "gatv2_bwd_src: float pointers must be 4-byte aligned");
  V2Split sd;
  if (int rc = split_view(split, H, C, false, &sd, "gatv2_bwd_src")) return rc;
  V2Rng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "gatv2_bwd_src")) return rc;
  const int vec = pick_vec(C, {xl, xr, att, gout, g_xl, sd.pacc}, {ldl, ldr, ldg, ldgl});
  GatLayout L;
  if (int rc = make_layout(H, C, vec, &L, "gatv2_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = gat_grid(N);
  const float2* nq = reinterpret_cast<const float2*>(nodeq);
#define RGBX_GATV2_BS(V, T)                                                                                          \
  do {                                                                                                               \
    gatv2_bwd_src_kernel<V, false, T><<<grid, 256, 0, s>>>(rowptr_t, col_t, t2f, xl, ldl, xr, ldr, att, nq, gout,    \
                                                           ldg, g_xl, ldgl, (int)N, slope, L, sd, rng);              \
    if (sd.threshold > 0) {                                                                                          \
      gatv2_bwd_src_kernel<V, true, T><<<gat_grid(split->n_chunks), 256, 0, s>>>(                                    \
          rowptr_t, col_t, t2f, xl, ldl, xr, ldr, att, nq, gout, ldg, g_xl, ldgl, split->n_chunks, slope, L, sd,     \
          rng);                                                                                                      \
      gatv2_bwd_combine_kernel<V><<<gat_grid(split->n_long), 256, 0, s>>>(                                           \
          split->n_long, split->long_row, split->long_chunk_ptr, g_xl, ldgl, L, sd);                                 \
    }                                                                                                                \
  } while (0)
  if (seed) {
    if (vec == 4) RGBX_GATV2_BS(4, true);
    else if (vec == 2) RGBX_GATV2_BS(2, true);
    else RGBX_GATV2_BS(1, true);
  } else {
    if (vec == 4) RGBX_GATV2_BS(4, false);
    else if (vec == 2) RGBX_GATV2_BS(2, false);
    else RGBX_GATV2_BS(1, false);
  }
#undef RGBX_GATV2_BS
  RGBX_CHECK_LAUNCH("gatv2_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gatv2_draws_u8(const uint32_t* seed, int64_t nnz, int H, float p_drop, uint8_t* keep,
                                   rgbx_stream_t stream) {
  if (nnz < 0 || H <= 0) return fail(RGBX_E_ARG, "gatv2_draws: bad size");
  if (nnz == 0) return RGBX_OK;
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "gatv2_draws: E' exceeds int32");
  if (!seed || !keep) return fail(RGBX_E_ARG, "gatv2_draws: null pointer");
  gatv2_draws_kernel<<<flat_grid(nnz, 256), 256, 0, (hipStream_t)stream>>>(seed, nnz, H, p_drop, keep);
  RGBX_CHECK_LAUNCH("gatv2_draws_kernel");
  return RGBX_OK;
}
