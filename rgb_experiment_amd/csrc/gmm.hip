// GMMConv / MoNet (Monti et al., "Geometric deep learning on graphs and manifolds using mixture model CNNs"): the fused
// Gaussian mixture message with its backward, and the paper's degree pseudo-coordinates, for gfx950. Stands in for
// GMMConv.message (separate_gaussians=False) [PyG].
//
// Every edge j -> i carries D pseudo-coordinates e[p, :] (p = the edge's forward CSR slot; one row PER SLOT, in forward
// slot order). With the kernel products h = x @ g viewed as [N, K, M] and the trained mu, sigma [K, D]:
//   gauss[p, k] = exp(-0.5 * sum_d (e[p,d] - mu[k,d])^2 * inv[k,d]),   inv[k,d] = 1 / (1e-15 + sigma[k,d]^2)
//   out[i, :]   = y0[i, :] + rs[i] * sum_p sum_k gauss[p, k] * h[col[p], k, :]
// where rs[i] = 1 / max(indeg(i), 1) gives the mean and rs = NULL the sum. The coefficient is a continuous, trained
// function of the edge's coordinates: every kernel evaluates it in registers from mu and sigma in DEVICE memory, so a
// captured launch follows the parameters an optimizer moves, and no [nnz, K] coefficient table passes from forward to
// backward. The lane layout is attn_common.h's with H = K heads of M channels (a head on LPH lanes of VEC channels, HPC
// heads side by side in a group of G lanes, NG = 64 / G neighbour rows per wave-instruction); the output is ONE head
// wide, so the forward also sums over the heads of a group and over the head chunks. The e rows of a target are
// consecutive: the forward and the edge pass read them as a stream beside the gather of h; the source pass, which walks
// the transposed CSR, gathers them through t2f.
//
// No float atomics, no scratch, no LDS; every sum runs in a fixed order: the slots of a lane group in slot order, the
// lane groups and then the heads of a group by a butterfly, the head chunks in ascending order, the hub-row chunks in
// chunk order (y0 rides on a row's first chunk); the parameter gradients by slot ranges of a fixed length, the ranges
// in ascending order.
#include "edge_common.h"

namespace rgbx {
namespace {

constexpr int kMaxKernels = 64;  // a wave of one-lane heads
constexpr int kMaxDim = 8;       // pseudo-coordinates per edge: a head's mu and inv stay in 16 registers
constexpr float kGmmEps = 1e-15f;

// A head's centres and inverse variances: loaded once per (row item, head chunk), never per slot. The loops over d run
// to kMaxDim with a wave-uniform guard, so every index is a constant and the arrays stay in registers.
struct GmmHead {
  float mu[kMaxDim], inv[kMaxDim];
};

__device__ __forceinline__ void load_head(GmmHead& hd, const float* __restrict__ mu, const float* __restrict__ sigma,
                                          int head, int D, bool active) {
#pragma unroll
  for (int d = 0; d < kMaxDim; ++d) {
    hd.mu[d] = 0.f;
    hd.inv[d] = 0.f;
    if (active && d < D) {
      const float s = sigma[head * D + d];
      hd.mu[d] = mu[head * D + d];
      hd.inv[d] = 1.0f / (kGmmEps + s * s);
    }
  }
}

// The D coordinates of one slot (all lanes of a lane group read the same row: one line).
__device__ __forceinline__ void load_coords(float (&ev)[kMaxDim], const float* __restrict__ erow, int D, bool on) {
#pragma unroll
  for (int d = 0; d < kMaxDim; ++d) ev[d] = (on && d < D) ? erow[d] : 0.f;
}

// d >= D holds e = mu = inv = 0 and adds an exact zero.
__device__ __forceinline__ float gauss_of(const float (&ev)[kMaxDim], const GmmHead& hd) {
  float q = 0.f;
#pragma unroll
  for (int d = 0; d < kMaxDim; ++d) {
    const float t = ev[d] - hd.mu[d];
    q = fmaf(t * t, hd.inv[d], q);
  }
  return expf(-0.5f * q);
}

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR. Per head chunk a lane accumulates gauss * h over its slots (U slots in flight per
// lane group); the butterfly then adds the lane groups and the heads of a group, and the head chunks are added in
// ascending order. CHUNK: the wave owns a chunk of a hub row and leaves a partial row of M floats, already scaled; the
// chunk that starts the row carries y0, so the combine kernel only adds.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gmm_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ e, int64_t lde,
               const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ rs,
               const float* __restrict__ h, int64_t ldh, const float* __restrict__ y0, int64_t ldy,
               float* __restrict__ out, int64_t ldo, int N, int D, const GatLayout L, const AttnSplit sp) {
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
      GmmHead hd;
      load_head(hd, mu, sigma, head, D, active && start < end);
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float hv[U][VEC], coef[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            const bool on = active && idx < n;
            float ev[kMaxDim];
            load_coords(ev, e + (int64_t)(base + (on ? idx : 0)) * lde, D, on);
#pragma unroll
            for (int i = 0; i < VEC; ++i) hv[u][i] = 0.f;
            if (on) load_vec<VEC>(hv[u], h + (int64_t)src * ldh + cofs);
            coef[u] = on ? gauss_of(ev, hd) : 0.f;
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
      if (rs) {
        const float scale = rs[row];
#pragma unroll
        for (int i = 0; i < VEC; ++i) tot[i] *= scale;
      }
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
// Backward, source side, over the TRANSPOSED CSR (row = source j, col_t[q] = target i, t2f[q] = the edge's forward
// slot, w_t[q] = rs[i] or NULL): g_h[j,k,:] = sum_q w_t[q] * gauss[t2f[q], k] * gout[col_t[q], :]. Every head of a group
// gathers the same gout fragment; the e row of the edge is gathered too. A source without out-edges stores zeros.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gmm_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ t2f,
                   const float* __restrict__ w_t, const float* __restrict__ e, int64_t lde,
                   const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ gout,
                   int64_t ldg, float* __restrict__ g_h, int64_t ldgh, int N, int D, const GatLayout L,
                   const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      GmmHead hd;
      load_head(hd, mu, sigma, head, D, active && start < end);
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col_t[base + lane] : 0;
        const int myslot = lane < n ? t2f[base + lane] : 0;
        const float myw = (lane < n && w_t) ? w_t[base + lane] : 1.0f;
        for (int k = 0; k < n; k += NG * U) {
          float go[U][VEC], coef[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int tgt = __shfl(mycol, idx & 63);
            const int slot = __shfl(myslot, idx & 63);
            const float ws = __shfl(myw, idx & 63);
            const bool on = active && idx < n;
            float ev[kMaxDim];
            load_coords(ev, e + (int64_t)(on ? slot : 0) * lde, D, on);
#pragma unroll
            for (int i = 0; i < VEC; ++i) go[u][i] = 0.f;
            if (on) load_vec<VEC>(go[u], gout + (int64_t)tgt * ldg + ch);
            coef[u] = on ? ws * gauss_of(ev, hd) : 0.f;
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

// ------------------------------------------------------------------------------------------
// Backward, edge side, stage 1, over the forward CSR (row = target i): s[p,k] = rs[i] * gauss[p,k] *
// <h[col[p],k,:], gout[i,:]>, one store per (slot, head) into the workspace table s [nnz, K]. No sum over slots is formed
// here: the chunk items only balance the hub rows and there is nothing to combine.
template <int VEC, bool CHUNK>
__global__ void __launch_bounds__(256)
gmm_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ e,
                    int64_t lde, const float* __restrict__ mu, const float* __restrict__ sigma,
                    const float* __restrict__ rs, const float* __restrict__ h, int64_t ldh,
                    const float* __restrict__ gout, int64_t ldg, float* __restrict__ s_tab, int N, int D,
                    const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    if (start == end) continue;
    const float scale = rs ? rs[row] : 1.0f;
    for (int hbase = 0; hbase < L.H; hbase += L.HPC) {
      const int head = hbase + hl;
      const bool active = hl < L.HPC && head < L.H && ch < L.C;
      const int cofs = head * L.C + ch;
      GmmHead hd;
      load_head(hd, mu, sigma, head, D, active);
      float go[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) go[i] = 0.f;
      if (active) load_vec<VEC>(go, gout + (int64_t)row * ldg + ch);

      for (int base = start; base < end; base += kWave) {
        const int n = min(kWave, end - base);
        const int mycol = lane < n ? col[base + lane] : 0;
        for (int k = 0; k < n; k += NG * U) {
          float hv[U][VEC], coef[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const int src = __shfl(mycol, idx & 63);
            const bool on = active && idx < n;
            float ev[kMaxDim];
            load_coords(ev, e + (int64_t)(base + (on ? idx : 0)) * lde, D, on);
#pragma unroll
            for (int i = 0; i < VEC; ++i) hv[u][i] = 0.f;
            if (on) load_vec<VEC>(hv[u], h + (int64_t)src * ldh + cofs);
            coef[u] = on ? scale * gauss_of(ev, hd) : 0.f;
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int idx = k + u * NG + g;
            const float dot = head_sum(dot_vec<VEC>(hv[u], go), L.LPH);
            if (active && idx < n && ch == 0) s_tab[(int64_t)(base + idx) * L.H + head] = coef[u] * dot;
          }
        }
      }
    }
  }
}

// Stage 2a: g_e[p,d] = -sum_k s[p,k] * (e[p,d] - mu[k,d]) * inv[k,d], one thread per slot, the heads in ascending order.
__global__ void __launch_bounds__(256)
gmm_edge_attr_kernel(const float* __restrict__ s_tab, const float* __restrict__ e, int64_t lde,
                     const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ g_e,
                     int64_t ldge, int64_t nnz, int K, int D) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    float ev[kMaxDim], ge[kMaxDim];
    load_coords(ev, e + p * lde, D, true);
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) ge[d] = 0.f;
    for (int k = 0; k < K; ++k) {
      const float s = s_tab[p * K + k];
#pragma unroll
      for (int d = 0; d < kMaxDim; ++d) {
        if (d < D) {
          const float sg = sigma[k * D + d];
          const float inv = 1.0f / (kGmmEps + sg * sg);
          ge[d] = fmaf(-s, (ev[d] - mu[k * D + d]) * inv, ge[d]);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d)
      if (d < D) g_e[p * ldge + d] = ge[d];
  }
}

// Stage 2b: the parameter gradients. A wave owns `per` consecutive slots (a multiple of 64) and, head by head, keeps 2 D
// running sums per lane over its slots in slot order, adds the lanes by a butterfly and leaves a record of 2 K D floats:
//   part[item, k, 0, d] = sum_p s[p,k] * (e[p,d] - mu[k,d]) * inv[k,d]
//   part[item, k, 1, d] = sum_p s[p,k] * (e[p,d] - mu[k,d])^2 * sigma[k,d] * inv[k,d]^2
__global__ void __launch_bounds__(256)
gmm_edge_param_kernel(const float* __restrict__ s_tab, const float* __restrict__ e, int64_t lde,
                      const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ part,
                      int64_t nnz, int64_t per, int n_items, int K, int D) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    const int64_t p0 = (int64_t)item * per;
    const int64_t p1 = p0 + per < nnz ? p0 + per : nnz;
    for (int k = 0; k < K; ++k) {
      float m[kMaxDim], iv[kMaxDim], sg[kMaxDim], am[kMaxDim], as[kMaxDim];
#pragma unroll
      for (int d = 0; d < kMaxDim; ++d) {
        m[d] = iv[d] = sg[d] = am[d] = as[d] = 0.f;
        if (d < D) {
          sg[d] = sigma[k * D + d];
          m[d] = mu[k * D + d];
          iv[d] = 1.0f / (kGmmEps + sg[d] * sg[d]);
        }
      }
      for (int64_t p = p0 + lane; p < p1; p += kWave) {
        const float s = s_tab[p * K + k];
        float ev[kMaxDim];
        load_coords(ev, e + p * lde, D, true);
#pragma unroll
        for (int d = 0; d < kMaxDim; ++d) {
          const float t = (ev[d] - m[d]) * iv[d];  // d >= D: e = mu = inv = 0
          const float st = s * t;
          am[d] += st;
          as[d] = fmaf(st * t, sg[d], as[d]);
        }
      }
#pragma unroll
      for (int d = 0; d < kMaxDim; ++d) {
        if (d < D) {
          for (int off = 32; off > 0; off >>= 1) {
            am[d] += __shfl_xor(am[d], off);
            as[d] += __shfl_xor(as[d], off);
          }
          if (lane == 0) {
            float* rec = part + ((int64_t)item * K + k) * 2 * D;
            rec[d] = am[d];
            rec[D + d] = as[d];
          }
        }
      }
    }
  }
}

// Stage 3: a wave per output element; lane l adds the records l, l + 64, ... in ascending order, then the butterfly.
__global__ void __launch_bounds__(256)
gmm_param_combine_kernel(const float* __restrict__ part, float* __restrict__ g_mu, float* __restrict__ g_sigma,
                         int n_items, int K, int D) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int n_out = 2 * K * D;
  for (int o = blockIdx.x * wpb + (threadIdx.x >> 6); o < n_out; o += gridDim.x * wpb) {
    float acc = 0.f;
    for (int it = lane; it < n_items; it += kWave) acc += part[(int64_t)it * n_out + o];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
      const int k = o / (2 * D), r = o % (2 * D);
      if (r < D) g_mu[k * D + r] = acc;
      else g_sigma[k * D + (r - D)] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The MoNet paper's pseudo-coordinates of a graph without edge attributes, per forward CSR slot p of row i:
//   u[p] = (1 / sqrt(1 + indeg(col[p])), 1 / sqrt(1 + indeg(i))),  indeg(v) = rowptr[v + 1] - rowptr[v].
// The + 1 keeps a source without in-edges finite. Integers until the one square root and the one division.
template <bool CHUNK>
__global__ void __launch_bounds__(256)
gmm_degree_pseudo_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, float* __restrict__ u, int N,
                         const AttnSplit sp) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    int deg = end - start;
    if constexpr (CHUNK) deg = rowptr[row + 1] - rowptr[row];
    const float mine = 1.0f / sqrtf((float)(1 + deg));
    for (int p = start + lane; p < end; p += kWave) {
      const int j = col[p];
      const int dj = rowptr[j + 1] - rowptr[j];
      u[2 * (int64_t)p] = 1.0f / sqrtf((float)(1 + dj));
      u[2 * (int64_t)p + 1] = mine;
    }
  }
}

bool gmm_supported(int64_t K, int64_t M, int64_t D) {
  return K > 0 && K <= kMaxKernels && head_width_supported(M) && D > 0 && D <= kMaxDim;
}

int check_sizes(int64_t N, int K, int M, int D, const char* name) {
  if (int rc = check_common(N, K, M, name)) return rc;
  if (!gmm_supported(K, M, D))
    return fail(RGBX_E_SHAPE,
                "%s: %d kernels of %d channels over %d coordinates (1 <= K <= %d; any M <= 64, even M <= 128, M %% 4 == 0 "
                "up to 256; 1 <= D <= %d)", name, K, M, D, kMaxKernels, kMaxDim);
  return RGBX_OK;
}

// The slot ranges of the parameter reduction: at most 8192 records, each over a multiple of 64 slots (at least 1024).
constexpr int64_t kMaxParamItems = 8192;

int64_t param_range(int64_t nnz) {
  const int64_t items = std::min<int64_t>(std::max<int64_t>(cdiv(nnz, 1024), 1), kMaxParamItems);
  return cdiv(cdiv(nnz, items), kWave) * kWave;
}

int64_t param_items(int64_t nnz) { return nnz > 0 ? cdiv(nnz, param_range(nnz)) : 0; }

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gmm_supported(int K, int M, int D) { return gmm_supported(K, M, D); }

extern "C" int rgbx_gmm_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* e, int64_t lde, const float* mu,
                                const float* sigma, const float* rs, const float* h, int64_t ldh, const float* y0,
                                int64_t ldy, float* out, int64_t ldo, int64_t N, int K, int M, int D,
                                const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, K, M, D, "gmm_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !e || !mu || !sigma || !h || !out) return fail(RGBX_E_ARG, "gmm_fwd: null pointer");
  if (ldh < (int64_t)K * M) return fail(RGBX_E_ARG, "gmm_fwd: leading dimension of h < K*M");
  if (lde < D) return fail(RGBX_E_ARG, "gmm_fwd: leading dimension of e < D");
  if (ldo < M || (y0 && ldy < M)) return fail(RGBX_E_ARG, "gmm_fwd: leading dimension < M");
  if (out == h || out == y0 || out == e) return fail(RGBX_E_ARG, "gmm_fwd: out must not alias h, y0 or e");
  if (!aligned_to({e, mu, sigma, rs, h, y0, out}, 4))
    return fail(RGBX_E_ALIGN, "gmm_fwd: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, M, 0, &sd, "gmm_fwd")) return rc;
  const int vec = pick_vec(M, {h, y0, out, sd.pacc}, {ldh, y0 ? ldy : 0, ldo});
  GatLayout L, L1;
  if (int rc = make_layout(K, M, vec, &L, "gmm_fwd")) return rc;
  if (int rc = make_layout(1, M, vec, &L1, "gmm_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(gmm_fwd_kernel, N, rowptr, col, e, lde, mu, sigma, rs, h, ldh, y0, ldy, out, ldo, n_items, D, L, sd);
  if (sd.threshold > 0)  // a plain sum of one-head rows: the chunk partials added in chunk order
    RGBX_VEC_SWITCH(vec, attn_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(
                             split->n_long, split->long_row, split->long_chunk_ptr, out, ldo, M, 0, L1, sd));
  RGBX_CHECK_LAUNCH("gmm_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gmm_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* w_t,
                                    const float* e, int64_t lde, const float* mu, const float* sigma, const float* gout,
                                    int64_t ldg, float* g_h, int64_t ldgh, int64_t N, int K, int M, int D,
                                    const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, K, M, D, "gmm_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !t2f || !e || !mu || !sigma || !gout || !g_h)
    return fail(RGBX_E_ARG, "gmm_bwd_src: null pointer");
  const int64_t F = (int64_t)K * M;
  if (ldg < M) return fail(RGBX_E_ARG, "gmm_bwd_src: leading dimension of gout < M");
  if (ldgh < F) return fail(RGBX_E_ARG, "gmm_bwd_src: leading dimension of g_h < K*M");
  if (lde < D) return fail(RGBX_E_ARG, "gmm_bwd_src: leading dimension of e < D");
  if (g_h == gout || g_h == e) return fail(RGBX_E_ARG, "gmm_bwd_src: g_h must not alias gout or e");
  if (!aligned_to({t2f, w_t, e, mu, sigma, gout, g_h}, 4))
    return fail(RGBX_E_ALIGN, "gmm_bwd_src: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, K, M, 0, &sd, "gmm_bwd_src")) return rc;
  const int vec = pick_vec(M, {gout, g_h, sd.pacc}, {ldg, ldgh});
  GatLayout L;
  if (int rc = make_layout(K, M, vec, &L, "gmm_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_EDGE_ROWS(gmm_bwd_src_kernel, N, rowptr_t, col_t, t2f, w_t, e, lde, mu, sigma, gout, ldg, g_h, ldgh, n_items, D, L,
                 sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(g_h, ldgh, F, 0);
  RGBX_CHECK_LAUNCH("gmm_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gmm_bwd_edge_workspace_bytes(int64_t nnz, int K, int D, size_t* bytes) {
  if (!bytes || nnz < 0 || K <= 0 || D <= 0) return fail(RGBX_E_ARG, "gmm_bwd_edge_workspace_bytes: bad argument");
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "gmm_bwd_edge_workspace_bytes: nnz exceeds int32");
  // the table s [nnz, K], then one record of 2 K D floats per slot range
  *bytes = ((size_t)nnz * (size_t)K + (size_t)param_items(nnz) * 2 * (size_t)K * (size_t)D) * sizeof(float);
  return RGBX_OK;
}

extern "C" int rgbx_gmm_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* e, int64_t lde,
                                     const float* mu, const float* sigma, const float* rs, const float* h, int64_t ldh,
                                     const float* gout, int64_t ldg, float* g_e, int64_t ldge, float* g_mu,
                                     float* g_sigma, void* workspace, size_t workspace_bytes, int64_t N, int64_t nnz,
                                     int K, int M, int D, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, K, M, D, "gmm_bwd_edge")) return rc;
  if (nnz < 0) return fail(RGBX_E_ARG, "gmm_bwd_edge: bad size");
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "gmm_bwd_edge: nnz exceeds int32");
  if ((g_mu == nullptr) != (g_sigma == nullptr))
    return fail(RGBX_E_ARG, "gmm_bwd_edge: g_mu and g_sigma go together (both or neither)");
  if (!g_e && !g_mu) return RGBX_OK;  // nothing asked for
  if (!mu || !sigma) return fail(RGBX_E_ARG, "gmm_bwd_edge: null pointer");
  if (!aligned_to({e, mu, sigma, rs, h, gout, g_e, g_mu, g_sigma, workspace}, 4))
    return fail(RGBX_E_ALIGN, "gmm_bwd_edge: pointers must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0 || nnz == 0) {  // no slot: no g_e row, and the parameter gradients are zeros, written
    if (g_mu) {
      if (hipError_t err = hipMemsetAsync(g_mu, 0, sizeof(float) * K * D, s); err != hipSuccess)
        return hip_fail(err, "gmm_bwd_edge: memset");
      if (hipError_t err = hipMemsetAsync(g_sigma, 0, sizeof(float) * K * D, s); err != hipSuccess)
        return hip_fail(err, "gmm_bwd_edge: memset");
    }
    return RGBX_OK;
  }
  if (!rowptr || !col || !e || !h || !gout) return fail(RGBX_E_ARG, "gmm_bwd_edge: null pointer");
  if (ldh < (int64_t)K * M) return fail(RGBX_E_ARG, "gmm_bwd_edge: leading dimension of h < K*M");
  if (ldg < M) return fail(RGBX_E_ARG, "gmm_bwd_edge: leading dimension of gout < M");
  if (lde < D || (g_e && ldge < D)) return fail(RGBX_E_ARG, "gmm_bwd_edge: leading dimension of e or g_e < D");
  if (g_e && (g_e == e || (const void*)g_e == workspace))
    return fail(RGBX_E_ARG, "gmm_bwd_edge: g_e must not alias e or the workspace");
  size_t need = 0;
  if (int rc = rgbx_gmm_bwd_edge_workspace_bytes(nnz, K, D, &need)) return rc;
  if (!workspace || workspace_bytes < need)
    return fail(RGBX_E_WS, "gmm_bwd_edge: workspace %zu < %zu bytes", workspace_bytes, need);
  AttnSplit sd;
  if (int rc = split_view(split, 1, 1, 0, &sd, "gmm_bwd_edge")) return rc;  // the plan only: no chunk record
  const int vec = pick_vec(M, {h, gout}, {ldh, ldg});
  GatLayout L;
  if (int rc = make_layout(K, M, vec, &L, "gmm_bwd_edge")) return rc;
  float* s_tab = static_cast<float*>(workspace);
  float* part = s_tab + (size_t)nnz * K;
  RGBX_EDGE_ROWS(gmm_bwd_edge_kernel, N, rowptr, col, e, lde, mu, sigma, rs, h, ldh, gout, ldg, s_tab, n_items, D, L, sd);
  if (g_e)
    gmm_edge_attr_kernel<<<capped_grid(nnz, 256), 256, 0, s>>>(s_tab, e, lde, mu, sigma, g_e, ldge, nnz, K, D);
  if (g_mu) {
    const int64_t per = param_range(nnz);
    const int n_items = (int)param_items(nnz);
    gmm_edge_param_kernel<<<capped_grid(n_items, 4), 256, 0, s>>>(s_tab, e, lde, mu, sigma, part, nnz, per, n_items, K, D);
    gmm_param_combine_kernel<<<capped_grid(2 * K * D, 4), 256, 0, s>>>(part, g_mu, g_sigma, n_items, K, D);
  }
  RGBX_CHECK_LAUNCH("gmm_bwd_edge_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gmm_degree_pseudo_f32(const int32_t* rowptr, const int32_t* col, float* u, int64_t N,
                                          const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0) return fail(RGBX_E_ARG, "gmm_degree_pseudo: bad size");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "gmm_degree_pseudo: size exceeds int32");
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !u) return fail(RGBX_E_ARG, "gmm_degree_pseudo: null pointer");
  if (!aligned_to({rowptr, col, u}, 4)) return fail(RGBX_E_ALIGN, "gmm_degree_pseudo: pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, 1, 0, &sd, "gmm_degree_pseudo")) return rc;  // the plan only: no chunk record
  hipStream_t s = (hipStream_t)stream;
  gmm_degree_pseudo_kernel<false><<<row_grid(N), 256, 0, s>>>(rowptr, col, u, (int)N, sd);
  if (sd.threshold > 0)
    gmm_degree_pseudo_kernel<true><<<row_grid(split->n_chunks), 256, 0, s>>>(rowptr, col, u, split->n_chunks, sd);
  RGBX_CHECK_LAUNCH("gmm_degree_pseudo_kernel");
  return RGBX_OK;
}
