// FAGCN's layer (FAConv [PyG] behind reference models/fagcn.py): a GCN-weighted gather whose per-edge coefficient is
// signed, tanh(<x_j, att_l> + <x_i, att_r>), with dropout on the coefficient and an eps * x_0 residual, and its
// backward, for gfx950. For an edge j -> i of the target-grouped CSR (self-loop slot included):
//   a = tanh(al_j + ar_i),  c = k a w,  out_i = sum_j c x_j + eps x0_i,   k = keep / (1 - p) (1 outside training)
// al / ar live interleaved in alr [N, 2] (one skinny product, fa_scores_kernel). The coefficient is never written:
// the 64 (col, w, al_j) triples of a row chunk are read once, coalesced, tanh is taken once per slot, and the
// result is handed to the lane groups with ds_bpermute beside the column index, as spmm.hip hands its weights.
//
// Backward, with g = dL/dout, q = k w (1 - a^2) and s = q <g_i, x_j>:
//   target side (forward CSR):     g_ar[i] = sum_j s
//   source side (transposed CSR):  g_al[j] = sum_i s,  g_x[j] = sum_i c g_i + g_al[j] att_l + g_ar[j] att_r
// Neither pass reduces <g_i, x_j> across lanes per slot: a row's sum of s is the sum over the lanes of
// sum_slots q * (this lane's share of the dot product), so every lane keeps one running scalar and the wave adds the
// 64 of them once per row, in a fixed order. s is recomputed on the source side (x_j is the row in registers, g_i is
// gathered there anyway); nothing per edge is stored (FAConv, has the byte count of the alternative).
//
// Dropout is counter-based (rgbx_rng.h): the keep of a slot is a hash of (seed, FORWARD slot id); the source-side
// pass finds that id in t2f. Lane layout, row-split plan and reproducibility are those of spmm.hip / supergat.hip.
#include "attn_common.h"

namespace rgbx {
namespace {

constexpr uint32_t kStreamFaDrop = 0xA4093822u;

// AttnSplit here: pacc [n_chunks, C], p0 [n_chunks] (backward only). AttnRng, row_item, dot_vec: attn_common.h
__device__ __forceinline__ float fa_keep(uint32_t s0, uint32_t s1, int slot, const AttnRng& rng) {
  return unit24(draw32(s0, s1, kStreamFaDrop, (uint32_t)slot, 0u)) >= rng.p_drop ? rng.inv_keep : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// alr[r] = (<x_r, att_l>, <x_r, att_r>): a group of G = 2^lg lanes per row, any C.
template <int VEC>
__global__ void __launch_bounds__(256)
fa_scores_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ att_l,
                 const float* __restrict__ att_r, float2* __restrict__ alr, int N, int C, int lg) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << lg, NG = kWave >> lg;
  const int g = lane >> lg, t = lane & (G - 1);
  const int wpb = blockDim.x >> 6;
  for (int r0 = (blockIdx.x * wpb + (threadIdx.x >> 6)) * NG; r0 < N; r0 += gridDim.x * wpb * NG) {
    const int row = r0 + g;
    float sl = 0.f, sr = 0.f;
    if (row < N) {
      for (int c = t * VEC; c < C; c += G * VEC) {
        float v[VEC], a[VEC], b[VEC];
        load_vec<VEC>(v, x + (int64_t)row * ldx + c);
        load_vec<VEC>(a, att_l + c);
        load_vec<VEC>(b, att_r + c);
        sl += dot_vec<VEC>(v, a);
        sr += dot_vec<VEC>(v, b);
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) {
      sl += __shfl_xor(sl, off);
      sr += __shfl_xor(sr, off);
    }
    if (row < N && t == 0) alr[row] = make_float2(sl, sr);
  }
}

// ------------------------------------------------------------------------------------------
// Forward.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
fa_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
              const float* __restrict__ x, int64_t ldx, const float2* __restrict__ alr, const float* __restrict__ x0,
              int64_t ldx0, float eps, float* __restrict__ out, int64_t ldo, int n_items, int C, int lg,
              const AttnSplit sp, const AttnRng rng) {
  constexpr int U = 4;  // neighbour rows in flight per lane group
  const int lane = threadIdx.x & 63;
  const int G = 1 << lg, NG = kWave >> lg;
  const int g = lane >> lg;
  const int ch = (lane & (G - 1)) * VEC;
  const bool active = ch < C;
  const int wpb = blockDim.x >> 6;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    const float ar = alr[row].y;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int mycol = 0;
      float myc = 0.f;
      if (lane < n) {
        mycol = col[base + lane];
        float wk = w[base + lane];
        if constexpr (TRAIN) wk *= fa_keep(s0, s1, base + lane, rng);
        myc = tanhf(alr[mycol].x + ar) * wk;
      }
      for (int k = 0; k < n; k += NG * U) {
        float v[U][VEC];
        float cc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
          cc[u] = __shfl(myc, idx & 63);
          const bool ok = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
          if (ok) load_vec<VEC>(v[u], x + (int64_t)src * ldx + ch);
          else cc[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(cc[u], v[u][i], acc[i]);
        }
      }
    }
    for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
    }
    if (g == 0 && active) {
      if constexpr (CHUNK) {
        store_vec<VEC>(sp.pacc + (int64_t)item * C + ch, acc);
      } else {
        if (x0) {
          float r[VEC];
          load_vec<VEC>(r, x0 + (int64_t)row * ldx0 + ch);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(eps, r[i], acc[i]);
        }
        store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);
      }
    }
  }
}

// One wave per hub row: chunk sums added in chunk order, then the row's epilogue.
//   MODE 0 (forward):       out = sum + eps x0
//   MODE 1 (target side):   g_alr[row].y = sum p0
//   MODE 2 (source side):   g_alr[row].x = sum p0,  g_x = sum + g_al att_l + g_alr[row].y att_r
template <int VEC, int MODE>
__global__ void __launch_bounds__(256)
fa_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                  const float* __restrict__ x0, int64_t ldx0, float eps, const float* __restrict__ att_l,
                  const float* __restrict__ att_r, float* __restrict__ g_alr, float* __restrict__ out, int64_t ldo,
                  int C, const AttnSplit sp) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    float ss = 0.f, other = 0.f;
    if constexpr (MODE != 0) {
      for (int c = c0; c < c1; ++c) ss += sp.p0[c];
      if (lane == 0) g_alr[(int64_t)row * 2 + (MODE == 1 ? 1 : 0)] = ss;
      if constexpr (MODE == 2) other = g_alr[(int64_t)row * 2 + 1];
    }
    if constexpr (MODE == 1) continue;
    for (int ch = lane * VEC; ch < C; ch += kWave * VEC) {
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (int c = c0; c < c1; ++c) {
        float p[VEC];
        load_vec<VEC>(p, sp.pacc + (int64_t)c * C + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += p[i];
      }
      if constexpr (MODE == 0) {
        if (x0) {
          float rv[VEC];
          load_vec<VEC>(rv, x0 + (int64_t)row * ldx0 + ch);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(eps, rv[i], acc[i]);
        }
      } else {
        float al[VEC], arv[VEC];
        load_vec<VEC>(al, att_l + ch);
        load_vec<VEC>(arv, att_r + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(ss, al[i], fmaf(other, arv[i], acc[i]));
      }
      store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward, target side, over the forward CSR (row = target i): g_alr[i].y = sum_j q <g_i, x_j>.
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
fa_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
                  const float* __restrict__ x, int64_t ldx, const float2* __restrict__ alr,
                  const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_alr, int n_items, int C, int lg,
                  const AttnSplit sp, const AttnRng rng) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int G = 1 << lg, NG = kWave >> lg;
  const int g = lane >> lg;
  const int ch = (lane & (G - 1)) * VEC;
  const bool active = ch < C;
  const int wpb = blockDim.x >> 6;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    const float ar = alr[row].y;
    float go[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) go[i] = 0.f;
    if (active) load_vec<VEC>(go, gout + (int64_t)row * ldg + ch);
    float acc_s = 0.f;  // this lane's share of sum_j s
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int mycol = 0;
      float myq = 0.f;
      if (lane < n) {
        mycol = col[base + lane];
        float wk = w[base + lane];
        if constexpr (TRAIN) wk *= fa_keep(s0, s1, base + lane, rng);
        const float a = tanhf(alr[mycol].x + ar);
        myq = wk * (1.f - a * a);
      }
      for (int k = 0; k < n; k += NG * U) {
        float v[U][VEC];
        float qq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
          qq[u] = __shfl(myq, idx & 63);
          const bool ok = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
          if (ok) load_vec<VEC>(v[u], x + (int64_t)src * ldx + ch);
          else qq[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc_s = fmaf(qq[u], dot_vec<VEC>(v[u], go), acc_s);
      }
    }
    acc_s = wave_sum(acc_s);
    if (lane == 0) {
      if constexpr (CHUNK) sp.p0[item] = acc_s;
      else g_alr[(int64_t)row * 2 + 1] = acc_s;
    }
  }
}

// Backward, source side, over the TRANSPOSED CSR (row = source j, col_t[p] = target i, t2f[p] = the forward slot of
// the same edge, which keys its dropout decision); runs after the target side (reads g_alr[j].y):
//   g_alr[j].x = sum_i q <g_i, x_j>,   g_x[j] = sum_i c g_i + g_alr[j].x att_l + g_alr[j].y att_r
template <int VEC, bool CHUNK, bool TRAIN>
__global__ void __launch_bounds__(256)
fa_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const float* __restrict__ w_t,
                  const int* __restrict__ t2f, const float* __restrict__ x, int64_t ldx,
                  const float2* __restrict__ alr, const float* __restrict__ gout, int64_t ldg,
                  const float* __restrict__ att_l, const float* __restrict__ att_r, float* __restrict__ g_alr,
                  float* __restrict__ g_x, int64_t ldgx, int n_items, int C, int lg, const AttnSplit sp,
                  const AttnRng rng) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int G = 1 << lg, NG = kWave >> lg;
  const int g = lane >> lg;
  const int ch = (lane & (G - 1)) * VEC;
  const bool active = ch < C;
  const int wpb = blockDim.x >> 6;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    const float al = alr[row].x;
    float xj[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) xj[i] = acc[i] = 0.f;
    if (active) load_vec<VEC>(xj, x + (int64_t)row * ldx + ch);
    float acc_s = 0.f;
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int mycol = 0;
      float myc = 0.f, myq = 0.f;
      if (lane < n) {
        mycol = col_t[base + lane];
        float wk = w_t[base + lane];
        if constexpr (TRAIN) wk *= fa_keep(s0, s1, t2f[base + lane], rng);
        const float a = tanhf(al + alr[mycol].y);
        myc = wk * a;
        myq = wk * (1.f - a * a);
      }
      for (int k = 0; k < n; k += NG * U) {
        float v[U][VEC];
        float cc[U], qq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int tgt = __shfl(mycol, idx & 63);
          cc[u] = __shfl(myc, idx & 63);
          qq[u] = __shfl(myq, idx & 63);
          const bool ok = active && idx < n;
#pragma unroll
          for (int i = 0; i < VEC; ++i) v[u][i] = 0.f;
          if (ok) load_vec<VEC>(v[u], gout + (int64_t)tgt * ldg + ch);
          else cc[u] = qq[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          acc_s = fmaf(qq[u], dot_vec<VEC>(v[u], xj), acc_s);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(cc[u], v[u][i], acc[i]);
        }
      }
    }
    for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
    }
    acc_s = wave_sum(acc_s);
    if constexpr (CHUNK) {
      if (g == 0 && active) store_vec<VEC>(sp.pacc + (int64_t)item * C + ch, acc);
      if (lane == 0) sp.p0[item] = acc_s;
    } else {
      const float gar = g_alr[(int64_t)row * 2 + 1];
      if (g == 0 && active) {
        float a1[VEC], a2[VEC];
        load_vec<VEC>(a1, att_l + ch);
        load_vec<VEC>(a2, att_r + ch);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(acc_s, a1[i], fmaf(gar, a2[i], acc[i]));
        store_vec<VEC>(g_x + (int64_t)row * ldgx + ch, acc);
      }
      if (lane == 0) g_alr[(int64_t)row * 2] = acc_s;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Composed path (widths the fused kernels refuse): the per-slot coefficient c = k a w (and q = k w (1 - a^2)) written
// out for rgbx_spmm_csr_f32, one wave per CSR row. transposed: the row supplies al and the column ar; `slot` maps a
// slot to the forward slot that keys its dropout decision (NULL = identity).
template <bool TRAIN>
__global__ void __launch_bounds__(256)
fa_edge_coef_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
                    const int* __restrict__ slot, const float2* __restrict__ alr, int transposed, int N,
                    const AttnRng rng, float* __restrict__ coef, float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  uint32_t s0 = 0, s1 = 0;
  if constexpr (TRAIN) {
    s0 = rng.seed[0];
    s1 = rng.seed[1];
  }
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int start = rowptr[row], end = rowptr[row + 1];
    const float2 mine = alr[row];
    for (int p = start + lane; p < end; p += kWave) {
      const float2 other = alr[col[p]];
      const float a = tanhf(transposed ? mine.x + other.y : other.x + mine.y);
      float wk = w[p];
      if constexpr (TRAIN) wk *= fa_keep(s0, s1, slot ? slot[p] : p, rng);
      coef[p] = wk * a;
      if (q) q[p] = wk * (1.f - a * a);
    }
  }
}

// out[i * stride] = sum_p q[p] <a[i,:], b[col[p],:]> for any width: one wave per row, one slot at a time. The slots are
// summed in runs of kWave and the runs' sums added up: one accumulator over a hub row of k equal terms (k copies of one
// edge) rounds the same way on every step and drifts by up to k 2^-25 of the sum, 2.6e-4 at k = 3070. Rows of up to
// kWave slots keep their bits.
__global__ void __launch_bounds__(256)
fa_edge_dot_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ q,
                   const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                   float* __restrict__ out, int64_t stride, int N, int C) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int start = rowptr[row], end = rowptr[row + 1];
    float acc = 0.f;
    for (int base = start; base < end; base += kWave) {
      const int stop = min(base + kWave, end);
      float run = 0.f;
      for (int p = base; p < stop; ++p) {
        const float* br = b + (int64_t)col[p] * ldb;
        float d = 0.f;
        for (int c = lane; c < C; c += kWave) d = fmaf(a[(int64_t)row * lda + c], br[c], d);
        run = fmaf(q[p], d, run);
      }
      acc += run;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[(int64_t)row * stride] = acc;
  }
}

// The dropout decisions of a training forward, written out for inspection (tests): keep[p] in forward CSR slot order.
__global__ void __launch_bounds__(256)
fa_draws_kernel(const uint32_t* __restrict__ seed, int64_t nnz, const AttnRng rng, uint8_t* __restrict__ keep) {
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x)
    keep[p] = fa_keep(s0, s1, (int)p, rng) != 0.f ? 1 : 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------

int fa_vec(int64_t C) { return C % 4 == 0 ? 4 : (C % 2 == 0 ? 2 : 1); }

int fa_lg(int64_t C, int vec) {  // log2 of the lanes per row, capped at a whole wave
  int lg = 0;
  while ((1 << lg) * vec < C && lg < 6) ++lg;
  return lg;
}

int fa_check(int64_t N, int64_t C, bool fused, const char* name) {
  if (N < 0 || C <= 0) return fail(RGBX_E_ARG, "%s: bad size", name);
  if (N >= INT32_MAX || C >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: size exceeds int32", name);
  if (fused && !rgbx_faconv_supported(C))
    return fail(RGBX_E_SHAPE, "%s: C=%lld needs more than 64 lanes per row; take the composed path", name,
                (long long)C);
  return RGBX_OK;
}

// Rows are read in fragments of vec floats, vec from C alone: pointers and leading dimensions must allow it.
int fa_aligned(int64_t C, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds,
               const char* name) {
  const int vec = fa_vec(C);
  for (int64_t ld : lds) {
    if (ld < C) return fail(RGBX_E_ARG, "%s: leading dimension < C", name);
    if (ld % vec) return fail(RGBX_E_ALIGN, "%s: leading dimension %lld is not a multiple of %d", name, (long long)ld, vec);
  }
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % (vec * 4))
      return fail(RGBX_E_ALIGN, "%s: pointer not aligned to %d bytes", name, vec * 4);
  return RGBX_OK;
}

// pacc [n_chunks, C] and one scalar per chunk; the fragments are read vec floats at a time.
int fa_split_view(const rgbx_row_split_t* split, int64_t C, AttnSplit* sd, const char* name) {
  if (int rc = split_view(split, 1, (int)C, 1, sd, name)) return rc;
  if (sd->threshold > 0 && reinterpret_cast<uintptr_t>(split->partial) % 16)
    return fail(RGBX_E_ALIGN, "%s: split->partial must be 16-byte aligned", name);
  return RGBX_OK;
}

#define RGBX_FA_COMBINE(MODE, ...)                                                                        \
  RGBX_VEC_SWITCH(vec, fa_combine_kernel<V, MODE><<<row_grid(split->n_long), 256, 0, s>>>(                \
                           split->n_long, split->long_row, split->long_chunk_ptr, __VA_ARGS__, (int)C, sd))

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_faconv_supported(int64_t C) {
  return head_width_supported(C);
}

extern "C" int rgbx_faconv_scores_f32(const float* x, int64_t ldx, const float* att_l, const float* att_r, float* alr,
                                      int64_t N, int64_t C, rgbx_stream_t stream) {
  if (int rc = fa_check(N, C, false, "faconv_scores")) return rc;
  if (N == 0) return RGBX_OK;
  if (!x || !att_l || !att_r || !alr) return fail(RGBX_E_ARG, "faconv_scores: null pointer");
  if (int rc = fa_aligned(C, {x, att_l, att_r}, {ldx}, "faconv_scores")) return rc;
  if (reinterpret_cast<uintptr_t>(alr) % 8) return fail(RGBX_E_ALIGN, "faconv_scores: alr must be 8-byte aligned");
  const int vec = fa_vec(C), lg = fa_lg(C, vec);
  const int grid = capped_grid(N, 4 * (kWave >> lg));
  hipStream_t s = (hipStream_t)stream;
  float2* o = reinterpret_cast<float2*>(alr);
  RGBX_VEC_SWITCH(vec, fa_scores_kernel<V><<<grid, 256, 0, s>>>(x, ldx, att_l, att_r, o, (int)N, (int)C, lg));
  RGBX_CHECK_LAUNCH("fa_scores_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* x,
                                   int64_t ldx, const float* alr, const float* x0, int64_t ldx0, float eps, float* out,
                                   int64_t ldo, int64_t N, int64_t C, const uint32_t* seed, float p_drop,
                                   const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = fa_check(N, C, true, "faconv_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !w || !x || !alr || !out) return fail(RGBX_E_ARG, "faconv_fwd: null pointer");
  if (out == x) return fail(RGBX_E_ARG, "faconv_fwd: out must not alias x");
  if (int rc = fa_aligned(C, {x, out}, {ldx, ldo}, "faconv_fwd")) return rc;
  if (x0) {
    if (int rc = fa_aligned(C, {x0}, {ldx0}, "faconv_fwd")) return rc;
  }
  if (reinterpret_cast<uintptr_t>(alr) % 8) return fail(RGBX_E_ALIGN, "faconv_fwd: alr must be 8-byte aligned");
  AttnSplit sd;
  if (int rc = fa_split_view(split, C, &sd, "faconv_fwd")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "faconv_fwd")) return rc;
  const int vec = fa_vec(C), lg = fa_lg(C, vec);
  hipStream_t s = (hipStream_t)stream;
  const float2* a2 = reinterpret_cast<const float2*>(alr);
  RGBX_ATTN_DISPATCH(fa_fwd_kernel, row_grid, N, rowptr, col, w, x, ldx, a2, x0, ldx0, eps, out, ldo, n_items, (int)C,
                     lg, sd, rng);
  if (sd.threshold > 0) RGBX_FA_COMBINE(0, x0, ldx0, eps, nullptr, nullptr, nullptr, out, ldo);
  RGBX_CHECK_LAUNCH("fa_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* w, const float* x,
                                       int64_t ldx, const float* alr, const float* gout, int64_t ldg, float* g_alr,
                                       int64_t N, int64_t C, const uint32_t* seed, float p_drop,
                                       const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = fa_check(N, C, true, "faconv_bwd_dst")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !w || !x || !alr || !gout || !g_alr) return fail(RGBX_E_ARG, "faconv_bwd_dst: null pointer");
  if (int rc = fa_aligned(C, {x, gout}, {ldx, ldg}, "faconv_bwd_dst")) return rc;
  if (reinterpret_cast<uintptr_t>(alr) % 8) return fail(RGBX_E_ALIGN, "faconv_bwd_dst: alr must be 8-byte aligned");
  AttnSplit sd;
  if (int rc = fa_split_view(split, C, &sd, "faconv_bwd_dst")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "faconv_bwd_dst")) return rc;
  const int vec = fa_vec(C), lg = fa_lg(C, vec);
  hipStream_t s = (hipStream_t)stream;
  const float2* a2 = reinterpret_cast<const float2*>(alr);
  RGBX_ATTN_DISPATCH(fa_bwd_dst_kernel, row_grid, N, rowptr, col, w, x, ldx, a2, gout, ldg, g_alr, n_items, (int)C, lg,
                     sd, rng);
  if (sd.threshold > 0) RGBX_FA_COMBINE(1, nullptr, 0, 0.f, nullptr, nullptr, g_alr, nullptr, 0);
  RGBX_CHECK_LAUNCH("fa_bwd_dst_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* w_t,
                                       const int32_t* t2f, const float* x, int64_t ldx, const float* alr,
                                       const float* gout, int64_t ldg, const float* att_l, const float* att_r,
                                       float* g_alr, float* g_x, int64_t ldgx, int64_t N, int64_t C,
                                       const uint32_t* seed, float p_drop, const rgbx_row_split_t* split,
                                       rgbx_stream_t stream) {
  if (int rc = fa_check(N, C, true, "faconv_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !w_t || !x || !alr || !gout || !att_l || !att_r || !g_alr || !g_x)
    return fail(RGBX_E_ARG, "faconv_bwd_src: null pointer");
  if (seed && !t2f) return fail(RGBX_E_ARG, "faconv_bwd_src: training mode needs the slot map");
  if (g_x == gout || g_x == x) return fail(RGBX_E_ARG, "faconv_bwd_src: g_x must not alias gout or x");
  if (int rc = fa_aligned(C, {x, gout, g_x, att_l, att_r}, {ldx, ldg, ldgx}, "faconv_bwd_src")) return rc;
  if (reinterpret_cast<uintptr_t>(alr) % 8) return fail(RGBX_E_ALIGN, "faconv_bwd_src: alr must be 8-byte aligned");
  AttnSplit sd;
  if (int rc = fa_split_view(split, C, &sd, "faconv_bwd_src")) return rc;
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "faconv_bwd_src")) return rc;
  const int vec = fa_vec(C), lg = fa_lg(C, vec);
  hipStream_t s = (hipStream_t)stream;
  const float2* a2 = reinterpret_cast<const float2*>(alr);
  RGBX_ATTN_DISPATCH(fa_bwd_src_kernel, row_grid, N, rowptr_t, col_t, w_t, t2f, x, ldx, a2, gout, ldg, att_l, att_r,
                     g_alr, g_x, ldgx, n_items, (int)C, lg, sd, rng);
  if (sd.threshold > 0) RGBX_FA_COMBINE(2, nullptr, 0, 0.f, att_l, att_r, g_alr, g_x, ldgx);
  RGBX_CHECK_LAUNCH("fa_bwd_src_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_edge_coef_f32(const int32_t* rowptr, const int32_t* col, const float* w,
                                         const int32_t* slot, const float* alr, int transposed, int64_t N,
                                         const uint32_t* seed, float p_drop, float* coef, float* q,
                                         rgbx_stream_t stream) {
  if (int rc = fa_check(N, 1, false, "faconv_edge_coef")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !w || !alr || !coef) return fail(RGBX_E_ARG, "faconv_edge_coef: null pointer");
  if (reinterpret_cast<uintptr_t>(alr) % 8) return fail(RGBX_E_ALIGN, "faconv_edge_coef: alr must be 8-byte aligned");
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "faconv_edge_coef")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float2* a2 = reinterpret_cast<const float2*>(alr);
  const int grid = row_grid(N);
  if (seed) fa_edge_coef_kernel<true><<<grid, 256, 0, s>>>(rowptr, col, w, slot, a2, transposed, (int)N, rng, coef, q);
  else fa_edge_coef_kernel<false><<<grid, 256, 0, s>>>(rowptr, col, w, slot, a2, transposed, (int)N, rng, coef, q);
  RGBX_CHECK_LAUNCH("fa_edge_coef_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_edge_dot_f32(const int32_t* rowptr, const int32_t* col, const float* q, const float* a,
                                        int64_t lda, const float* b, int64_t ldb, float* out, int64_t out_stride,
                                        int64_t N, int64_t C, rgbx_stream_t stream) {
  if (int rc = fa_check(N, C, false, "faconv_edge_dot")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !q || !a || !b || !out) return fail(RGBX_E_ARG, "faconv_edge_dot: null pointer");
  if (out_stride < 1) return fail(RGBX_E_ARG, "faconv_edge_dot: output stride < 1");
  if (int rc = fa_aligned(C, {a, b}, {lda, ldb}, "faconv_edge_dot")) return rc;
  fa_edge_dot_kernel<<<row_grid(N), 256, 0, (hipStream_t)stream>>>(rowptr, col, q, a, lda, b, ldb, out, out_stride,
                                                                  (int)N, (int)C);
  RGBX_CHECK_LAUNCH("fa_edge_dot_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_faconv_draws_u8(const uint32_t* seed, int64_t nnz, float p_drop, uint8_t* keep,
                                    rgbx_stream_t stream) {
  if (nnz < 0) return fail(RGBX_E_ARG, "faconv_draws: bad size");
  if (nnz == 0) return RGBX_OK;
  if (nnz >= INT32_MAX) return fail(RGBX_E_RANGE, "faconv_draws: E' exceeds int32");
  if (!seed || !keep) return fail(RGBX_E_ARG, "faconv_draws: null pointer");
  AttnRng rng;
  if (int rc = make_rng(seed, p_drop, &rng, "faconv_draws")) return rc;
  const int grid = capped_grid(nnz, 256);
  fa_draws_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(seed, nnz, rng, keep);
  RGBX_CHECK_LAUNCH("fa_draws_kernel");
  return RGBX_OK;
}
