// CGConv (crystal graph convolution): fused gated softplus edge message + aggregation + root term, and its backward,
// for gfx950. Stands in for CGConv.forward / message [PyG] (Xie & Grossman, "Crystal Graph Convolutional Neural
// Networks for an Accurate and Interpretable Prediction of Material Properties").
//
// The layer's two Linear maps act on cat([x_i, x_j, e_ij]), so each splits into a target, a source and an edge term.
// For an edge j -> i in forward CSR slot p, with a, b [N, 2C] and c [nnz, 2C] (ONE ROW PER SLOT, in forward slot order;
// every row is (f half | s half); each operand its own pointer and leading dimension; c may be absent):
//   zf = a_f[i,:] + b_f[j,:] + c_f[p,:]        zs = a_s[i,:] + b_s[j,:] + c_s[p,:]
//   msg_p    = sigmoid(zf) (.) softplus(zs)                      (a VECTOR per edge: one gate per channel)
//   out[i,:] = root[i,:] + scale_i * sum_p msg_p                 scale_i = 1 (add) or 1 / deg_i (mean; 0 for deg_i = 0)
// The lane layout is attn_common.h's with H = 1 (a row fragment of VEC channels per lane, G lanes per neighbour row,
// 64 / G rows per wave-instruction), and a lane never talks to its neighbours inside a slot: it holds the f and the s
// fragment of the same channels. The target's a row stays in registers, the b row of the source is gathered and the c
// rows of a target are consecutive, so the forward and the target-side pass read them as a stream; only the source-side
// pass, which walks the transposed CSR, gathers them (through t2f). The edges are taken as given, so a row may have no
// slot at all: it stores the root term alone (zeros without one).
//
// Nothing per edge is saved and no record passes between the kernels: both backward passes recompute both branches from
// a, b, c. The mean's 1 / deg_i comes from rowptr inside the kernels (no host read: a captured launch stays valid). No
// float atomics; every sum runs in a fixed order (slots of a lane group in slot order, lane groups by a butterfly,
// hub-row chunks in chunk order, the root term on the row's first chunk).
#include <cmath>

#include "edge_common.h"

namespace rgbx {
namespace {

// Both branches go through e = exp(-|z|) in [0, 1], so nothing on the way can overflow, whatever z is:
//   sigmoid(z)  = (z >= 0 ? 1 : e) / (1 + e)     the denominator stays in [1, 2]; once e underflows to 0 the gate is
//                                                exactly 0 or 1 (resgated.hip's gate)
//   softplus(z) = max(z, 0) + log(1 + e)         log(1 + e) in [0, ln 2]
// exp, log and the reciprocal are the hardware's (v_exp_f32, v_log_f32, v_rcp_f32, about 1 ulp each) and not the
// correctly rounded library calls: with expf / log1pf / an IEEE division the kernels were VALU-bound, the forward at
// three times rgbx_resgated_fwd_f32 of the same run; with these it runs level with it (DESIGN 3.27,
// profiles/cgconv_bench_L.txt). The rounding of 1 + e costs softplus an ABSOLUTE error of at most 2^-24 per slot (a
// relative one only where softplus itself is below 1e-3); log(u) * e / (u - 1) would put it back and was measured too:
// + 20 % on the forward without the edge term, with the same measured error against float64 to four digits.
__device__ __forceinline__ float exp_neg_abs(float z) { return __expf(-fabsf(z)); }
__device__ __forceinline__ float sigmoid_e(float z, float e) { return __fdividef(z >= 0.f ? 1.f : e, 1.f + e); }
__device__ __forceinline__ float softplus_e(float z, float e) { return fmaxf(z, 0.f) + __logf(1.f + e); }

__device__ __forceinline__ float message(float zf, float zs) {
  return sigmoid_e(zf, exp_neg_abs(zf)) * softplus_e(zs, exp_neg_abs(zs));
}

// (d msg / d zf, d msg / d zs) = (s (1 - s) t, s u) with s = sigmoid(zf), t = softplus(zs), u = sigmoid(zs); the one
// exp(-|zs|) serves t and u.
__device__ __forceinline__ void message_grad(float zf, float zs, float& df, float& ds) {
  const float s = sigmoid_e(zf, exp_neg_abs(zf));
  const float es = exp_neg_abs(zs);
  df = s * (1.f - s) * softplus_e(zs, es);
  ds = s * sigmoid_e(zs, es);
}

// 1 / deg of a row of the FORWARD CSR (the whole row, also from inside a chunk); 0 for a row without slots.
__device__ __forceinline__ float row_scale(const int* __restrict__ rowptr, int row, bool mean) {
  if (!mean) return 1.f;
  const int deg = rowptr[row + 1] - rowptr[row];
  return deg > 0 ? 1.f / (float)deg : 0.f;
}

// ------------------------------------------------------------------------------------------
// Forward over the target-grouped CSR: the target's a row (both halves) stays in registers, per slot the two halves of
// the source's b row are gathered and the slot's c row streamed (U slots in flight per lane group). EDGE: c is there.
// CHUNK: the wave owns a chunk of a hub row and leaves its scaled partial sum; the chunk that starts the row carries the
// root term, so the combine kernel only adds.
template <int VEC, bool CHUNK, bool EDGE>
__global__ void __launch_bounds__(256)
cgconv_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ a, int64_t lda,
                  const float* __restrict__ b, int64_t ldb, const float* __restrict__ c, int64_t ldc,
                  const float* __restrict__ root, int64_t ldr, float* __restrict__ out, int64_t ldo, int N, bool mean,
                  const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;  // slots in flight per lane group (two b fragments and two c fragments each)
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;  // H = 1: the group is the head, t / LPH = 0
  const int C = L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float af[VEC], as[VEC], acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) af[i] = as[i] = acc[i] = 0.f;
    if (active) {
      load_vec<VEC>(af, a + (int64_t)row * lda + ch);
      load_vec<VEC>(as, a + (int64_t)row * lda + C + ch);
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float zf[U][VEC], zs[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) zf[u][i] = zs[u][i] = 0.f;
          if (active && idx < n) {
            load_vec<VEC>(zf[u], b + (int64_t)src * ldb + ch);
            load_vec<VEC>(zs[u], b + (int64_t)src * ldb + C + ch);
            if constexpr (EDGE) {
              float cf[VEC], cs[VEC];
              load_vec<VEC>(cf, c + (int64_t)(base + idx) * ldc + ch);
              load_vec<VEC>(cs, c + (int64_t)(base + idx) * ldc + C + ch);
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                zf[u][i] += cf[i];
                zs[u][i] += cs[i];
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // the message of all-zero inputs is sigmoid(a_f) softplus(a_s), not zero: a slot past the row's end adds nothing
          // only because it is skipped here
          if (active && k + u * NG + g < n) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += message(af[i] + zf[u][i], as[i] + zs[u][i]);
          }
        }
      }
    }
    groups_sum<VEC>(acc, L.G);
    if (g == 0 && active) {
      const float scale = row_scale(rowptr, row, mean);
      bool with_root = root != nullptr;
      if constexpr (CHUNK) with_root = with_root && start == rowptr[row];
      float ri[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) ri[i] = 0.f;
      if (with_root) load_vec<VEC>(ri, root + (int64_t)row * ldr + ch);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(scale, acc[i], ri[i]);
      if constexpr (CHUNK) store_vec<VEC>(sp.pacc + (int64_t)item * F + ch, acc);
      else store_vec<VEC>(out + (int64_t)row * ldo + ch, acc);  // rows without slots: the root term (or zeros), written
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward. With w_i = scale_i gout[i,:] and (df_p, ds_p) the message's derivatives at slot p:
//   gf_p = w_i (.) df_p,  gs_p = w_i (.) ds_p
//   g_a[i,:] = (sum_p gf_p | sum_p gs_p)     g_c[p,:] = (gf_p | gs_p)     g_b[j,:] = (sum_q gf_q | sum_q gs_q)
//
// Target side, over the forward CSR (row = target i): the same reads as the forward; the row's w fragment stays in
// registers. g_a and g_c are each optional (NULL: not wanted) and come from the same registers. A chunk's record is
// (gf sum | gs sum); a slot is owned by exactly one item (its row, or one chunk of its hub row), which writes its g_c
// row once.
template <int VEC, bool CHUNK, bool EDGE>
__global__ void __launch_bounds__(256)
cgconv_bwd_dst_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ a,
                      int64_t lda, const float* __restrict__ b, int64_t ldb, const float* __restrict__ c, int64_t ldc,
                      const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_a, int64_t ldga,
                      float* __restrict__ g_c, int64_t ldgc, int N, bool mean, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 4;
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;
  const int C = L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr, sp, item, row, start, end)) continue;
    float af[VEC], as[VEC], w[VEC], sf[VEC], ss[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) af[i] = as[i] = w[i] = sf[i] = ss[i] = 0.f;
    if (active) {
      load_vec<VEC>(af, a + (int64_t)row * lda + ch);
      load_vec<VEC>(as, a + (int64_t)row * lda + C + ch);
      load_vec<VEC>(w, gout + (int64_t)row * ldg + ch);
      const float scale = row_scale(rowptr, row, mean);
#pragma unroll
      for (int i = 0; i < VEC; ++i) w[i] *= scale;
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float zf[U][VEC], zs[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) zf[u][i] = zs[u][i] = 0.f;
          if (active && idx < n) {
            load_vec<VEC>(zf[u], b + (int64_t)src * ldb + ch);
            load_vec<VEC>(zs[u], b + (int64_t)src * ldb + C + ch);
            if constexpr (EDGE) {
              float cf[VEC], cs[VEC];
              load_vec<VEC>(cf, c + (int64_t)(base + idx) * ldc + ch);
              load_vec<VEC>(cs, c + (int64_t)(base + idx) * ldc + C + ch);
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                zf[u][i] += cf[i];
                zs[u][i] += cs[i];
              }
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          if (active && idx < n) {  // a slot past the row's end is skipped: its derivative is not zero
            float gf[VEC], gs[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              float df, ds;
              message_grad(af[i] + zf[u][i], as[i] + zs[u][i], df, ds);
              gf[i] = w[i] * df;
              gs[i] = w[i] * ds;
              sf[i] += gf[i];
              ss[i] += gs[i];
            }
            if (g_c) {
              store_vec<VEC>(g_c + (int64_t)(base + idx) * ldgc + ch, gf);
              store_vec<VEC>(g_c + (int64_t)(base + idx) * ldgc + C + ch, gs);
            }
          }
        }
      }
    }
    if (!g_a) continue;  // (uniform) only the per-slot rows were wanted
    groups_sum<VEC>(sf, L.G);
    groups_sum<VEC>(ss, L.G);
    if (g == 0 && active) {
      if constexpr (CHUNK) {
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + ch, sf);
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + F + ch, ss);
      } else {
        store_vec<VEC>(g_a + (int64_t)row * ldga + ch, sf);  // rows without slots: zeros, written
        store_vec<VEC>(g_a + (int64_t)row * ldga + C + ch, ss);
      }
    }
  }
}

// Source side, over the TRANSPOSED CSR (row = source j, col_t[q] = target i, t2f[q] = the edge's forward slot): the
// source's own b row stays in registers; the a and gout rows of the target and the c row of the edge are gathered per
// slot. The target's 1 / deg comes from the FORWARD rowptr (one read per lane beside col_t, handed round by shuffle). A
// chunk's record is (gf sum | gs sum). A source without out-edges stores zeros.
template <int VEC, bool CHUNK, bool EDGE>
__global__ void __launch_bounds__(256)
cgconv_bwd_src_kernel(const int* __restrict__ rowptr_t, const int* __restrict__ col_t, const int* __restrict__ t2f,
                      const int* __restrict__ rowptr_f, const float* __restrict__ a, int64_t lda,
                      const float* __restrict__ b, int64_t ldb, const float* __restrict__ c, int64_t ldc,
                      const float* __restrict__ gout, int64_t ldg, float* __restrict__ g_b, int64_t ldgb, int N,
                      bool mean, const GatLayout L, const AttnSplit sp) {
  constexpr int U = 2;  // five gathered fragments per slot: two in flight keep the kernel at the forward's register count
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
  const bool active = ch < L.C;
  const int C = L.C;

  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < N; item += gridDim.x * wpb) {
    int row, start, end;
    if (!row_item<CHUNK>(rowptr_t, sp, item, row, start, end)) continue;
    float bf[VEC], bs[VEC], sf[VEC], ss[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) bf[i] = bs[i] = sf[i] = ss[i] = 0.f;
    if (active) {
      load_vec<VEC>(bf, b + (int64_t)row * ldb + ch);
      load_vec<VEC>(bs, b + (int64_t)row * ldb + C + ch);
    }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? col_t[base + lane] : 0;
      int myslot = 0;
      if constexpr (EDGE) myslot = lane < n ? t2f[base + lane] : 0;
      float myscale = 1.f;  // the target has this edge, so its degree is >= 1
      if (mean && lane < n) myscale = 1.f / (float)(rowptr_f[mycol + 1] - rowptr_f[mycol]);
      for (int k = 0; k < n; k += NG * U) {
        float zf[U][VEC], zs[U][VEC], w[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int tgt = __shfl(mycol, idx & 63);
          const int slot = __shfl(myslot, idx & 63);
          const float scale = __shfl(myscale, idx & 63);
#pragma unroll
          for (int i = 0; i < VEC; ++i) zf[u][i] = zs[u][i] = w[u][i] = 0.f;
          if (active && idx < n) {
            load_vec<VEC>(zf[u], a + (int64_t)tgt * lda + ch);
            load_vec<VEC>(zs[u], a + (int64_t)tgt * lda + C + ch);
            load_vec<VEC>(w[u], gout + (int64_t)tgt * ldg + ch);
            if constexpr (EDGE) {
              float cf[VEC], cs[VEC];
              load_vec<VEC>(cf, c + (int64_t)slot * ldc + ch);
              load_vec<VEC>(cs, c + (int64_t)slot * ldc + C + ch);
#pragma unroll
              for (int i = 0; i < VEC; ++i) {  // the forward's order of adds: (a + (b + c))
                zf[u][i] = zf[u][i] + (bf[i] + cf[i]);
                zs[u][i] = zs[u][i] + (bs[i] + cs[i]);
              }
            } else {
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                zf[u][i] += bf[i];
                zs[u][i] += bs[i];
              }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) w[u][i] *= scale;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (active && k + u * NG + g < n) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              float df, ds;
              message_grad(zf[u][i], zs[u][i], df, ds);
              sf[i] = fmaf(w[u][i], df, sf[i]);
              ss[i] = fmaf(w[u][i], ds, ss[i]);
            }
          }
        }
      }
    }
    groups_sum<VEC>(sf, L.G);
    groups_sum<VEC>(ss, L.G);
    if (g == 0 && active) {
      if constexpr (CHUNK) {
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + ch, sf);
        store_vec<VEC>(sp.pacc + (int64_t)item * 2 * F + F + ch, ss);
      } else {
        store_vec<VEC>(g_b + (int64_t)row * ldgb + ch, sf);  // sources without out-edges: zeros, written
        store_vec<VEC>(g_b + (int64_t)row * ldgb + C + ch, ss);
      }
    }
  }
}

// KERNEL<V, CHUNK, EDGE> through the shared ladder (edge_common.h), EDGE = the run-time `edge` as a constant.
#define RGBX_CGCONV_ROWS(KERNEL, edge, n_rows, ...)                          \
  do {                                                                       \
    if (edge) RGBX_EDGE_ROWS_X(KERNEL, (true), n_rows, __VA_ARGS__);         \
    else RGBX_EDGE_ROWS_X(KERNEL, (false), n_rows, __VA_ARGS__);             \
  } while (0)

int check_sizes(int64_t N, int C, int mean, const char* name) {
  if (int rc = check_sizes(N, C, name)) return rc;
  if (mean != 0 && mean != 1) return fail(RGBX_E_ARG, "%s: mean must be 0 or 1", name);
  return RGBX_OK;
}

// The a / b / c operands are (f half | s half) rows: 2C floats wide.
int check_operands(int C, const float* c, int64_t lda, int64_t ldb, int64_t ldc, const char* name) {
  if (lda < 2 * (int64_t)C || ldb < 2 * (int64_t)C) return fail(RGBX_E_ARG, "%s: leading dimension of a / b < 2C", name);
  if (c && ldc < 2 * (int64_t)C) return fail(RGBX_E_ARG, "%s: c given with a leading dimension < 2C", name);
  return RGBX_OK;
}

// pick_vec took the widest vector the pointers and leading dimensions allow; the row must still fit a wave at it.
int check_vec(int C, int vec, const char* name) {
  if (C > kWave * vec)
    return fail(RGBX_E_ALIGN,
                "%s: %d channels need %d-float vectors (pointers on %d-byte boundaries, leading dimensions %% %d == 0); "
                "the operands allow %d",
                name, C, C > 2 * kWave ? 4 : 2, C > 2 * kWave ? 16 : 8, C > 2 * kWave ? 4 : 2, vec);
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_cgconv_supported(int C) { return head_width_supported(C); }

extern "C" int rgbx_cgconv_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda,
                                   const float* b, int64_t ldb, const float* c, int64_t ldc, const float* root,
                                   int64_t ldr, float* out, int64_t ldo, int64_t N, int C, int mean,
                                   const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, mean, "cgconv_fwd")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !a || !b || !out) return fail(RGBX_E_ARG, "cgconv_fwd: null pointer");
  if (int rc = check_operands(C, c, lda, ldb, ldc, "cgconv_fwd")) return rc;
  if (ldo < C || (root && ldr < C)) return fail(RGBX_E_ARG, "cgconv_fwd: leading dimension of out / root < C");
  if (!aligned_to({a, b, c, root, out}, 4))
    return fail(RGBX_E_ALIGN, "cgconv_fwd: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "cgconv_fwd")) return rc;
  const int vec = pick_vec(C, {a, b, c, root, out, sd.pacc}, {lda, ldb, c ? ldc : 0, root ? ldr : 0, ldo});
  if (int rc = check_vec(C, vec, "cgconv_fwd")) return rc;
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "cgconv_fwd")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_CGCONV_ROWS(cgconv_fwd_kernel, c != nullptr, N, rowptr, col, a, lda, b, ldb, c, ldc, root, ldr, out, ldo,
                   n_items, mean != 0, L, sd);
  if (sd.threshold > 0) RGBX_ATTN_BWD_COMBINE(out, ldo, C, 0);  // a plain sum: the chunk partials added in chunk order
  RGBX_CHECK_LAUNCH("cgconv_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_cgconv_bwd_dst_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda,
                                       const float* b, int64_t ldb, const float* c, int64_t ldc, const float* gout,
                                       int64_t ldg, float* g_a, int64_t ldga, float* g_c, int64_t ldgc, int64_t N,
                                       int C, int mean, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, mean, "cgconv_bwd_dst")) return rc;
  if (!g_a && !g_c) return fail(RGBX_E_ARG, "cgconv_bwd_dst: neither g_a nor g_c is wanted");
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !a || !b || !gout) return fail(RGBX_E_ARG, "cgconv_bwd_dst: null pointer");
  if (int rc = check_operands(C, c, lda, ldb, ldc, "cgconv_bwd_dst")) return rc;
  if (ldg < C) return fail(RGBX_E_ARG, "cgconv_bwd_dst: leading dimension of gout < C");
  if ((g_a && ldga < 2 * (int64_t)C) || (g_c && ldgc < 2 * (int64_t)C))
    return fail(RGBX_E_ARG, "cgconv_bwd_dst: leading dimension of g_a / g_c < 2C");
  if (!aligned_to({a, b, c, gout, g_a, g_c}, 4))
    return fail(RGBX_E_ALIGN, "cgconv_bwd_dst: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "cgconv_bwd_dst")) return rc;
  const int vec = pick_vec(C, {a, b, c, gout, g_a, g_c, sd.pacc},
                           {lda, ldb, c ? ldc : 0, ldg, g_a ? ldga : 0, g_c ? ldgc : 0});
  if (int rc = check_vec(C, vec, "cgconv_bwd_dst")) return rc;
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "cgconv_bwd_dst")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_CGCONV_ROWS(cgconv_bwd_dst_kernel, c != nullptr, N, rowptr, col, a, lda, b, ldb, c, ldc, gout, ldg, g_a, ldga,
                   g_c, ldgc, n_items, mean != 0, L, sd);
  if (sd.threshold > 0 && g_a) {  // a chunk's record is (gf sum | gs sum)
    RGBX_ATTN_BWD_COMBINE(g_a, ldga, 2 * (int64_t)C, 0);
    RGBX_ATTN_BWD_COMBINE(g_a + C, ldga, 2 * (int64_t)C, C);
  }
  RGBX_CHECK_LAUNCH("cgconv_bwd_dst_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_cgconv_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                       const int32_t* rowptr_f, const float* a, int64_t lda, const float* b,
                                       int64_t ldb, const float* c, int64_t ldc, const float* gout, int64_t ldg,
                                       float* g_b, int64_t ldgb, int64_t N, int C, int mean,
                                       const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (int rc = check_sizes(N, C, mean, "cgconv_bwd_src")) return rc;
  if (N == 0) return RGBX_OK;
  if (!rowptr_t || !col_t || !a || !b || !gout || !g_b) return fail(RGBX_E_ARG, "cgconv_bwd_src: null pointer");
  if (c && !t2f) return fail(RGBX_E_ARG, "cgconv_bwd_src: c given without t2f");
  if (mean && !rowptr_f) return fail(RGBX_E_ARG, "cgconv_bwd_src: mean needs the forward rowptr");
  if (int rc = check_operands(C, c, lda, ldb, ldc, "cgconv_bwd_src")) return rc;
  if (ldg < C) return fail(RGBX_E_ARG, "cgconv_bwd_src: leading dimension of gout < C");
  if (ldgb < 2 * (int64_t)C) return fail(RGBX_E_ARG, "cgconv_bwd_src: leading dimension of g_b < 2C");
  if (!aligned_to({a, b, c, gout, g_b}, 4))
    return fail(RGBX_E_ALIGN, "cgconv_bwd_src: float pointers must be 4-byte aligned");
  AttnSplit sd;
  if (int rc = split_view(split, 1, C, 0, &sd, "cgconv_bwd_src")) return rc;
  const int vec = pick_vec(C, {a, b, c, gout, g_b, sd.pacc}, {lda, ldb, c ? ldc : 0, ldg, ldgb});
  if (int rc = check_vec(C, vec, "cgconv_bwd_src")) return rc;
  GatLayout L;
  if (int rc = make_layout(1, C, vec, &L, "cgconv_bwd_src")) return rc;
  hipStream_t s = (hipStream_t)stream;
  RGBX_CGCONV_ROWS(cgconv_bwd_src_kernel, c != nullptr, N, rowptr_t, col_t, t2f, rowptr_f, a, lda, b, ldb, c, ldc,
                   gout, ldg, g_b, ldgb, n_items, mean != 0, L, sd);
  if (sd.threshold > 0) {
    RGBX_ATTN_BWD_COMBINE(g_b, ldgb, 2 * (int64_t)C, 0);
    RGBX_ATTN_BWD_COMBINE(g_b + C, ldgb, 2 * (int64_t)C, C);
  }
  RGBX_CHECK_LAUNCH("cgconv_bwd_src_kernel");
  return RGBX_OK;
}
