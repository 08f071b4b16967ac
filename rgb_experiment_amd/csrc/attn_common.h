// What the fused attention families (supergat.hip, gatv2.hip, transformer.hip, faconv.hip) share: the lane layout, the
// online-softmax arithmetic, the hub-row plan (row kernel, chunk kernel, combine kernel) and the host-side checks and
// launch ladder. Everything has internal linkage: each translation unit launches its own copy of the kernels below and
// the library exports nothing from here. gat.hip does NOT include this header; it keeps its own copy of the layout
// code because its text keys the recorded counter measurements of its kernels (bench.py KERNEL_SOURCES).
#pragma once
#include "rgbx_common.h"
#include "rgbx_rng.h"

namespace rgbx {
namespace {

// Lane layout of one wave per CSR row: a head occupies LPH = pow2ceil(C / VEC) consecutive lanes of VEC channels, HPC
// heads sit side by side in a group of G lanes that reads one neighbour row per step, NG = 64 / G rows per
// wave-instruction.
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

// Sum of a row fragment over the NG lane groups of a wave, in a fixed order; group 0 ends with the total.
template <int VEC>
__device__ __forceinline__ void groups_sum(float (&acc)[VEC], int G) {
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
}

// (m, rden) = (0, 0) is the saved state of a row without slots: shift 0, and no slot to apply it to.
__device__ __forceinline__ float softmax_shift(float m, float rden) { return rden > 0.f ? m - logf(rden) : 0.f; }

// Online softmax: the state (m2, l2, a2(i)) = (running max, denominator, rescaled accumulator) merged into (m, l, acc).
// a2 is a callable so that each caller's reads stay where its statements had them: the group merge shuffles acc[i]
// inside the loop, the combine kernel reads a loaded fragment. Hoisting the shuffles changed which product of
// acc * s1 + a2 * s2 the compiler fuses into the multiply-add, and with it the bits.
template <int VEC, class A2>
__device__ __forceinline__ void softmax_merge(float& m, float& l, float (&acc)[VEC], float m2, float l2, A2 a2) {
  const float mn = fmaxf(m, m2);
  const float s1 = expf(m - mn), s2 = expf(m2 - mn);
  l = l * s1 + l2 * s2;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = acc[i] * s1 + a2(i) * s2;
  m = mn;
}

// The NG online-softmax states of a wave merged in a fixed order; group 0 ends with the row's state.
template <int VEC>
__device__ __forceinline__ void softmax_merge_groups(float& m, float& l, float (&acc)[VEC], int G) {
  for (int off = 32; off >= G; off >>= 1) {
    const float m2 = __shfl_xor(m, off);
    const float l2 = __shfl_xor(l, off);
    softmax_merge<VEC>(m, l, acc, m2, l2, [&](int i) { return __shfl_xor(acc[i], off); });
  }
}

// Attention dropout: the keep of (forward CSR slot, head) on the caller's stream constant. mix32 / draw32 / unit24:
// rgbx_rng.h. GATv2 and TransformerConv share kStreamAttnDrop (rgbx_gatv2_draws_u8 writes the decisions of both out);
// SuperGAT and FAConv draw on constants of their own.
constexpr uint32_t kStreamAttnDrop = 0xA4093822u;

template <uint32_t STREAM>
__device__ __forceinline__ bool drop_keep(uint32_t s0, uint32_t s1, int slot, int head, float p) {
  return unit24(draw32(s0, s1, STREAM, (uint32_t)slot, (uint32_t)head)) >= p;
}

// The hub-row plan as the kernels see it. A chunk's partial record is pacc (a row fragment per chunk) followed by up to
// two per-(chunk, head) scalars.
struct AttnSplit {
  int threshold;
  const int* chunk_row;
  const int* chunk_begin;
  const int* chunk_end;
  float* pacc;  // [n_chunks, F] (transformer's source side: [n_chunks, 2F])
  float* p0;    // [n_chunks, H]  (forward: running max; supergat / faconv backward: the scalar sum)
  float* p1;    // [n_chunks, H]  (forward only: denominator)
};

// Training-mode state of one forward: `seed` = two 32-bit words on the device (NULL: no dropout).
struct AttnRng {
  const uint32_t* seed;
  float p_drop;
  float inv_keep;  // 1 / (1 - p_drop)
};

// This lane's place in the layout.
struct LaneCoords {
  int lane, NG, g, t, hl, ch, wpb, F;
};

template <int VEC>
__device__ __forceinline__ LaneCoords lane_coords(const GatLayout L) {
  LaneCoords c;
  c.lane = threadIdx.x & 63;
  c.NG = kWave / L.G;
  c.g = c.lane / L.G;
  c.t = c.lane % L.G;
  c.hl = c.t / L.LPH;
  c.ch = (c.t % L.LPH) * VEC;
  c.wpb = blockDim.x >> 6;
  c.F = L.H * L.C;
  return c;
}

// The row (or hub-row chunk) a wave owns. false: a hub row met by the row kernel, whose sums the chunk + combine
// kernels own.
template <bool CHUNK>
__device__ __forceinline__ bool row_item(const int* __restrict__ rowptr, const AttnSplit sp, int item, int& row,
                                         int& start, int& end) {
  if constexpr (CHUNK) {
    row = __builtin_amdgcn_readfirstlane(sp.chunk_row[item]);
    start = __builtin_amdgcn_readfirstlane(sp.chunk_begin[item]);
    end = __builtin_amdgcn_readfirstlane(sp.chunk_end[item]);
    return true;
  } else {
    row = item;
    start = __builtin_amdgcn_readfirstlane(rowptr[row]);
    end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    return !(sp.threshold > 0 && end - start > sp.threshold);
  }
}

// One wave per hub row: merge the chunk states in chunk order, normalise, store. BIAS: the family has a bias, which may
// still be NULL (the add of zeros stays, as in the row kernels); without it the store is the bare product. m_out /
// rden_out may be NULL.
template <int VEC, bool BIAS>
__global__ void __launch_bounds__(256)
attn_fwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                        const float* __restrict__ bias, float* __restrict__ out, int64_t ldo,
                        float* __restrict__ m_out, float* __restrict__ rden_out, const GatLayout L,
                        const AttnSplit sp) {
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
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
        softmax_merge<VEC>(m, l, acc, m2, l2, [&](int i) { return a2[i]; });
      }
      const float rd = l > 0.f ? 1.0f / (l + 1e-16f) : 0.f;
      if constexpr (BIAS) {
        float bv[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) bv[i] = 0.f;
        if (bias) load_vec<VEC>(bv, bias + cofs);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = acc[i] * rd + bv[i];
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] *= rd;
      }
      store_vec<VEC>(out + (int64_t)row * ldo + cofs, acc);
      if (m_out && ch == 0) {
        m_out[(int64_t)row * L.H + head] = l > 0.f ? m : 0.f;
        rden_out[(int64_t)row * L.H + head] = rd;
      }
    }
  }
}

// One wave per hub row of a backward pass: chunk sums added in chunk order. A chunk's record is `stride` floats wide
// and this output's sums start `ofs` floats into it.
template <int VEC>
__global__ void __launch_bounds__(256)
attn_bwd_combine_kernel(int n_long, const int* __restrict__ long_row, const int* __restrict__ long_chunk_ptr,
                        float* __restrict__ gx, int64_t ldgx, int64_t stride, int64_t ofs, const GatLayout L,
                        const AttnSplit sp) {
  const auto [lane, NG, g, t, hl, ch, wpb, F] = lane_coords<VEC>(L);
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

// ---- host side ---------------------------------------------------------------------------------------------------

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

// Grid-stride kernels, and row kernels that leave one record per workgroup: `per_block` items a block, capped.
int capped_grid(int64_t n, int per_block) {
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

// Head widths the layout covers: up to 64 lanes per head at the widest vector that divides C.
bool head_width_supported(int64_t C) {
  return C > 0 && (C <= 64 || (C % 2 == 0 && C <= 128) || (C % 4 == 0 && C <= 256));
}

int fail_head_width(const char* name, int C) {
  return fail(RGBX_E_SHAPE, "%s: %d channels per head (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)", name, C);
}

// `scalars`: how many of p0, p1 follow the [n_chunks, H * C] fragments in split->partial.
int split_view(const rgbx_row_split_t* split, int H, int C, int scalars, AttnSplit* sd, const char* name) {
  *sd = AttnSplit{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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
  if (scalars > 0) sd->p0 = sd->pacc + (int64_t)split->n_chunks * F;
  if (scalars > 1) sd->p1 = sd->p0 + (int64_t)split->n_chunks * H;
  return RGBX_OK;
}

int make_rng(const uint32_t* seed, float p_drop, AttnRng* rng, const char* name) {
  *rng = AttnRng{seed, p_drop, 1.0f};
  if (!seed) return RGBX_OK;
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(RGBX_E_ARG, "%s: dropout must be in [0, 1)", name);
  rng->inv_keep = 1.0f / (1.0f - p_drop);
  return RGBX_OK;
}

// The statement with V = the vector width `vec` as a constant.
#define RGBX_VEC_SWITCH(vec, ...)      \
  do {                                 \
    if ((vec) == 4) {                  \
      constexpr int V = 4;             \
      __VA_ARGS__;                     \
    } else if ((vec) == 2) {           \
      constexpr int V = 2;             \
      __VA_ARGS__;                     \
    } else {                           \
      constexpr int V = 1;             \
      __VA_ARGS__;                     \
    }                                  \
  } while (0)

// KERNEL<V, CHUNK, TRAIN> over the rows and then, with a split plan, over the hub-row chunks, each on GRID(items)
// workgroups. The argument list is written once: in it `n_items` is the pass's item count and `chunk_pass` tells the
// two passes apart. Expects `s`, `sd` and `split` in scope.
#define RGBX_ATTN_ROWS(KERNEL, V, T, GRID, n_rows, ...)                     \
  do {                                                                      \
    {                                                                       \
      const int n_items = (int)(n_rows);                                    \
      constexpr bool chunk_pass = false;                                    \
      (void)chunk_pass;                                                     \
      KERNEL<V, false, T><<<GRID(n_items), 256, 0, s>>>(__VA_ARGS__);       \
    }                                                                       \
    if (sd.threshold > 0) {                                                 \
      const int n_items = split->n_chunks;                                  \
      constexpr bool chunk_pass = true;                                     \
      (void)chunk_pass;                                                     \
      KERNEL<V, true, T><<<GRID(n_items), 256, 0, s>>>(__VA_ARGS__);        \
    }                                                                       \
  } while (0)

// The ladder over VEC in {4, 2, 1} x TRAIN (= a seed was given). Expects `vec` and `rng` in scope as well.
#define RGBX_ATTN_DISPATCH(KERNEL, GRID, n_rows, ...)                                      \
  RGBX_VEC_SWITCH(vec, if (rng.seed) RGBX_ATTN_ROWS(KERNEL, V, true, GRID, n_rows, __VA_ARGS__); \
                       else RGBX_ATTN_ROWS(KERNEL, V, false, GRID, n_rows, __VA_ARGS__))

// The hub rows' combine kernels, after the two passes above. Expect `vec`, `split`, `L`, `sd` and `s` in scope.
#define RGBX_ATTN_FWD_COMBINE(BIAS, bias, out, ldo, m, rden)                                        \
  RGBX_VEC_SWITCH(vec, attn_fwd_combine_kernel<V, BIAS><<<row_grid(split->n_long), 256, 0, s>>>(    \
                           split->n_long, split->long_row, split->long_chunk_ptr, bias, out, ldo, m, rden, L, sd))

#define RGBX_ATTN_BWD_COMBINE(gx, ldgx, stride, ofs)                                                \
  RGBX_VEC_SWITCH(vec, attn_bwd_combine_kernel<V><<<row_grid(split->n_long), 256, 0, s>>>(          \
                           split->n_long, split->long_row, split->long_chunk_ptr, gx, ldgx, stride, ofs, L, sd))

}  // namespace
}  // namespace rgbx
