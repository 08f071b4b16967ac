// Max / min neighbourhood aggregation over a CSR for gfx950, and its source-side backward.
//   forward : out[i,c] = max (or min) over the slots p of row i of x[col[p], c];  arg[i,c] = the slot p that supplied it
//   backward: gx[j,c]  = sum over the transposed slots q of row j of gout[col_t[q], c] * [arg[col_t[q], c] == t2f[q]]
// Replaces MessagePassing.propagate(aggr='max' | 'min') behind my_SAGEConv(..., aggr=...) (reference
// models/graphsage.py:38-40,58: kwargs.setdefault('aggr', 'mean') leaves the choice to the caller) and behind
// torch_geometric.nn.SAGEConv(aggr=...) (models/graphsage2.py:20-23). The first reduction of the library that is not a sum.
//
// Lane layout: the row gather's (spmm.hip, edge_dot.hip). One wave owns one target row, the wave is split into NG = 64/G
// groups of G lanes, a group reads ONE neighbour row per step with 16-byte loads, U steps are issued back to back, and the 64
// column indices of a row chunk are read once, coalesced, and handed to the groups with ds_bpermute. Where the gather adds,
// this kernel compares: every lane keeps (best value, slot of the best value) for its 4 columns.
//
// Ties: the LOWEST slot wins (what torch_scatter's CPU scatter_max does in edge order, the CSR build being a stable sort).
// A group meets its slots in ascending order and replaces on strict > / < only; the NG groups, and the chunks of a hub row, are
// then merged under "better value, or equal value and lower slot" — an order that does not depend on how the slots were dealt
// out, so the row split changes neither values nor arg. An extremum involves no rounding: the result is exact.
// Inputs are finite (no NaN policy): the running best starts at -inf / +inf, which every finite value beats.
//
// Backward: a row of the transposed CSR lists the targets i a source j feeds; the wave gathers gout[i,:] and arg[i,:] and adds
// the entries whose winning slot is this very edge (t2f[q] = forward slot of transposed slot q — matching the slot, not the
// source id, keeps duplicate edges j -> i from counting twice). Plain fixed-order sums, no float atomics: two runs give the
// same bits. Hub rows of either CSR go through the row-split plan (chunk kernel + combine in chunk order).
#include "rgbx_common.h"

namespace rgbx {
namespace {

using f4v = __attribute__((ext_vector_type(4))) float;
using i4v = __attribute__((ext_vector_type(4))) int;

__device__ __forceinline__ void load_ivec4(int (&v)[4], const int* p) {
  const int4 t = *reinterpret_cast<const int4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

__device__ __forceinline__ void store_ivec4(int* p, const int (&v)[4]) {
  *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
}

// `a` at slot `sa` beats `b` at slot `sb`: strictly better, or equal and from a lower slot (-1 = no slot: the highest unsigned)
template <bool MAX>
__device__ __forceinline__ bool beats(float a, int sa, float b, int sb) {
  const bool better = MAX ? a > b : a < b;
  return better || (a == b && (unsigned)sa < (unsigned)sb);
}

struct ExtArgs {
  const int* rowptr;
  const int* col;
  const float* x;
  float* out;
  int* arg;  // or NULL
  int64_t ldx, ldo;
  int N, d;
  int skip_longer;
};

// Slots [start, end): best / slot of this lane's 4 columns (base pointer xc), the NG groups merged on return.
template <int G, bool MAX>
__device__ __forceinline__ void extremum_slots(const ExtArgs& A, int start, int end, const float* xc, bool active, int lane,
                                               int g, float (&best)[4], int (&slot)[4]) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  constexpr float kWorst = MAX ? -INFINITY : INFINITY;
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int mycol = lane < n ? A.col[base + lane] : 0;
    for (int k = 0; k < n; k += NG * U) {
      float v[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int src = __shfl(mycol, idx & 63);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[u][i] = kWorst;  // never replaces
        if (active && idx < n) load_vec<4>(v[u], xc + (int64_t)src * A.ldx);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int p = base + k + u * NG + g;  // ascending within the group: strict comparison keeps the lowest slot
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool take = MAX ? v[u][i] > best[i] : v[u][i] < best[i];
          best[i] = take ? v[u][i] : best[i];
          slot[i] = take ? p : slot[i];
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ob = __shfl_xor(best[i], off);
      const int os = __shfl_xor(slot[i], off);
      const bool take = beats<MAX>(ob, os, best[i], slot[i]);
      best[i] = take ? ob : best[i];
      slot[i] = take ? os : slot[i];
    }
  }
}

// A row without slots aggregates 0 (PyG: nodes without in-edges), arg -1.
__device__ __forceinline__ void extremum_store(const ExtArgs& A, int row, int c, const float (&best)[4], const int (&slot)[4]) {
  f4v o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = slot[i] < 0 ? 0.f : best[i];
  __builtin_nontemporal_store(o, reinterpret_cast<f4v*>(A.out + (int64_t)row * A.ldo + c));
  if (A.arg) {
    i4v s = {slot[0], slot[1], slot[2], slot[3]};
    __builtin_nontemporal_store(s, reinterpret_cast<i4v*>(A.arg + (int64_t)row * A.d + c));
  }
}

template <int G, bool MAX>
__global__ void __launch_bounds__(256) extremum_kernel(const ExtArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;  // the chunk + combine kernels own long rows
  float best[4];
  int slot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = MAX ? -INFINITY : INFINITY; slot[i] = -1; }
  extremum_slots<G, MAX>(A, start, end, A.x + c, active, lane, g, best, slot);
  if (g == 0 && active) extremum_store(A, row, c, best, slot);
}

// One wave per chunk of a long row: (best, slot) of the chunk into pval / pslot [n_chunks, d].
template <int G, bool MAX>
__global__ void __launch_bounds__(256)
extremum_chunk_kernel(const ExtArgs A, int n_chunks, const int* __restrict__ chunk_begin,
                      const int* __restrict__ chunk_end, float* __restrict__ pval, int* __restrict__ pslot) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    float best[4];
    int slot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = MAX ? -INFINITY : INFINITY; slot[i] = -1; }
    extremum_slots<G, MAX>(A, start, end, A.x + c, active, lane, g, best, slot);
    if (g == 0 && active) {
      store_vec<4>(pval + (int64_t)ch * A.d + c, best);
      store_ivec4(pslot + (int64_t)ch * A.d + c, slot);
    }
  }
}

// One wave per long row: its chunks in chunk order (ascending slots) under the strict comparison.
template <bool MAX>
__global__ void __launch_bounds__(256)
extremum_combine_kernel(const ExtArgs A, int n_long, const int* __restrict__ long_row,
                        const int* __restrict__ long_chunk_ptr, const float* __restrict__ pval,
                        const int* __restrict__ pslot) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < A.d; c += kWave * 4) {
      float best[4];
      int slot[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { best[i] = MAX ? -INFINITY : INFINITY; slot[i] = -1; }
      for (int ch = c0; ch < c1; ++ch) {
        float v[4];
        int s[4];
        load_vec<4>(v, pval + (int64_t)ch * A.d + c);
        load_ivec4(s, pslot + (int64_t)ch * A.d + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool take = MAX ? v[i] > best[i] : v[i] < best[i];
          best[i] = take ? v[i] : best[i];
          slot[i] = take ? s[i] : slot[i];
        }
      }
      extremum_store(A, row, c, best, slot);
    }
  }
}

template <int G, bool MAX>
int launch_extremum(const ExtArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  // one row per wave, uncapped grid: rows differ in length and the dispatcher balances fresh blocks (as spmm.hip)
  extremum_kernel<G, MAX><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("extremum_kernel");
  if (sp) {
    float* pval = sp->partial;
    int* pslot = reinterpret_cast<int*>(sp->partial + (size_t)sp->n_chunks * A.d);
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    extremum_chunk_kernel<G, MAX><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end, pval, pslot);
    RGBX_CHECK_LAUNCH("extremum_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    extremum_combine_kernel<MAX><<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->long_row, sp->long_chunk_ptr, pval, pslot);
    RGBX_CHECK_LAUNCH("extremum_combine_kernel");
  }
  return RGBX_OK;
}

template <int G>
int launch_extremum_mode(const ExtArgs& A, int mode, const rgbx_row_split_t* sp, hipStream_t s) {
  return mode == RGBX_EXTREMUM_MAX ? launch_extremum<G, true>(A, sp, s) : launch_extremum<G, false>(A, sp, s);
}

// ---- backward over the transposed CSR ------------------------------------------------------------------------------------

struct ExtBwdArgs {
  const int* rowptr;  // transposed CSR: rows = sources, col = targets
  const int* col;
  const int* t2f;
  const float* gout;
  const int* arg;
  float* gx;
  int64_t ldg, ldgx;
  int N, d;
  int skip_longer;
};

// acc += gout[tgt, c..c+3] where arg[tgt, c..] names this transposed slot's forward slot; groups folded on return.
template <int G>
__device__ __forceinline__ void winner_slots(const ExtBwdArgs& A, int start, int end, int c, bool active, int lane, int g,
                                             float (&acc)[4]) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int mycol = 0, myfwd = -2;
    if (lane < n) {
      mycol = A.col[base + lane];
      myfwd = A.t2f[base + lane];
    }
    for (int k = 0; k < n; k += NG * U) {
      float v[U][4];
      int w[U][4];
      int fs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int tgt = __shfl(mycol, idx & 63);
        fs[u] = __shfl(myfwd, idx & 63);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[u][i] = 0.f; w[u][i] = -1; }
        if (active && idx < n) {
          load_ivec4(w[u], A.arg + (int64_t)tgt * A.d + c);
          load_vec<4>(v[u], A.gout + (int64_t)tgt * A.ldg + c);
        } else {
          fs[u] = -2;  // matches no arg (arg >= -1)
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += w[u][i] == fs[u] ? v[u][i] : 0.f;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
}

template <int G>
__global__ void __launch_bounds__(256) extremum_bwd_kernel(const ExtBwdArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  winner_slots<G>(A, start, end, c, active, lane, g, acc);
  if (g == 0 && active) {
    f4v o = {acc[0], acc[1], acc[2], acc[3]};
    __builtin_nontemporal_store(o, reinterpret_cast<f4v*>(A.gx + (int64_t)row * A.ldgx + c));
  }
}

template <int G>
__global__ void __launch_bounds__(256)
extremum_bwd_chunk_kernel(const ExtBwdArgs A, int n_chunks, const int* __restrict__ chunk_begin,
                          const int* __restrict__ chunk_end, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    winner_slots<G>(A, start, end, c, active, lane, g, acc);
    if (g == 0 && active) store_vec<4>(partial + (int64_t)ch * A.d + c, acc);
  }
}

// One wave per long row: partial sums added in chunk order.
__global__ void __launch_bounds__(256)
extremum_bwd_combine_kernel(const ExtBwdArgs A, int n_long, const int* __restrict__ long_row,
                            const int* __restrict__ long_chunk_ptr, const float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < A.d; c += kWave * 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = c0; ch < c1; ++ch) {
        float p[4];
        load_vec<4>(p, partial + (int64_t)ch * A.d + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += p[i];
      }
      store_vec<4>(A.gx + (int64_t)row * A.ldgx + c, acc);
    }
  }
}

template <int G>
int launch_extremum_bwd(const ExtBwdArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  extremum_bwd_kernel<G><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("extremum_bwd_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    extremum_bwd_chunk_kernel<G><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end, sp->partial);
    RGBX_CHECK_LAUNCH("extremum_bwd_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    extremum_bwd_combine_kernel<<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->long_row, sp->long_chunk_ptr, sp->partial);
    RGBX_CHECK_LAUNCH("extremum_bwd_combine_kernel");
  }
  return RGBX_OK;
}

const rgbx_row_split_t* usable_split(const rgbx_row_split_t* split) {
  return (split && split->threshold > 0 && split->n_chunks > 0) ? split : nullptr;
}

bool complete_split(const rgbx_row_split_t* sp) {
  return sp->n_long > 0 && sp->chunk_begin && sp->chunk_end && sp->long_row && sp->long_chunk_ptr && sp->partial &&
         aligned16(sp->partial);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_spmm_csr_extremum_supported(int64_t d) { return d >= 4 && d % 4 == 0 && d <= 256; }

extern "C" int rgbx_spmm_csr_extremum_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, float* out,
                                          int64_t ldo, int32_t* arg, int64_t N, int64_t d, int mode,
                                          const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "spmm_extremum: negative size");
  if (!rowptr || !col || !x || !out) return fail(RGBX_E_ARG, "spmm_extremum: null pointer");
  if (mode != RGBX_EXTREMUM_MAX && mode != RGBX_EXTREMUM_MIN)
    return fail(RGBX_E_ARG, "spmm_extremum: mode must be RGBX_EXTREMUM_MAX or RGBX_EXTREMUM_MIN (got %d)", mode);
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "spmm_extremum: N exceeds int32");
  if (!rgbx_spmm_csr_extremum_supported(d))
    return fail(RGBX_E_SHAPE, "spmm_extremum: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld); pad or cut the rows", (long long)d);
  if (ldx < d || ldo < d) return fail(RGBX_E_ARG, "spmm_extremum: leading dimension < d");
  if (out == x) return fail(RGBX_E_ARG, "spmm_extremum: out must not alias x");
  if (!aligned16(x) || !aligned16(out) || ldx % 4 || ldo % 4 || (arg && !aligned16(arg)))
    return fail(RGBX_E_ALIGN, "spmm_extremum: x / out / arg must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "spmm_extremum: incomplete row-split plan");
  ExtArgs A{rowptr, col, x, out, arg, ldx, ldo, (int)N, (int)d, sp ? sp->threshold : 0};
  hipStream_t s = (hipStream_t)stream;
  const int lanes = (int)(d / 4);
  if (lanes <= 1) return launch_extremum_mode<1>(A, mode, sp, s);
  if (lanes <= 2) return launch_extremum_mode<2>(A, mode, sp, s);
  if (lanes <= 4) return launch_extremum_mode<4>(A, mode, sp, s);
  if (lanes <= 8) return launch_extremum_mode<8>(A, mode, sp, s);
  if (lanes <= 16) return launch_extremum_mode<16>(A, mode, sp, s);
  if (lanes <= 32) return launch_extremum_mode<32>(A, mode, sp, s);
  return launch_extremum_mode<64>(A, mode, sp, s);
}

extern "C" int rgbx_extremum_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* gout,
                                     int64_t ldg, const int32_t* arg, float* gx, int64_t ldgx, int64_t N, int64_t d,
                                     const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "extremum_bwd: negative size");
  if (!rowptr_t || !col_t || !t2f || !gout || !arg || !gx) return fail(RGBX_E_ARG, "extremum_bwd: null pointer");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "extremum_bwd: N exceeds int32");
  if (!rgbx_spmm_csr_extremum_supported(d))
    return fail(RGBX_E_SHAPE, "extremum_bwd: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld); pad or cut the rows", (long long)d);
  if (ldg < d || ldgx < d) return fail(RGBX_E_ARG, "extremum_bwd: leading dimension < d");
  if (gx == gout) return fail(RGBX_E_ARG, "extremum_bwd: gx must not alias gout");
  if (!aligned16(gout) || !aligned16(gx) || !aligned16(arg) || ldg % 4 || ldgx % 4)
    return fail(RGBX_E_ALIGN, "extremum_bwd: gout / arg / gx must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "extremum_bwd: incomplete row-split plan");
  ExtBwdArgs A{rowptr_t, col_t, t2f, gout, arg, gx, ldg, ldgx, (int)N, (int)d, sp ? sp->threshold : 0};
  hipStream_t s = (hipStream_t)stream;
  const int lanes = (int)(d / 4);
  if (lanes <= 1) return launch_extremum_bwd<1>(A, sp, s);
  if (lanes <= 2) return launch_extremum_bwd<2>(A, sp, s);
  if (lanes <= 4) return launch_extremum_bwd<4>(A, sp, s);
  if (lanes <= 8) return launch_extremum_bwd<8>(A, sp, s);
  if (lanes <= 16) return launch_extremum_bwd<16>(A, sp, s);
  if (lanes <= 32) return launch_extremum_bwd<32>(A, sp, s);
  return launch_extremum_bwd<64>(A, sp, s);
}
