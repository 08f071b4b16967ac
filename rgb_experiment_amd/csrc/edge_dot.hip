// Per-slot dot product over a CSR for gfx950: g[p] = <a[i,:], b[col[p],:]> for every slot p of row i.
// This is dL/dw of out = sum_p w[p] * x[col[p],:] (message norm * x_j, reference models/dagnn.py:57-59, with the
// norm of models/dagnn.py:12-31 taken as a variable): a = dL/dout, b = x. It serves learnable edge weights.
//
// Same access pattern as the row gather of spmm.hip, and the same lane layout: one wave owns one row, the wave is
// split into NG = 64/G groups of G lanes, a group reads ONE neighbour row per step with 16-byte loads, U steps are
// issued back to back (NG * U neighbour rows in flight), and the 64 column indices of a row chunk are read once,
// coalesced, and handed to the groups with ds_bpermute. Where the gather ACCUMULATES the neighbour rows, this kernel
// multiplies each with the lane's fragment of a[i,:] (held in registers for the whole row), folds the G partial
// products with shuffles, and hands slot k's dot to lane k: a chunk of 64 slots leaves as ONE coalesced 256-byte store.
// No atomics; every g[p] is one fixed-order sum, so two runs give the same bits.
//
// Degree skew: with a row-split plan (rgbx_row_split_t) the row kernel skips rows longer than the threshold and a
// second launch gives every chunk of such a row its own wave (chunk_row names the row). Slots are independent, so
// there are no partials to combine.
#include "rgbx_common.h"

namespace rgbx {
namespace {

struct EdgeDotArgs {
  const int* rowptr;
  const int* col;
  const float* a;
  const float* b;
  float* g;
  int64_t lda, ldb;
  int N, d;
  int skip_longer;
};

// Slots [start, end) of `row`: afrag = this lane's 4 floats of a[row,:] (zero beyond d).
template <int G>
__device__ __forceinline__ void dot_slots(const EdgeDotArgs& A, int start, int end, const float (&afrag)[4],
                                          const float* bc, bool active, int lane, int g) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int mycol = lane < n ? A.col[base + lane] : 0;
    float mine = 0.f;
    for (int k = 0; k < n; k += NG * U) {
      float v[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int src = __shfl(mycol, idx & 63);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[u][i] = 0.f;
        if (active && idx < n) load_vec<4>(v[u], bc + (int64_t)src * A.ldb);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float r = afrag[0] * v[u][0];
        r = fmaf(afrag[1], v[u][1], r);
        r = fmaf(afrag[2], v[u][2], r);
        r = fmaf(afrag[3], v[u][3], r);
#pragma unroll
        for (int off = G >> 1; off >= 1; off >>= 1) r += __shfl_xor(r, off);
        // every lane of group g now holds the dot of slot k + u * NG + g; lane (k + u * NG + j) takes group j's
        const int first = k + u * NG;
        const float got = __shfl(r, ((lane - first) & (NG - 1)) * G);
        if (lane >= first && lane < first + NG) mine = got;
      }
    }
    if (lane < n) A.g[base + lane] = mine;
  }
}

template <int G>
__device__ __forceinline__ void load_afrag(const EdgeDotArgs& A, int row, int c, bool active, float (&afrag)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) afrag[i] = 0.f;
  if (active) load_vec<4>(afrag, A.a + (int64_t)row * A.lda + c);
}

template <int G>
__global__ void __launch_bounds__(256) edge_dot_kernel(const EdgeDotArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (end <= start || (A.skip_longer > 0 && end - start > A.skip_longer)) return;  // the chunk kernel owns long rows
  float afrag[4];
  load_afrag<G>(A, row, c, active, afrag);
  dot_slots<G>(A, start, end, afrag, A.b + c, active, lane, g);
}

template <int G>
__global__ void __launch_bounds__(256)
edge_dot_chunk_kernel(const EdgeDotArgs A, int n_chunks, const int* __restrict__ chunk_begin,
                      const int* __restrict__ chunk_end, const int* __restrict__ chunk_row) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    const int row = __builtin_amdgcn_readfirstlane(chunk_row[ch]);
    float afrag[4];
    load_afrag<G>(A, row, c, active, afrag);
    dot_slots<G>(A, start, end, afrag, A.b + c, active, lane, g);
  }
}

template <int G>
int launch_edge_dot(const EdgeDotArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  // one row per wave, uncapped grid: rows differ in length and the dispatcher balances fresh blocks (as spmm.hip)
  edge_dot_kernel<G><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("edge_dot_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    edge_dot_chunk_kernel<G><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end, sp->chunk_row);
    RGBX_CHECK_LAUNCH("edge_dot_chunk_kernel");
  }
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_edge_dot_supported(int64_t d) { return d >= 4 && d % 4 == 0 && d <= 256; }

extern "C" int rgbx_edge_dot_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda,
                                 const float* b, int64_t ldb, float* g, int64_t N, int64_t d,
                                 const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "edge_dot: negative size");
  if (!rowptr || !col || !a || !b || !g) return fail(RGBX_E_ARG, "edge_dot: null pointer");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "edge_dot: N exceeds int32");
  if (!rgbx_edge_dot_supported(d))
    return fail(RGBX_E_SHAPE, "edge_dot: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld); pad or cut the rows", (long long)d);
  if (lda < d || ldb < d) return fail(RGBX_E_ARG, "edge_dot: leading dimension < d");
  if (!aligned16(a) || !aligned16(b) || lda % 4 || ldb % 4)
    return fail(RGBX_E_ALIGN, "edge_dot: a / b must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = (split && split->threshold > 0 && split->n_chunks > 0) ? split : nullptr;
  if (sp && (!sp->chunk_begin || !sp->chunk_end || !sp->chunk_row))
    return fail(RGBX_E_ARG, "edge_dot: incomplete row-split plan");
  EdgeDotArgs A{rowptr, col, a, b, g, lda, ldb, (int)N, (int)d, sp ? sp->threshold : 0};
  hipStream_t s = (hipStream_t)stream;
  const int lanes = (int)(d / 4);
  if (lanes <= 1) return launch_edge_dot<1>(A, sp, s);
  if (lanes <= 2) return launch_edge_dot<2>(A, sp, s);
  if (lanes <= 4) return launch_edge_dot<4>(A, sp, s);
  if (lanes <= 8) return launch_edge_dot<8>(A, sp, s);
  if (lanes <= 16) return launch_edge_dot<16>(A, sp, s);
  if (lanes <= 32) return launch_edge_dot<32>(A, sp, s);
  return launch_edge_dot<64>(A, sp, s);
}
