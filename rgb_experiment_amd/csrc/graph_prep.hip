// Graph preparation: int64 edge list -> CSR grouped by aggregation index (stable), degree
// normalisation. Replaces the per-call index bookkeeping of PyG's propagate / gcn_norm
// (reference models/dagnn.py:12-31; call sites models/gcn.py:27, graphsage.py:53-58, gat.py:28,
// appnp_stack.py:29). Runs once per edge_index; all outputs live in caller-owned buffers.
#include "rgbx_common.h"

#include <rocprim/rocprim.hpp>

namespace rgbx {

char* err_buf() {
  static thread_local char buf[256] = "";
  return buf;
}

namespace {

// Slot e < E is input edge e; slot E + i is the self-loop added for node i (loops_mode != 0).
// A removed self-loop gets key N, which sorts behind every real row and is cut off by
// rowptr[N].
__global__ void __launch_bounds__(256)
fill_keys_kernel(const int64_t* __restrict__ agg_row, const int64_t* __restrict__ other_row,
                 int64_t E, int64_t M, int N, int loops_mode, int* __restrict__ keys,
                 int* __restrict__ ids) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M;
       e += (int64_t)gridDim.x * blockDim.x) {
    int key;
    if (e < E) {
      const int64_t t = agg_row[e];
      key = (loops_mode != RGBX_LOOPS_KEEP && other_row[e] == t) ? N : (int)t;
    } else {
      key = (int)(e - E);
    }
    keys[e] = key;
    ids[e] = (int)e;
  }
}

// After the sort: gather index per slot, and rowptr from the key boundaries. Slot p opens every
// row in (key[p-1], key[p]]; the last slot also closes the rows behind its key.
__global__ void __launch_bounds__(256)
finish_csr_kernel(const int* __restrict__ keys, const int* __restrict__ perm,
                  const int64_t* __restrict__ other_row, int64_t E, int64_t M, int N,
                  int* __restrict__ col, int* __restrict__ rowptr) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < M;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int key = keys[p];
    const int id = perm[p];
    col[p] = id < E ? (int)other_row[id] : (int)(id - E);
    const int prev = p > 0 ? keys[p - 1] : -1;
    for (int r = prev + 1; r <= key; ++r) rowptr[r] = (int)p;
    if (p == M - 1)
      for (int r = key + 1; r <= N; ++r) rowptr[r] = (int)M;
  }
}

__global__ void __launch_bounds__(256) zero_rowptr_kernel(int* rowptr, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    rowptr[i] = 0;
}

__global__ void __launch_bounds__(256)
deg_inv_sqrt_kernel(const int* __restrict__ rowptr, int N, float* __restrict__ dis) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int cnt = rowptr[i + 1] - rowptr[i];
    dis[i] = cnt > 0 ? 1.0f / sqrtf((float)cnt) : 0.0f;  // inf -> 0, dagnn.py:29-30
  }
}

__global__ void __launch_bounds__(256)
inv_degree_kernel(const int* __restrict__ rowptr, int N, float* __restrict__ inv) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int cnt = rowptr[i + 1] - rowptr[i];
    inv[i] = 1.0f / (float)(cnt > 1 ? cnt : 1);
  }
}

// One wave per row, lanes over its slots: w = (dis[src] * 1) * dis[tgt] as dagnn.py:31.
__global__ void __launch_bounds__(256)
gcn_norm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int N,
                const float* __restrict__ dis, float* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int s = rowptr[row], e = rowptr[row + 1];
    const float di = dis[row];
    for (int p = s + lane; p < e; p += 64) w[p] = dis[col[p]] * di;
  }
}

// ---- weighted graphs: gcn_norm(edge_index, edge_weight) of models/dagnn.py:12-31 with the weight present ----------

__global__ void __launch_bounds__(256) fill_i32_kernel(int* __restrict__ v, int64_t n, int value) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = value;
}

// The input self-loop that supplies node i's loop weight: the one with the HIGHEST edge id (the CPU assignment
// loop_w[row[~keep]] = edge_weight[~keep] of add_remaining_self_loops leaves the last one standing). An integer max
// has one answer whatever the order of the threads.
__global__ void __launch_bounds__(256)
loop_source_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t E,
                   int* __restrict__ loop_src) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = dst[e];
    if (src[e] == t) atomicMax(loop_src + t, (int)e);
  }
}

__global__ void __launch_bounds__(256)
loop_weight_kernel(const int* __restrict__ loop_src, const float* __restrict__ ew, int N, float fill,
                   float* __restrict__ loop_w) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int e = loop_src[i];
    loop_w[i] = e >= 0 ? ew[e] : fill;
  }
}

__global__ void __launch_bounds__(256)
slot_weight_kernel(const int* __restrict__ perm, int64_t nnz, const float* __restrict__ ew, int64_t E,
                   const float* __restrict__ loop_w, float* __restrict__ ew_slot) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
    const int id = perm[p];
    ew_slot[p] = id < E ? ew[id] : loop_w[id - E];
  }
}

// Fixed-order sum of v over the wave: lane l adds its strided elements in slot order, then a butterfly.
__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One wave per row (any length: a hub row is one long strided loop, this runs once per graph):
// deg = sum of the row's slot weights, dis = deg^-1/2 with inf -> 0 (dagnn.py:25-30). Not clamped: a negative sum gives NaN.
__global__ void __launch_bounds__(256)
weighted_deg_inv_sqrt_kernel(const int* __restrict__ rowptr, const float* __restrict__ ew_slot, int N,
                             float* __restrict__ dis) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int s = rowptr[row], e = rowptr[row + 1];
    float acc = 0.f;
    for (int p = s + lane; p < e; p += 64) acc += ew_slot[p];
    const float deg = wave_sum_fixed(acc);
    if (lane == 0) dis[row] = deg == 0.f ? 0.f : 1.0f / sqrtf(deg);
  }
}

// w = (dis[src] * ew) * dis[tgt], dagnn.py:31.
__global__ void __launch_bounds__(256)
gcn_norm_weighted_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                         const float* __restrict__ ew_slot, int N, const float* __restrict__ dis,
                         float* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int s = rowptr[row], e = rowptr[row + 1];
    const float di = dis[row];
    for (int p = s + lane; p < e; p += 64) w[p] = dis[col[p]] * ew_slot[p] * di;
  }
}

// Backward of the normalisation, first half: with w_p = dis[j] ew_p dis[i] and g = dL/dw,
//   ddis[k] = sum_{p: tgt = k} g_p ew_p dis[src_p] + sum_{p: src = k} g_p ew_p dis[tgt_p]
// (first sum over the forward row k, second over the transposed row k, whose slots name their forward slot in t2f),
//   ddeg[k] = -1/2 deg[k]^-3/2 ddis[k] = -1/2 dis[k]^3 ddis[k]   (dis = 0 where inf was masked: no gradient there).
// One wave per row, both sums in a fixed order.
__global__ void __launch_bounds__(256)
gcn_norm_bwd_deg_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                        const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                        const int* __restrict__ t2f, const float* __restrict__ g,
                        const float* __restrict__ ew_slot, const float* __restrict__ dis, int N,
                        float* __restrict__ ddeg) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    float acc = 0.f;
    for (int p = rowptr[row] + lane; p < rowptr[row + 1]; p += 64) acc = fmaf(g[p] * ew_slot[p], dis[col[p]], acc);
    float acc_t = 0.f;
    for (int q = rowptr_t[row] + lane; q < rowptr_t[row + 1]; q += 64) {
      const int p = t2f[q];
      acc_t = fmaf(g[p] * ew_slot[p], dis[col_t[q]], acc_t);
    }
    const float ddis = wave_sum_fixed(acc) + wave_sum_fixed(acc_t);
    const float di = dis[row];
    if (lane == 0) ddeg[row] = -0.5f * di * di * di * ddis;
  }
}

// Second half: dL/dew of slot p of row i = g_p dis[j] dis[i] + ddeg[i] (deg[i] sums the row's slot weights), sent to the
// input edge behind the slot: perm[p] < E is that edge; an added loop E + i goes to the input self-loop that supplied its
// weight (loop_src[i]), or nowhere when the loop was filled in. Every edge is written at most once (dew is zeroed first:
// removed self-loops that lost, or were dropped, take no part in the output).
__global__ void __launch_bounds__(256)
gcn_norm_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                         const int* __restrict__ perm, const int* __restrict__ loop_src,
                         const float* __restrict__ g, const float* __restrict__ dis,
                         const float* __restrict__ ddeg, int N, int64_t E, float* __restrict__ dew) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < N; row += gridDim.x * wpb) {
    const int s = rowptr[row], e = rowptr[row + 1];
    const float di = dis[row], dd = ddeg[row];
    for (int p = s + lane; p < e; p += 64) {
      int id = perm[p];
      if (id >= E) id = loop_src ? loop_src[id - E] : -1;
      if (id >= 0) dew[id] = fmaf(g[p] * dis[col[p]], di, dd);
    }
  }
}

int sort_bits(int64_t N) {
  int b = 1;
  while (((int64_t)1 << b) <= N) ++b;  // keys lie in [0, N]
  return b;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int grid_for(int64_t n, int per_block = 256) {
  int64_t g = cdiv(n > 0 ? n : 1, per_block);
  return (int)(g < kMaxGrid ? g : kMaxGrid);
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_version(void) { return RGBX_VERSION; }

extern "C" const char* rgbx_last_error_string(void) { return err_buf(); }

extern "C" int rgbx_csr_workspace_bytes(int64_t E, int64_t N, size_t* bytes) {
  if (!bytes || E < 0 || N < 0) return fail(RGBX_E_ARG, "csr_workspace_bytes: bad argument");
  const int64_t M = E + N;
  if (M >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "E+N=%lld exceeds int32", (long long)M);
  size_t tmp = 0;
  int* nul = nullptr;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp, nul, nul, nul, nul, (size_t)(M > 0 ? M : 1),
                                           0, sort_bits(N), (hipStream_t) nullptr);
  if (e != hipSuccess) return hip_fail(e, "radix_sort_pairs(size query)");
  *bytes = 3 * align256((size_t)(M > 0 ? M : 1) * sizeof(int)) + align256(tmp);
  return RGBX_OK;
}

extern "C" int rgbx_csr_build(const int64_t* agg_row, const int64_t* other_row, int64_t E, int64_t N,
                              int loops_mode, int32_t* rowptr, int32_t* col, int32_t* perm,
                              void* workspace, size_t workspace_bytes, rgbx_stream_t stream) {
  if (E < 0 || N < 0 || !rowptr || (E > 0 && (!agg_row || !other_row)))
    return fail(RGBX_E_ARG, "csr_build: null pointer or negative size");
  if (loops_mode < RGBX_LOOPS_KEEP || loops_mode > RGBX_LOOPS_REMOVE_ADD)
    return fail(RGBX_E_ARG, "csr_build: loops_mode %d", loops_mode);
  size_t need = 0;
  if (int rc = rgbx_csr_workspace_bytes(E, N, &need)) return rc;
  const int64_t M = loops_mode == RGBX_LOOPS_KEEP ? E : E + N;
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {
    zero_rowptr_kernel<<<grid_for(N + 1), 256, 0, s>>>(rowptr, N + 1);
    RGBX_CHECK_LAUNCH("zero_rowptr_kernel");
    return RGBX_OK;
  }
  if (!col || !perm || !workspace) return fail(RGBX_E_ARG, "csr_build: null output/workspace");
  if (workspace_bytes < need)
    return fail(RGBX_E_WS, "csr_build: workspace %zu < %zu bytes", workspace_bytes, need);

  const size_t slab = align256((size_t)(E + N > 0 ? E + N : 1) * sizeof(int));
  char* ws = static_cast<char*>(workspace);
  int* keys_in = reinterpret_cast<int*>(ws);
  int* keys_out = reinterpret_cast<int*>(ws + slab);
  int* ids_in = reinterpret_cast<int*>(ws + 2 * slab);
  void* sort_tmp = ws + 3 * slab;
  size_t sort_bytes = workspace_bytes - 3 * slab;

  fill_keys_kernel<<<grid_for(M), 256, 0, s>>>(agg_row, other_row, E, M, (int)N, loops_mode,
                                               keys_in, ids_in);
  RGBX_CHECK_LAUNCH("fill_keys_kernel");
  // LSD radix sort is stable: slots of one row keep the rewritten list's order.
  RGBX_HIP(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys_in, keys_out, ids_in, perm,
                                     (size_t)M, 0, sort_bits(N), s));
  finish_csr_kernel<<<grid_for(M), 256, 0, s>>>(keys_out, perm, other_row, E, M, (int)N, col,
                                                rowptr);
  RGBX_CHECK_LAUNCH("finish_csr_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_deg_inv_sqrt_f32(const int32_t* rowptr, int64_t N, float* dis,
                                     rgbx_stream_t stream) {
  if (N < 0 || !rowptr || (N > 0 && !dis)) return fail(RGBX_E_ARG, "deg_inv_sqrt: bad argument");
  if (N == 0) return RGBX_OK;
  deg_inv_sqrt_kernel<<<grid_for(N), 256, 0, (hipStream_t)stream>>>(rowptr, (int)N, dis);
  RGBX_CHECK_LAUNCH("deg_inv_sqrt_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_inv_degree_f32(const int32_t* rowptr, int64_t N, float* inv,
                                   rgbx_stream_t stream) {
  if (N < 0 || !rowptr || (N > 0 && !inv)) return fail(RGBX_E_ARG, "inv_degree: bad argument");
  if (N == 0) return RGBX_OK;
  inv_degree_kernel<<<grid_for(N), 256, 0, (hipStream_t)stream>>>(rowptr, (int)N, inv);
  RGBX_CHECK_LAUNCH("inv_degree_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gcn_norm_f32(const int32_t* rowptr, const int32_t* col, int64_t N,
                                 const float* dis, float* w, rgbx_stream_t stream) {
  if (N < 0 || !rowptr || !col || !dis || !w) return fail(RGBX_E_ARG, "gcn_norm: bad argument");
  if (N == 0) return RGBX_OK;
  gcn_norm_kernel<<<grid_for(N, 4), 256, 0, (hipStream_t)stream>>>(rowptr, col, (int)N, dis, w);
  RGBX_CHECK_LAUNCH("gcn_norm_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_loop_weights_f32(const int64_t* src, const int64_t* dst, const float* ew, int64_t E,
                                     int64_t N, int loops_mode, float fill, float* loop_w,
                                     int32_t* loop_src, rgbx_stream_t stream) {
  if (E < 0 || N < 0 || (E > 0 && (!src || !dst || !ew)) || (N > 0 && (!loop_w || !loop_src)))
    return fail(RGBX_E_ARG, "loop_weights: null pointer or negative size");
  if (loops_mode != RGBX_LOOPS_ADD_REMAINING && loops_mode != RGBX_LOOPS_REMOVE_ADD)
    return fail(RGBX_E_ARG, "loop_weights: loops_mode %d adds no loops", loops_mode);
  if (E >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "loop_weights: E or N exceeds int32");
  if (N == 0) return RGBX_OK;
  hipStream_t s = (hipStream_t)stream;
  fill_i32_kernel<<<grid_for(N), 256, 0, s>>>(loop_src, N, -1);
  RGBX_CHECK_LAUNCH("fill_i32_kernel");
  if (loops_mode == RGBX_LOOPS_ADD_REMAINING && E > 0) {
    loop_source_kernel<<<grid_for(E), 256, 0, s>>>(src, dst, E, loop_src);
    RGBX_CHECK_LAUNCH("loop_source_kernel");
  }
  loop_weight_kernel<<<grid_for(N), 256, 0, s>>>(loop_src, ew, (int)N, fill, loop_w);
  RGBX_CHECK_LAUNCH("loop_weight_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_edge_slot_weights_f32(const int32_t* perm, int64_t nnz, const float* ew, int64_t E,
                                          const float* loop_w, float* ew_slot, rgbx_stream_t stream) {
  if (nnz < 0 || E < 0 || (nnz > 0 && (!perm || !ew_slot)) || (E > 0 && !ew))
    return fail(RGBX_E_ARG, "edge_slot_weights: null pointer or negative size");
  if (nnz > E && !loop_w) return fail(RGBX_E_ARG, "edge_slot_weights: nnz > E needs loop weights");
  if (nnz == 0) return RGBX_OK;
  slot_weight_kernel<<<grid_for(nnz), 256, 0, (hipStream_t)stream>>>(perm, nnz, ew, E, loop_w, ew_slot);
  RGBX_CHECK_LAUNCH("slot_weight_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_weighted_deg_inv_sqrt_f32(const int32_t* rowptr, const float* ew_slot, int64_t N, float* dis,
                                              rgbx_stream_t stream) {
  if (N < 0 || !rowptr || !ew_slot || (N > 0 && !dis)) return fail(RGBX_E_ARG, "weighted_deg_inv_sqrt: bad argument");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "weighted_deg_inv_sqrt: N exceeds int32");
  if (N == 0) return RGBX_OK;
  weighted_deg_inv_sqrt_kernel<<<grid_for(N, 4), 256, 0, (hipStream_t)stream>>>(rowptr, ew_slot, (int)N, dis);
  RGBX_CHECK_LAUNCH("weighted_deg_inv_sqrt_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gcn_norm_weighted_f32(const int32_t* rowptr, const int32_t* col, const float* ew_slot,
                                          int64_t N, const float* dis, float* w, rgbx_stream_t stream) {
  if (N < 0 || !rowptr || !col || !ew_slot || !dis || !w) return fail(RGBX_E_ARG, "gcn_norm_weighted: bad argument");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "gcn_norm_weighted: N exceeds int32");
  if (N == 0) return RGBX_OK;
  gcn_norm_weighted_kernel<<<grid_for(N, 4), 256, 0, (hipStream_t)stream>>>(rowptr, col, ew_slot, (int)N, dis, w);
  RGBX_CHECK_LAUNCH("gcn_norm_weighted_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gcn_norm_bwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                     const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                     const int32_t* loop_src, const float* g, const float* ew_slot,
                                     const float* dis, int64_t N, int64_t E, float* ddeg, float* dew,
                                     rgbx_stream_t stream) {
  if (N < 0 || E < 0) return fail(RGBX_E_ARG, "gcn_norm_bwd: negative size");
  if (!rowptr || !col || !perm || !rowptr_t || !col_t || !t2f || !g || !ew_slot || !dis || !ddeg || (E > 0 && !dew))
    return fail(RGBX_E_ARG, "gcn_norm_bwd: null pointer");
  if (N >= INT32_MAX || E >= INT32_MAX) return fail(RGBX_E_RANGE, "gcn_norm_bwd: N or E exceeds int32");
  hipStream_t s = (hipStream_t)stream;
  if (E > 0) RGBX_HIP(hipMemsetAsync(dew, 0, sizeof(float) * (size_t)E, s));
  if (N == 0) return RGBX_OK;
  gcn_norm_bwd_deg_kernel<<<grid_for(N, 4), 256, 0, s>>>(rowptr, col, rowptr_t, col_t, t2f, g, ew_slot, dis, (int)N, ddeg);
  RGBX_CHECK_LAUNCH("gcn_norm_bwd_deg_kernel");
  gcn_norm_bwd_edge_kernel<<<grid_for(N, 4), 256, 0, s>>>(rowptr, col, perm, loop_src, g, dis, ddeg, (int)N, E, dew);
  RGBX_CHECK_LAUNCH("gcn_norm_bwd_edge_kernel");
  return RGBX_OK;
}
