// Tall-skinny fp32 GEMM on the MFMA units: C[M,N] = A^T B with A [K,M], B [K,N] row-major and
// K (= number of nodes) in the millions, M, N (= feature widths) in the hundreds. This is the weight
// gradient dW = dY^T X of every dense layer on the path (reference: the nn.Linear / GCNConv.lin /
// GATConv.lin_src inside models/gcn.py:18-21, graphsage.py:46-47, gat.py:18-21, appnp_stack.py:19-20,
// differentiated by loss.backward(), itexperiments.py:439). A generic GEMM library tiles M x N only,
// which leaves 16 workgroups for a 128 x 128 output; here K is split across the whole chip.
//
// Kernel 1: grid (S, ceil(M/128), ceil(N/128)); a workgroup (4 waves) owns one 128x128 output tile over
// one K-slab, stages [32 x 128] tiles of A and B through LDS with 16-byte loads, and every wave
// accumulates a 64x64 quadrant with v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain). Both operands are
// read along their contiguous dimension: lane l of a fragment holds row k0 + (l >> 5), column
// c0 + (l & 31) — no transposes anywhere. Partial tiles go to a workspace with plain stores.
// Kernel 2: sums the S partials in slab order (bitwise reproducible, no float atomics).
// Optionally the column sums of A (= the bias gradient when A = dY) are taken from the staged A tiles by the
// workgroups of the first N-tile and reduced the same way: dY is then read once for dW and db together.
//
// Round 5 — the reference's default shapes (initial_params.py:25-29: F = 1433 -> hidden 64 -> C = 7), where dW1 = dH^T X
// is [64, 1433] over K = |V| rows and was 16.9 of the 42 ms epoch at |V| = 2 M:
//  (1) the 16-byte path no longer needs M % 4 == 0 / N % 4 == 0, only 16-byte aligned ROWS (lda % 4 == 0, ldb % 4 == 0):
//      a row's last float4 may reach into its padding (columns [N, ld)), whose products land in output columns that are
//      never stored. A feature matrix with F = 1433 is kept with a row stride of 1436 floats (ops.align_rows);
//  (2) M <= 64 runs a 64 x 128 tile (one 32-row MFMA block per wave instead of two): half the MFMAs and half the A-side
//      LDS traffic of the 128 x 128 tile, which multiplied 64 rows of zeros.
//
// Two forms of the A operand on the 16-byte path, same slabs, tile loop, MFMA order and reduce launches (so every sum
// keeps its order and the results are those of the plain kernel on the materialised operand, bit for bit):
//  - A_BN (rgbx_gemm_tn_bn_bwd_f32): A = BatchNorm's input gradient, formed from (G, X) and the per-column constants
//    between fetch_tile and put_tile (bn_bwd_input_grad, the expression of bn_bwd_apply_kernel) — the [K, M] matrix gx
//    is never written or read back. The constants sit in LDS (5 x MT floats): held in registers they would cost the
//    third workgroup per CU;
//  - A_ROWS (rgbx_gemm_tn_rows_f32): only the rows of an ascending list are multiplied, for operands whose other rows
//    are all zero (the loss gradient outside the rows the loss selects). Slab s takes the list entries inside its own
//    row range [s * slab, (s + 1) * slab), in list order: the non-zero products meet the accumulators in the order of
//    the full product, a skipped row only added zeros. The list entries of a tile are fetched one tile ahead of its rows
//    (10 more VGPRs; the workgroups per CU stay 3, and 4 for the 64-row tile).
#include "rgbx_common.h"

namespace rgbx {
namespace {

constexpr int BM = 128, BN = 128, KT = 32;
enum { A_PLAIN = 0, A_BN = 1, A_ROWS = 2 };

// What the A_BN / A_ROWS forms read beside A and B (unused, all zero, in the plain form)
struct TnExtra {
  const float* X;        // A_BN: BatchNorm's input, beside A = the gradient of its output
  int64_t ldx;
  const float *mean, *rstd, *ca, *cb, *ck;
  const int32_t* rows;   // A_ROWS: ascending row list
  int64_t n_rows;
};
using f32x16 = __attribute__((ext_vector_type(16))) float;

// Scalar staging (rows that are not 16-byte aligned): [KT x W] tile, row-major in LDS; rows >= k_end and columns >= ncols
// are zero-filled
template <int W>
__device__ __forceinline__ void stage_tile(float* __restrict__ lds, const float* __restrict__ src,
                                           int64_t ld, int64_t k0, int64_t k_end, int c0, int ncols) {
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int p = 0; p < KT * W / 256; ++p) {
    const int idx = p * 256 + tid;
    const int r = idx / W, c = idx % W;
    const int64_t k = k0 + r;
    lds[r * W + c] = (k < k_end && c0 + c < ncols) ? src[k * ld + c0 + c] : 0.f;
  }
}

// Register-staged variant (16-byte path): fetch_tile issues the global loads of one [KT x W] tile
// into registers, put_tile writes them to LDS. Splitting the two lets the loads of tile i+1 fly while the MFMAs
// of tile i run (the plain loop waits for HBM once per 32 rows of K with nothing else to do).
// W = tile width in floats (128, or 64 for the A side of the 64-row output tile); W / 4 float4 per tile row
template <int W>
__device__ __forceinline__ void fetch_tile(float4 (&regs)[KT * (W / 4) / 256], const float* __restrict__ src, int64_t ld,
                                           int64_t k0, int64_t k_end, int c0, int ncols) {
#pragma unroll
  for (int p = 0; p < KT * (W / 4) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int r = idx / (W / 4), c = (idx % (W / 4)) * 4;
    const int64_t k = k0 + r;
    regs[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    // c0 + c < ncols <= ld: the float4 may end in the row's padding (columns [ncols, ld)), never beyond the row
    if (k < k_end && c0 + c < ncols) regs[p] = *reinterpret_cast<const float4*>(src + k * ld + c0 + c);
  }
}

template <int W>
__device__ __forceinline__ void put_tile(float* __restrict__ lds, const float4 (&regs)[KT * (W / 4) / 256]) {
#pragma unroll
  for (int p = 0; p < KT * (W / 4) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int r = idx / (W / 4), c = (idx % (W / 4)) * 4;
    *reinterpret_cast<float4*>(lds + r * W + c) = regs[p];
  }
}

// A_BN: the staged A tile is bn_bwd_input_grad(G, X, ...) of the two fetched tiles. Rows >= k_end and columns >= ncols
// stay the zeros fetch_tile put there: they are not mapped. `lc` = [5][W] constants of columns c0 .. c0 + W (mean, rstd,
// ca, cb, ck; zero past ncols)
template <int W>
__device__ __forceinline__ void put_tile_bn(float* __restrict__ lds, const float4 (&rg)[KT * (W / 4) / 256],
                                            const float4 (&rx)[KT * (W / 4) / 256], const float* __restrict__ lc,
                                            int64_t k0, int64_t k_end, int c0, int ncols) {
#pragma unroll
  for (int p = 0; p < KT * (W / 4) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int r = idx / (W / 4), c = (idx % (W / 4)) * 4;
    float4 v = rg[p];
    if (k0 + r < k_end && c0 + c < ncols) {
      const float4 mu = *reinterpret_cast<const float4*>(lc + 0 * W + c);
      const float4 rs = *reinterpret_cast<const float4*>(lc + 1 * W + c);
      const float4 a = *reinterpret_cast<const float4*>(lc + 2 * W + c);
      const float4 b = *reinterpret_cast<const float4*>(lc + 3 * W + c);
      const float4 k = *reinterpret_cast<const float4*>(lc + 4 * W + c);
      v.x = bn_bwd_input_grad(v.x, rx[p].x, mu.x, rs.x, a.x, b.x, k.x);
      v.y = bn_bwd_input_grad(v.y, rx[p].y, mu.y, rs.y, a.y, b.y, k.y);
      v.z = bn_bwd_input_grad(v.z, rx[p].z, mu.z, rs.z, a.z, b.z, k.z);
      v.w = bn_bwd_input_grad(v.w, rx[p].w, mu.w, rs.w, a.w, b.w, k.w);
    }
    *reinterpret_cast<float4*>(lds + r * W + c) = v;
  }
}

// A_ROWS: tile row r is row rows[j0 + r] of src; list entries >= j_end are zero-filled. A tile is reached through two
// dependent loads (list entry, then row), so the entries travel ONE TILE AHEAD of the rows: fetch_row_ids reads the
// entries this thread's float4s of a [KT x W] tile belong to (-1 past j_end), fetch_tile_rows starts the row loads from
// entries that are already in registers.
template <int W>
__device__ __forceinline__ void fetch_row_ids(int32_t (&ids)[KT * (W / 4) / 256], const int32_t* __restrict__ rows,
                                              int64_t j0, int64_t j_end) {
#pragma unroll
  for (int p = 0; p < KT * (W / 4) / 256; ++p) {
    const int64_t j = j0 + (p * 256 + (int)threadIdx.x) / (W / 4);
    ids[p] = j < j_end ? rows[j] : -1;
  }
}

template <int W>
__device__ __forceinline__ void fetch_tile_rows(float4 (&regs)[KT * (W / 4) / 256], const float* __restrict__ src,
                                                int64_t ld, const int32_t (&ids)[KT * (W / 4) / 256], int c0, int ncols) {
#pragma unroll
  for (int p = 0; p < KT * (W / 4) / 256; ++p) {
    const int c = ((p * 256 + (int)threadIdx.x) % (W / 4)) * 4;
    regs[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ids[p] >= 0 && c0 + c < ncols) regs[p] = *reinterpret_cast<const float4*>(src + (int64_t)ids[p] * ld + c0 + c);
  }
}

// first list position whose row is >= key (rows ascending)
__device__ __forceinline__ int64_t lower_bound_rows(const int32_t* __restrict__ rows, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rows[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// MT = rows of the output tile a workgroup owns: 128 (each wave a 64 x 64 quadrant = 2 x 2 MFMA blocks) or 64 (each wave
// 32 x 64 = 1 x 2 blocks; M <= 64)
// MODE: the form of the A operand (A_PLAIN, or A_BN / A_ROWS on the 16-byte path; see the head of the file)
template <bool VEC4, int MT, int MODE = A_PLAIN>
__global__ void __launch_bounds__(256)
gemm_tn_partial_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                       float* __restrict__ part, float* __restrict__ colpart, int64_t K, int M, int N,
                       int64_t slab, TnExtra ex) {
  static_assert(MODE == A_PLAIN || VEC4, "the A_BN / A_ROWS forms exist on the 16-byte path only");
  constexpr int MI = MT / 64;  // 32-row MFMA blocks per wave along M
  __shared__ float lds[KT * (MT + 128) + (MODE == A_BN ? 5 * MT : 0)];
  float* la = lds;
  float* lb = lds + KT * MT;
  const int split = blockIdx.x;
  const int m0 = blockIdx.y * MT, n0 = blockIdx.z * BN;
  const int64_t k_begin = (int64_t)split * slab;
  const int64_t k_end = k_begin + slab < K ? k_begin + slab : K;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = (wave >> 1) * (MT / 2), wn = (wave & 1) * 64;
  const int kr = lane >> 5, cc = lane & 31;

  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const bool sums = colpart != nullptr && blockIdx.z == 0 && threadIdx.x < MT;
  float csum = 0.f;
  auto consume = [&]() {  // one staged pair of tiles: column sums of A (optional) + 16 MFMA steps
    if (sums) {  // thread t owns column m0 + t of A (rows past k_end were zero-filled)
#pragma unroll 8
      for (int r = 0; r < KT; ++r) csum += la[r * MT + threadIdx.x];
    }
#pragma unroll 4
    for (int kk = 0; kk < KT; kk += 2) {
      float a[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = la[(kk + kr) * MT + wm + i * 32 + cc];
      const float b0 = lb[(kk + kr) * 128 + wn + cc];
      const float b1 = lb[(kk + kr) * 128 + wn + 32 + cc];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b0, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b1, acc[i][1], 0, 0, 0);
      }
    }
  };
  if constexpr (MODE == A_BN) {
    float* lc = lds + KT * (MT + 128);
    for (int i = threadIdx.x; i < 5 * MT; i += 256) {  // visible after the loop's first barrier
      const float* src = i < MT ? ex.mean : i < 2 * MT ? ex.rstd : i < 3 * MT ? ex.ca : i < 4 * MT ? ex.cb : ex.ck;
      const int c = m0 + i % MT;
      lc[i] = c < M ? src[c] : 0.f;
    }
    float4 ra[KT * (MT / 4) / 256], rx[KT * (MT / 4) / 256], rb[KT * 32 / 256];
    fetch_tile<MT>(ra, A, lda, k_begin, k_end, m0, M);
    fetch_tile<MT>(rx, ex.X, ex.ldx, k_begin, k_end, m0, M);
    fetch_tile<128>(rb, B, ldb, k_begin, k_end, n0, N);
    for (int64_t k0 = k_begin; k0 < k_end; k0 += KT) {
      __syncthreads();
      put_tile_bn<MT>(la, ra, rx, lc, k0, k_end, m0, M);
      put_tile<128>(lb, rb);
      __syncthreads();
      if (k0 + KT < k_end) {
        fetch_tile<MT>(ra, A, lda, k0 + KT, k_end, m0, M);
        fetch_tile<MT>(rx, ex.X, ex.ldx, k0 + KT, k_end, m0, M);
        fetch_tile<128>(rb, B, ldb, k0 + KT, k_end, n0, N);
      }
      consume();
    }
  } else if constexpr (MODE == A_ROWS) {
    // this slab's segment of the list: the entries inside [k_begin, k_end)
    const int64_t j_begin = lower_bound_rows(ex.rows, ex.n_rows, k_begin);
    const int64_t j_end = lower_bound_rows(ex.rows, ex.n_rows, k_end);
    float4 ra[KT * (MT / 4) / 256], rb[KT * 32 / 256];
    int32_t ia[KT * (MT / 4) / 256], ib[KT * 32 / 256];  // list entries of the tile whose rows are fetched NEXT
    fetch_row_ids<MT>(ia, ex.rows, j_begin, j_end);
    fetch_row_ids<128>(ib, ex.rows, j_begin, j_end);
    fetch_tile_rows<MT>(ra, A, lda, ia, m0, M);
    fetch_tile_rows<128>(rb, B, ldb, ib, n0, N);
    fetch_row_ids<MT>(ia, ex.rows, j_begin + KT, j_end);
    fetch_row_ids<128>(ib, ex.rows, j_begin + KT, j_end);
    for (int64_t j0 = j_begin; j0 < j_end; j0 += KT) {
      __syncthreads();
      put_tile<MT>(la, ra);
      put_tile<128>(lb, rb);
      __syncthreads();
      if (j0 + KT < j_end) {  // the rows of tile j0 + KT from entries fetched a tile ago, then the entries of j0 + 2 KT
        fetch_tile_rows<MT>(ra, A, lda, ia, m0, M);
        fetch_tile_rows<128>(rb, B, ldb, ib, n0, N);
        fetch_row_ids<MT>(ia, ex.rows, j0 + 2 * KT, j_end);
        fetch_row_ids<128>(ib, ex.rows, j0 + 2 * KT, j_end);
      }
      consume();
    }
  } else if constexpr (VEC4) {
    float4 ra[KT * (MT / 4) / 256], rb[KT * 32 / 256];
    fetch_tile<MT>(ra, A, lda, k_begin, k_end, m0, M);
    fetch_tile<128>(rb, B, ldb, k_begin, k_end, n0, N);
    for (int64_t k0 = k_begin; k0 < k_end; k0 += KT) {
      __syncthreads();  // the previous tile pair is fully consumed
      put_tile<MT>(la, ra);
      put_tile<128>(lb, rb);
      __syncthreads();
      if (k0 + KT < k_end) {  // next pair in flight while this one is multiplied
        fetch_tile<MT>(ra, A, lda, k0 + KT, k_end, m0, M);
        fetch_tile<128>(rb, B, ldb, k0 + KT, k_end, n0, N);
      }
      consume();
    }
  } else {
    for (int64_t k0 = k_begin; k0 < k_end; k0 += KT) {
      __syncthreads();
      stage_tile<MT>(la, A, lda, k0, k_end, m0, M);
      stage_tile<128>(lb, B, ldb, k0, k_end, n0, N);
      __syncthreads();
      consume();
    }
  }

  if (sums && m0 + (int)threadIdx.x < M) colpart[(int64_t)split * M + m0 + threadIdx.x] = csum;
  // C/D layout of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  float* out = part + (int64_t)split * M * N;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kr;
        const int n = n0 + wn + j * 32 + cc;
        if (m < M && n < N) out[(int64_t)m * N + n] = acc[i][j][r];
      }
}

// 32 consecutive output elements per block; 8 split-lanes per element stride the S partials, then the
// 8 sub-sums are added in lane order: the summation order is fixed, so results are reproducible.
__global__ void __launch_bounds__(256)
gemm_tn_reduce_kernel(const float* __restrict__ part, int S, int64_t MN, float* __restrict__ C, int N,
                      int64_t ldc, float alpha) {
  __shared__ float sh[8][32];
  const int j = threadIdx.x & 31, q = threadIdx.x >> 5;
  for (int64_t base = (int64_t)blockIdx.x * 32; base < MN; base += (int64_t)gridDim.x * 32) {
    const int64_t i = base + j;
    float s = 0.f;
    if (i < MN)
      for (int p = q; p < S; p += 8) s += part[(int64_t)p * MN + i];
    __syncthreads();
    sh[q][j] = s;
    __syncthreads();
    if (q == 0 && i < MN) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t += sh[k][j];
      C[(i / N) * ldc + (i % N)] = alpha * t;
    }
  }
}

int tile_rows(int M) { return M <= 64 ? 64 : BM; }

int choose_splits(int64_t K, int M, int N) {
  const int64_t tiles = cdiv(M, tile_rows(M)) * cdiv(N, BN);
  // ONE round of workgroups over the chip: the kernel's registers (66 VGPRs + 64 accumulators) allow 3 workgroups per
  // CU, so 256 x 3 K-slabs; 1024 (round 3) left a second round of 256 workgroups on an otherwise idle chip:
  // 2 M x 128 x 128: 0.710 -> 0.656 ms (tools/dense_bench.py, profiles/r04_gemm_tn_variants.txt; 4 waves per SIMD by
  // __launch_bounds__ spills 7 registers and gains less)
  int64_t s = cdiv(tile_rows(M) == 64 ? 1024 : 768, tiles);  // the 64-row tile (32 accumulators) fits 4 workgroups per CU
  const int64_t max_s = cdiv(K, 16 * KT);   // at least 16 staged tiles per slab: fewer, longer slabs for small K
                                            // (K = 200 k: 391 partial tiles to reduce instead of 1024)
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  return (int)s;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gemm_tn_workspace_bytes(int64_t K, int64_t M, int64_t N, size_t* bytes) {
  if (!bytes || K < 0 || M < 0 || N < 0) return fail(RGBX_E_ARG, "gemm_tn_workspace_bytes: bad argument");
  if (M >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "gemm_tn: M or N exceeds int32");
  // S partial tiles of C, then S partial column-sum vectors of A
  *bytes = (size_t)choose_splits(K, (int)M, (int)N) * ((size_t)M * (size_t)N + (size_t)M) * sizeof(float);
  return RGBX_OK;
}

namespace rgbx {
namespace {

// The three entry points: argument checks, one partial launch (the form of its A operand by `mode`), the reduce launches
int run_gemm_tn(const char* name, int mode, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                int64_t ldc, float* a_colsum, int64_t K, int64_t M, int64_t N, float alpha, void* workspace,
                size_t workspace_bytes, rgbx_stream_t stream, const TnExtra& ex) {
  if (K < 0 || M < 0 || N < 0) return fail(RGBX_E_ARG, "%s: negative size", name);
  if (M == 0 || N == 0) return RGBX_OK;
  if (!C || (K > 0 && (!A || !B))) return fail(RGBX_E_ARG, "%s: null pointer", name);
  if (M >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: M or N exceeds int32", name);
  if (lda < M || ldb < N || ldc < N) return fail(RGBX_E_ARG, "%s: leading dimension too small", name);
  // 16-byte path: aligned ROWS are enough — a row's last float4 may end in its padding (header: "rows are read in whole
  // 16-byte groups")
  bool v4 = aligned16(A) && aligned16(B) && lda % 4 == 0 && ldb % 4 == 0;
  if (mode == A_BN) {
    if (K > 0 && (!ex.X || !ex.mean || !ex.rstd || !ex.ca || !ex.cb || !ex.ck))
      return fail(RGBX_E_ARG, "%s: null pointer", name);
    if (ex.ldx < M) return fail(RGBX_E_ARG, "%s: leading dimension too small", name);
    v4 = v4 && aligned16(ex.X) && ex.ldx % 4 == 0;
  }
  if (mode == A_ROWS) {
    if (ex.n_rows < 0 || ex.n_rows > K || (ex.n_rows > 0 && !ex.rows)) return fail(RGBX_E_ARG, "%s: bad row list", name);
    if (K >= INT32_MAX) return fail(RGBX_E_RANGE, "%s: K exceeds int32", name);
  }
  if (mode != A_PLAIN && !v4)
    return fail(RGBX_E_ALIGN, "%s: operands must be 16-byte aligned with leading dimensions that are multiples of 4", name);
  size_t need = 0;
  if (int rc = rgbx_gemm_tn_workspace_bytes(K, M, N, &need)) return rc;
  if (!workspace || workspace_bytes < need)
    return fail(RGBX_E_WS, "%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int S = choose_splits(K, (int)M, (int)N);
  const int64_t slab = cdiv(cdiv(K > 0 ? K : 1, S), KT) * KT;
  float* part = static_cast<float*>(workspace);
  float* colpart = a_colsum ? part + (size_t)S * M * N : nullptr;
  const int mt = tile_rows((int)M);
  dim3 grid(S, (unsigned)cdiv(M, mt), (unsigned)cdiv(N, BN));
#define RGBX_GEMM_TN(V4, MT, MODE) \
  gemm_tn_partial_kernel<V4, MT, MODE><<<grid, 256, 0, s>>>(A, lda, B, ldb, part, colpart, K, (int)M, (int)N, slab, ex)
  if (mode == A_BN) { if (mt == 64) RGBX_GEMM_TN(true, 64, A_BN); else RGBX_GEMM_TN(true, 128, A_BN); }
  else if (mode == A_ROWS) { if (mt == 64) RGBX_GEMM_TN(true, 64, A_ROWS); else RGBX_GEMM_TN(true, 128, A_ROWS); }
  else if (v4) { if (mt == 64) RGBX_GEMM_TN(true, 64, A_PLAIN); else RGBX_GEMM_TN(true, 128, A_PLAIN); }
  else { if (mt == 64) RGBX_GEMM_TN(false, 64, A_PLAIN); else RGBX_GEMM_TN(false, 128, A_PLAIN); }
#undef RGBX_GEMM_TN
  RGBX_CHECK_LAUNCH("gemm_tn_partial_kernel");
  const int64_t MN = M * N;
  int64_t rb = cdiv(MN, 32);
  if (rb > kMaxGrid) rb = kMaxGrid;
  gemm_tn_reduce_kernel<<<(int)rb, 256, 0, s>>>(part, S, MN, C, (int)N, ldc, alpha);
  RGBX_CHECK_LAUNCH("gemm_tn_reduce_kernel");
  if (a_colsum) {  // the same slab-ordered reduction over the [S, M] column-sum partials (unscaled)
    gemm_tn_reduce_kernel<<<(int)cdiv(M, 32), 256, 0, s>>>(colpart, S, M, a_colsum, (int)M, M, 1.0f);
    RGBX_CHECK_LAUNCH("gemm_tn_reduce_kernel");
  }
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

extern "C" int rgbx_gemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                                int64_t ldc, float* a_colsum, int64_t K, int64_t M, int64_t N, float alpha,
                                void* workspace, size_t workspace_bytes, rgbx_stream_t stream) {
  return run_gemm_tn("gemm_tn", A_PLAIN, A, lda, B, ldb, C, ldc, a_colsum, K, M, N, alpha, workspace, workspace_bytes,
                     stream, TnExtra{});
}

extern "C" int rgbx_gemm_tn_bn_bwd_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, const float* mean,
                                       const float* rstd, const float* ca, const float* cb, const float* ck,
                                       const float* B, int64_t ldb, float* C, int64_t ldc, float* a_colsum, int64_t K,
                                       int64_t M, int64_t N, float alpha, void* workspace, size_t workspace_bytes,
                                       rgbx_stream_t stream) {
  TnExtra ex{};
  ex.X = X, ex.ldx = ldx, ex.mean = mean, ex.rstd = rstd, ex.ca = ca, ex.cb = cb, ex.ck = ck;
  return run_gemm_tn("gemm_tn_bn_bwd", A_BN, G, ldg, B, ldb, C, ldc, a_colsum, K, M, N, alpha, workspace,
                     workspace_bytes, stream, ex);
}

extern "C" int rgbx_gemm_tn_rows_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                                     int64_t n_rows, float* C, int64_t ldc, float* a_colsum, int64_t K, int64_t M,
                                     int64_t N, float alpha, void* workspace, size_t workspace_bytes,
                                     rgbx_stream_t stream) {
  TnExtra ex{};
  ex.rows = rows, ex.n_rows = n_rows;
  return run_gemm_tn("gemm_tn_rows", A_ROWS, A, lda, B, ldb, C, ldc, a_colsum, K, M, N, alpha, workspace,
                     workspace_bytes, stream, ex);
}
