// GGNN (PyG GatedGraphConv, reference models/ggnn.py) — one propagation step is
//   m = x weight[i];  agg = A m (plain edge sum);  x' = GRUCell(agg, x)
// and by (A x) weight[i] W_ihᵀ = (A x) (W_ih weight[i]ᵀ)ᵀ the whole step is one gather of x at the state width C followed
// by two [C -> 4C] products of the same 32-row tile:
//   pre = (A x) Weffᵀ + x Wrootᵀ + bias, columns [ r, z pre-activations (2C) | gi_n (C) | gh_n (C) ]
//   r = σ(pre_r), z = σ(pre_z), n = tanh(gi_n + r ⊙ gh_n), x' = (1 - z) ⊙ n + z ⊙ x
// (ops.gru_step forms Weff / Wroot / bias from the parameters).
//
// Kernels:
//  - gru_step_kernel: the FUSED step. A workgroup (4 waves) owns 32 destination rows. Phase 1 gathers their aggregates
//    exactly like spmm_linear_kernel's row-per-wave loop (G lanes x float4 per neighbour row, NG x 4 neighbour rows in
//    flight, rows handed out from an LDS counter; hub rows read from the split-row kernels' compact aggregates) and
//    parks them in LDS next to the tile's own rows. Phase 2 runs both products on v_mfma_f32_32x32x2_f32 into the
//    same accumulators (the r / z columns take both, gi_n only the first, gh_n only the second: Weff's gh_n block and
//    Wroot's gi_n block are zero). The r / z / n / gh_n columns of one state column fall on different waves' column
//    tiles, so the finished [32, 4C] tile is parked in LDS (over the dead input tiles) and the GRU epilogue reads it
//    back by state column. Only x' [N, C] is written; a training forward also writes what the backward needs: the
//    aggregate A x (the weight gradient dWeff = dpreᵀ (A x) reads it) and pre.
//    Saved for the backward: pre, not a recompute. Storing pre costs a [N, 4C] write in the forward and a read in the
//    gate backward (2 + 2 GB at |V| = 2 M, C = 64); recomputing it from the stored aggregate reads A x and x (1 GB),
//    writes pre (2 GB) and reads it again in the gate backward (2 GB) unless the recompute and the gate backward are one
//    kernel — 1 GB more per step and one more launch.
//  - gru_gate_fwd_kernel / gru_gate_bwd_kernel: the GRU cell over a finished pre [N, 4C] — the composed and the general
//    forms' epilogue, and the backward of every form:
//      dn = dx' (1 - z), dz = dx' (x - n), dgi_n = dn (1 - n²), dgh_n = dgi_n r, dr = dgi_n gh_n,
//      dpre = [dr r (1 - r) | dz z (1 - z) | dgi_n | dgh_n],   dx_direct = dx' z.
#include "rgbx_common.h"
#include "spmm_internal.h"

namespace rgbx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f4v = __attribute__((ext_vector_type(4))) float;

constexpr int TM = kTileRows;
constexpr int kMaxStepC = 64;  // Nout = 4 C <= 256: at most two 32-column output tiles per wave

__device__ __forceinline__ void nt_store4(float* p, const float (&v)[4]) {
  f4v t = {v[0], v[1], v[2], v[3]};
  __builtin_nontemporal_store(t, reinterpret_cast<f4v*>(p));
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// One GRU cell on four state columns: pr / pz / gin / ghn = pre-activations, h = old state -> new state.
__device__ __forceinline__ void gru_cell4(const float (&pr)[4], const float (&pz)[4], const float (&gin)[4],
                                          const float (&ghn)[4], const float (&h)[4], float (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float r = sigmoidf(pr[i]), z = sigmoidf(pz[i]);
    const float n = tanhf(fmaf(r, ghn[i], gin[i]));
    o[i] = fmaf(z, h[i] - n, n);  // (1 - z) n + z h
  }
}

struct StepArgs {
  const int* rowptr;
  const int* col;
  const float* x;     // [N, C] (ldx): gathered and the tile's own rows
  const float* wt;    // Weffᵀ [C, 4C]
  const float* wtr;   // Wrootᵀ [C, 4C]
  const float* bias;  // [4C]
  float* out;         // x' [N, C] (ldo)
  float* z_out;       // A x [N, C] (ldz) or NULL
  float* pre_out;     // pre [N, 4C] (ldp) or NULL
  int64_t ldx, ldo, ldz, ldp;
  const int* long_row;
  const float* zlong;
  int threshold, n_long;
  int N, C;
};

// KC: the state width as a compile-time constant (the MFMA loops unroll), 0 = any supported C.
template <int G, int KC>
__global__ void __launch_bounds__(256, 4) gru_step_kernel(const StepArgs A) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  constexpr int VPT = 2;  // own-row float4 per thread: 32 rows x C / 4 <= 512 = 2 x 256
  extern __shared__ float lds[];
  const int C = KC ? KC : A.C;
  const int Nout = 4 * C;
  const int ldz = C + 4;
  float* zt = lds;                // [TM][C + 4] aggregates
  float* xt = lds + TM * ldz;     // [TM][C + 4] own rows
  float* pt = lds;                // [TM][4C + 4] the finished pre tile (after phase 2)
  const int ldq = Nout + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, t = lane % G;
  const int c = t * 4;
  const bool active = c < C;
  const int row_base = blockIdx.x * TM;
  const int c4n = C >> 2;

  // the tile's own rows: loaded first (their latency passes under the gather), kept in registers for the epilogue
  float hv[VPT][4];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int idx = threadIdx.x + j * 256;
    const int r = idx / c4n, c4 = (idx - r * c4n) * 4;
    const int row = row_base + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) hv[j][i] = 0.f;
    if (r < TM && row < A.N) load_vec<4>(hv[j], A.x + (int64_t)row * A.ldx + c4);
  }

  // ---- phase 1: aggregates of the 32 rows, handed to the waves one at a time
  __shared__ int next_row;
  if (threadIdx.x == 0) next_row = 0;
  __syncthreads();
  for (;;) {
    int lr = 0;
    if (lane == 0) lr = atomicAdd(&next_row, 1);
    lr = __builtin_amdgcn_readfirstlane(lr);
    if (lr >= TM) break;
    const int row = row_base + lr;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < A.N) {
      const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
      const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
      if (A.threshold > 0 && end - start > A.threshold) {
        // hub row (wave-uniform): its aggregate was finished by the split-row kernels
        int lo = 0, hi = A.n_long - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (A.long_row[mid] < row) lo = mid + 1;
          else hi = mid;
        }
        if (g == 0 && active) load_vec<4>(acc, A.zlong + (int64_t)lo * C + c);
      } else {
        const float* xc = A.x + c;
        for (int base = start; base < end; base += kWave) {
          const int n = min(kWave, end - base);
          int mycol = 0;
          if (lane < n) mycol = A.col[base + lane];
          for (int k = 0; k < n; k += NG * U) {
            float v[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int idx = k + u * NG + g;
              const int src = __shfl(mycol, idx & 63);
#pragma unroll
              for (int i = 0; i < 4; ++i) v[u][i] = 0.f;
              if (active && idx < n) load_vec<4>(v[u], xc + (int64_t)src * A.ldx);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[i] += v[u][i];
            }
          }
        }
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], off);
        }
      }
    }
    if (g == 0 && active) {
      store_vec<4>(&zt[lr * ldz + c], acc);
      if (A.z_out && row < A.N) nt_store4(A.z_out + (int64_t)row * A.ldz + c, acc);
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int idx = threadIdx.x + j * 256;
    const int r = idx / c4n, c4 = (idx - r * c4n) * 4;
    if (r < TM) store_vec<4>(&xt[r * ldz + c4], hv[j]);
  }
  __syncthreads();

  // ---- phase 2: acc = zt Weffᵀ + xt Wrootᵀ (+ bias); wave w owns the 32-column tiles w and w + 4
  const int kr = lane >> 5, cc = lane & 31;
  f32x16 acc[2];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
    const int n0 = wave * 32 + tt * 128;
    if (n0 < Nout) {
      for (int ks = 0; ks < C; ks += 2) {
        const float b0 = A.wt[(int64_t)(ks + kr) * Nout + n0 + cc];
        const float b1 = A.wtr[(int64_t)(ks + kr) * Nout + n0 + cc];
        const float a0 = zt[cc * ldz + ks + kr], a1 = xt[cc * ldz + ks + kr];
        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[tt], 0, 0, 0);
        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[tt], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wave is done reading zt / xt: the pre tile goes over them
  // C/D layout of the 32x32 MFMA: column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5)
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int n0 = wave * 32 + tt * 128;
    if (n0 < Nout) {
      const float bb = A.bias[n0 + cc];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * kr;
        const float v = acc[tt][r] + bb;
        pt[rl * ldq + n0 + cc] = v;
        const int row = row_base + rl;
        if (A.pre_out && row < A.N) __builtin_nontemporal_store(v, &A.pre_out[(int64_t)row * A.ldp + n0 + cc]);
      }
    }
  }
  __syncthreads();

  // ---- GRU epilogue: the same (row, 4 columns) mapping as the own-row load above
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int idx = threadIdx.x + j * 256;
    const int r = idx / c4n, c4 = (idx - r * c4n) * 4;
    const int row = row_base + r;
    if (r < TM && row < A.N) {
      float pr[4], pz[4], gin[4], ghn[4], o[4];
      const float* q = &pt[r * ldq + c4];
      load_vec<4>(pr, q);
      load_vec<4>(pz, q + C);
      load_vec<4>(gin, q + 2 * C);
      load_vec<4>(ghn, q + 3 * C);
      gru_cell4(pr, pz, gin, ghn, hv[j], o);
      nt_store4(A.out + (int64_t)row * A.ldo + c4, o);
    }
  }
}

// Thread = (row, 4 state columns), grid-stride.
__global__ void __launch_bounds__(256) gru_gate_fwd_kernel(const float* __restrict__ pre, int64_t ldp,
                                                           const float* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ out, int64_t ldo, int64_t N, int C) {
  const int c4n = C >> 2;
  const int64_t total = N * c4n;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / c4n;
    const int c4 = (int)(idx - row * c4n) * 4;
    const float* p = pre + row * ldp + c4;
    float pr[4], pz[4], gin[4], ghn[4], h[4], o[4];
    load_vec<4>(pr, p);
    load_vec<4>(pz, p + C);
    load_vec<4>(gin, p + 2 * C);
    load_vec<4>(ghn, p + 3 * C);
    load_vec<4>(h, x + row * ldx + c4);
    gru_cell4(pr, pz, gin, ghn, h, o);
    store_vec<4>(out + row * ldo + c4, o);
  }
}

__global__ void __launch_bounds__(256) gru_gate_bwd_kernel(const float* __restrict__ pre, int64_t ldp,
                                                           const float* __restrict__ x, int64_t ldx,
                                                           const float* __restrict__ gout, int64_t ldg,
                                                           float* __restrict__ dpre, int64_t lddp,
                                                           float* __restrict__ dx, int64_t lddx, int64_t N, int C) {
  const int c4n = C >> 2;
  const int64_t total = N * c4n;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / c4n;
    const int c4 = (int)(idx - row * c4n) * 4;
    const float* p = pre + row * ldp + c4;
    float pr[4], pz[4], gin[4], ghn[4], h[4], go[4];
    load_vec<4>(pr, p);
    load_vec<4>(pz, p + C);
    load_vec<4>(gin, p + 2 * C);
    load_vec<4>(ghn, p + 3 * C);
    load_vec<4>(h, x + row * ldx + c4);
    load_vec<4>(go, gout + row * ldg + c4);
    float dr[4], dz[4], dgin[4], dghn[4], dh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = sigmoidf(pr[i]), z = sigmoidf(pz[i]);
      const float n = tanhf(fmaf(r, ghn[i], gin[i]));
      const float dn = go[i] * (1.f - z);
      dgin[i] = dn * (1.f - n * n);
      dghn[i] = dgin[i] * r;
      dr[i] = dgin[i] * ghn[i] * r * (1.f - r);
      dz[i] = go[i] * (h[i] - n) * z * (1.f - z);
      dh[i] = go[i] * z;
    }
    float* q = dpre + row * lddp + c4;
    store_vec<4>(q, dr);
    store_vec<4>(q + C, dz);
    store_vec<4>(q + 2 * C, dgin);
    store_vec<4>(q + 3 * C, dghn);
    store_vec<4>(dx + row * lddx + c4, dh);
  }
}

int gate_grid(int64_t N, int C) {
  const int64_t blocks = cdiv(N * (C / 4), 256);
  return (int)std::min<int64_t>(std::max<int64_t>(blocks, 1), kMaxGrid);
}

template <int G, int KC>
int launch_step(const StepArgs& A, hipStream_t s) {
  const int C = KC ? KC : A.C;
  const size_t lds = (size_t)TM * std::max(2 * (C + 4), 4 * C + 4) * sizeof(float);
  gru_step_kernel<G, KC><<<(int)cdiv(A.N, TM), 256, lds, s>>>(A);
  RGBX_CHECK_LAUNCH("gru_step_kernel");
  return RGBX_OK;
}

bool ok16(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_gru_step_supported(int64_t C) { return C >= 8 && C % 8 == 0 && C <= kMaxStepC; }

extern "C" int rgbx_gru_step_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                                 const float* wt, const float* wt_root, const float* bias, float* out, int64_t ldo,
                                 float* z_out, int64_t ldz, float* pre_out, int64_t ldp, int64_t N, int64_t C,
                                 const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || C <= 0) return fail(RGBX_E_ARG, "gru_step: bad size");
  if (!rowptr || !col || !x || !wt || !wt_root || !bias || !out) return fail(RGBX_E_ARG, "gru_step: null pointer");
  if (!rgbx_gru_step_supported(C))
    return fail(RGBX_E_SHAPE, "gru_step: needs C %% 8 == 0, 8 <= C <= %d (got C=%lld)", kMaxStepC, (long long)C);
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "gru_step: N exceeds int32");
  if (ldx < C || ldo < C || (z_out && ldz < C) || (pre_out && ldp < 4 * C))
    return fail(RGBX_E_ARG, "gru_step: leading dimension too small");
  if (!ok16(x, ldx) || !ok16(out, ldo) || (z_out && !ok16(z_out, ldz)) || (pre_out && !ok16(pre_out, ldp)))
    return fail(RGBX_E_ALIGN, "gru_step: x / out / z_out / pre_out must be 16-byte aligned with ld %% 4 == 0");
  if (out == x) return fail(RGBX_E_ARG, "gru_step: out must not alias x");
  if (N == 0) return RGBX_OK;
  hipStream_t s = (hipStream_t)stream;
  StepArgs A{rowptr, col, x, wt, wt_root, bias, out, z_out, pre_out, ldx, ldo, ldz, ldp,
             nullptr, nullptr, 0, 0, (int)N, (int)C};
  if (split && split->threshold > 0 && split->n_chunks > 0) {
    // hub rows first: chunk sums + ordered combine into [n_long, C] behind the [n_chunks, C] partials
    float* zl = split->partial ? split->partial + (size_t)split->n_chunks * C : nullptr;
    if (int rc = spmm_long_rows_compact(rowptr, col, nullptr, nullptr, x, ldx, (int)C, split, zl, s)) return rc;
    A.long_row = split->long_row;
    A.zlong = zl;
    A.threshold = split->threshold;
    A.n_long = split->n_long;
  }
  const int lanes = (int)(C / 4);
  if (C == 64) return launch_step<16, 64>(A, s);
  if (C == 32) return launch_step<8, 32>(A, s);
  if (lanes <= 2) return launch_step<2, 0>(A, s);
  if (lanes <= 4) return launch_step<4, 0>(A, s);
  if (lanes <= 8) return launch_step<8, 0>(A, s);
  return launch_step<16, 0>(A, s);
}

extern "C" int rgbx_gru_gate_fwd_f32(const float* pre, int64_t ldp, const float* x, int64_t ldx, float* out,
                                     int64_t ldo, int64_t N, int64_t C, rgbx_stream_t stream) {
  if (N < 0 || C <= 0) return fail(RGBX_E_ARG, "gru_gate_fwd: bad size");
  if (!pre || !x || !out) return fail(RGBX_E_ARG, "gru_gate_fwd: null pointer");
  if (C % 4) return fail(RGBX_E_SHAPE, "gru_gate_fwd: needs C %% 4 == 0 (got C=%lld)", (long long)C);
  if (C >= INT32_MAX / 4) return fail(RGBX_E_RANGE, "gru_gate_fwd: C too large");
  if (ldp < 4 * C || ldx < C || ldo < C) return fail(RGBX_E_ARG, "gru_gate_fwd: leading dimension too small");
  if (!ok16(pre, ldp) || !ok16(x, ldx) || !ok16(out, ldo))
    return fail(RGBX_E_ALIGN, "gru_gate_fwd: pre / x / out must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  gru_gate_fwd_kernel<<<gate_grid(N, (int)C), 256, 0, (hipStream_t)stream>>>(pre, ldp, x, ldx, out, ldo, N, (int)C);
  RGBX_CHECK_LAUNCH("gru_gate_fwd_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_gru_gate_bwd_f32(const float* pre, int64_t ldp, const float* x, int64_t ldx, const float* gout,
                                     int64_t ldg, float* dpre, int64_t lddp, float* dx, int64_t lddx, int64_t N,
                                     int64_t C, rgbx_stream_t stream) {
  if (N < 0 || C <= 0) return fail(RGBX_E_ARG, "gru_gate_bwd: bad size");
  if (!pre || !x || !gout || !dpre || !dx) return fail(RGBX_E_ARG, "gru_gate_bwd: null pointer");
  if (C % 4) return fail(RGBX_E_SHAPE, "gru_gate_bwd: needs C %% 4 == 0 (got C=%lld)", (long long)C);
  if (C >= INT32_MAX / 4) return fail(RGBX_E_RANGE, "gru_gate_bwd: C too large");
  if (ldp < 4 * C || ldx < C || ldg < C || lddp < 4 * C || lddx < C)
    return fail(RGBX_E_ARG, "gru_gate_bwd: leading dimension too small");
  if (!ok16(pre, ldp) || !ok16(x, ldx) || !ok16(gout, ldg) || !ok16(dpre, lddp) || !ok16(dx, lddx))
    return fail(RGBX_E_ALIGN, "gru_gate_bwd: every matrix must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  gru_gate_bwd_kernel<<<gate_grid(N, (int)C), 256, 0, (hipStream_t)stream>>>(pre, ldp, x, ldx, gout, ldg, dpre, lddp,
                                                                            dx, lddx, N, (int)C);
  RGBX_CHECK_LAUNCH("gru_gate_bwd_kernel");
  return RGBX_OK;
}
