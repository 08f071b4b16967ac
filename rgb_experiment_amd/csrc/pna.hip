// PNAConv's degree-scaled multi-aggregation (Corso et al., "Principal Neighbourhood Aggregation for Graph Nets") for
// gfx950: the statistics of a per-edge message from ONE gather, every statistic multiplied by several functions of the
// in-degree and stored straight into PyG's concatenated layout, and the two backward passes. Stands in for
// PNAConv.message (pre_layers = 1) + DegreeScalerAggregation [PyG].
//
// For an edge j -> i in forward CSR slot p, b [N, d] per source, c [nnz, d] one row PER SLOT (may be absent), a [N, d]
// per target (may be absent), d = T * F (T towers of F channels):
//   u_p    = b[j,:] + c[p,:]                                   (one fp32 add)
//   stat_k = sum | mean | var | std | max | min of u_p over the n slots of row i      (multi_aggr.hip's definitions)
//   shift  : mean, max, min += a[i,:];  sum += n a[i,:];  var, std unchanged;  a row without slots stays 0
//   scale_s: 1 | log(D+1)/avg_log | avg_log/log(D+1) | D/avg_lin | avg_lin/D,   D = max(n, 1)
//   out[i, t*S*A*F + (s*A + k)*F + f] = scale_s(i) * stat_k[i, t*F + f]
// The message of PNAConv is linear in (x_i, x_j, e_ji) in front of the aggregation, so it splits into a target part a
// (which every statistic but the second moments simply carries along), a source part b and an edge part c; only b + c
// has to be walked per slot. avg_deg = [avg_lin, avg_log] is read from DEVICE memory.
//
// Lane layout, second moment (shifted sums, exact re-basing across hub-row chunks), extrema and ties: multi_aggr.hip's,
// copied here (that file stays as it is); with c absent the statistics have that kernel's bits. The c rows of a target
// are consecutive, so they are read as a stream beside the gather of b (as gine.hip reads e). After the butterfly every
// lane group of a wave holds the row's finished record, so the S * A output blocks are dealt out over the groups:
// group g stores blocks g, g + NG, ...
//
// Backward, with per-TARGET rows the caller prepares (G_k = sum_s scale_s g_out[(s,k)]; B = G_std / (n std) + 2 G_var / n;
// A = G_sum + G_mean / n - B mean_u), bracket(i, p) = A[i] + B[i] u_p + Gmax[i] [argmax[i] == p] + Gmin[i] [argmin[i] == p]:
//   source pass, TRANSPOSED CSR: g_b[j,:] = sum over the out-edges q of j of bracket(col_t[q], t2f[q])
//   edge pass, forward CSR     : g_c[p,:] = bracket(i, p), one row per slot, every slot row written
// u is recomputed from the forward's own add. No float atomics; every sum runs in a fixed order (slots of a lane group in
// slot order, groups by a butterfly, hub-row chunks in chunk order): two runs give the same bits. Inputs are finite.
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

__device__ __forceinline__ void nt_store(float* p, const float (&v)[4]) {
  f4v o = {v[0], v[1], v[2], v[3]};
  __builtin_nontemporal_store(o, reinterpret_cast<f4v*>(p));
}

// `a` at slot `sa` beats `b` at slot `sb`: strictly better, or equal and from a lower slot (-1 = no slot: the highest unsigned)
template <bool MAX>
__device__ __forceinline__ bool beats(float a, int sa, float b, int sb) {
  const bool better = MAX ? a > b : a < b;
  return better || (a == b && (unsigned)sa < (unsigned)sb);
}

constexpr float kStdFloor = 1e-5f;  // PyG StdAggregation: sqrt(var.clamp(min=1e-5)), 0 where that is <= sqrt(1e-5)
constexpr int kMaxScalers = 8;

struct PnaArgs {
  const int* rowptr;
  const int* col;
  const float* b;
  const float* c;  // per slot, or NULL
  const float* a;  // per target, or NULL
  int64_t ldb, ldc, lda;
  const float* avg_deg;  // [avg_lin, avg_log], device
  rgbx_pna_out_t o;
  int N, d, F;
  int n_aggr, n_scalers;
  int pos[6];  // output position k of sum, mean, var, std, max, min; -1 = not wanted
  int scaler[kMaxScalers];
  int skip_longer;
};

// This lane's 4 columns. M1: sum / mean wanted, M2: var / std wanted, MAX / MIN: that extremum wanted; members of a
// statistic that is not wanted are never touched.
struct Rec {
  int n;  // slots behind dev / sq
  float s[4];
  float dev[4], sq[4], shift[4];
  float maxv[4], minv[4];
  int maxs[4], mins[4];
};

template <bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void rec_init(Rec& R) {
  R.n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (M1) R.s[i] = 0.f;
    if constexpr (M2) { R.dev[i] = 0.f; R.sq[i] = 0.f; R.shift[i] = 0.f; }
    if constexpr (MAX) { R.maxv[i] = -INFINITY; R.maxs[i] = -1; }
    if constexpr (MIN) { R.minv[i] = INFINITY; R.mins[i] = -1; }
  }
}

// (na, dev, sq, shift) <- itself merged with (nb, db, qb, kb), re-based onto its own shift (onto kb where it is empty)
__device__ __forceinline__ void merge_moments(int na, float& dev, float& sq, float& shift, int nb, float db, float qb, float kb) {
  const float k = na == 0 ? kb : shift;
  const float delta = kb - k;
  const float fb = (float)nb;
  dev = dev + fmaf(fb, delta, db);
  sq = sq + fmaf(delta, fmaf(fb, delta, 2.f * db), qb);
  shift = k;
}

// Slots [start, end): the statistics of u = b[col[p]] + c[p] in this lane's 4 columns (column offset c0), the NG groups
// merged on return and the merged record in EVERY group. Every group deviates from the SAME shift, the u of slot `start`.
template <int G, bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void pna_slots(const PnaArgs& A, int start, int end, int c0, bool active, int lane, int g,
                                          Rec& R) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  const float* bc = A.b + c0;
  const float* cc = A.c ? A.c + c0 : nullptr;
  rec_init<M1, M2, MAX, MIN>(R);
  R.n = end - start;
  if constexpr (M2) {
    if (active && end > start) {  // one row, the same for all groups
      load_vec<4>(R.shift, bc + (int64_t)A.col[start] * A.ldb);
      if (cc) {
        float cv[4];
        load_vec<4>(cv, cc + (int64_t)start * A.ldc);
#pragma unroll
        for (int i = 0; i < 4; ++i) R.shift[i] += cv[i];
      }
    }
  }
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int mycol = lane < n ? A.col[base + lane] : 0;
    for (int k = 0; k < n; k += NG * U) {
      float v[U][4], cv[U][4];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int src = __shfl(mycol, idx & 63);
        ok[u] = active && idx < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[u][i] = cv[u][i] = 0.f;
        if (ok[u]) {
          load_vec<4>(v[u], bc + (int64_t)src * A.ldb);
          if (cc) load_vec<4>(cv[u], cc + (int64_t)(base + idx) * A.ldc);
        }
      }
      if (cc) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[u][i] += cv[u][i];  // a slot past the end: 0 + 0
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int p = base + k + u * NG + g;  // ascending within the group: strict comparison keeps the lowest slot
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (M1) R.s[i] += v[u][i];
          if constexpr (M2) {
            const float dv = ok[u] ? v[u][i] - R.shift[i] : 0.f;
            R.dev[i] += dv;
            R.sq[i] = fmaf(dv, dv, R.sq[i]);
          }
          if constexpr (MAX) {
            const bool take = ok[u] && v[u][i] > R.maxv[i];
            R.maxv[i] = take ? v[u][i] : R.maxv[i];
            R.maxs[i] = take ? p : R.maxs[i];
          }
          if constexpr (MIN) {
            const bool take = ok[u] && v[u][i] < R.minv[i];
            R.minv[i] = take ? v[u][i] : R.minv[i];
            R.mins[i] = take ? p : R.mins[i];
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (M1) R.s[i] += __shfl_xor(R.s[i], off);
      if constexpr (M2) {
        R.dev[i] += __shfl_xor(R.dev[i], off);
        R.sq[i] += __shfl_xor(R.sq[i], off);
      }
      if constexpr (MAX) {
        const float ob = __shfl_xor(R.maxv[i], off);
        const int os = __shfl_xor(R.maxs[i], off);
        const bool take = beats<true>(ob, os, R.maxv[i], R.maxs[i]);
        R.maxv[i] = take ? ob : R.maxv[i];
        R.maxs[i] = take ? os : R.maxs[i];
      }
      if constexpr (MIN) {
        const float ob = __shfl_xor(R.minv[i], off);
        const int os = __shfl_xor(R.mins[i], off);
        const bool take = beats<false>(ob, os, R.minv[i], R.mins[i]);
        R.minv[i] = take ? ob : R.minv[i];
        R.mins[i] = take ? os : R.mins[i];
      }
    }
  }
}

// scale_s of a row of D = max(n, 1) slots
__device__ __forceinline__ float scale_of(int kind, float D, float logD, float avg_lin, float avg_log) {
  switch (kind) {
    case RGBX_PNA_AMPLIFICATION: return logD / avg_log;
    case RGBX_PNA_ATTENUATION: return avg_log / logD;
    case RGBX_PNA_LINEAR: return D / avg_lin;
    case RGBX_PNA_INVERSE_LINEAR: return avg_lin / D;
  }
  return 1.f;
}

// The finished row `row` (n slots), columns c..c+3: the raw statistics the backward wants (`keep`: one caller per row and
// column stores them), then the shift by a and the S * A scaled blocks j = j0, j0 + jstep, ... of the tower of column c.
template <bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void pna_store(const PnaArgs& A, int row, int c, int n, const Rec& R, bool keep, int j0,
                                          int jstep) {
  const rgbx_pna_out_t& o = A.o;
  const float inv = 1.f / (float)max(n, 1);
  float sum[4], mean[4], var[4], sd[4], mx[4], mn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sum[i] = mean[i] = var[i] = sd[i] = mx[i] = mn[i] = 0.f;
  if constexpr (M1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { sum[i] = R.s[i]; mean[i] = R.s[i] * inv; }
    if (keep && o.mean) nt_store(o.mean + (int64_t)row * o.ld_mean + c, mean);
  }
  if constexpr (M2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float md = R.dev[i] * inv;
      var[i] = fmaf(-md, md, R.sq[i] * inv);
      sd[i] = var[i] > kStdFloor ? sqrtf(var[i]) : 0.f;
    }
    if (keep && o.var) nt_store(o.var + (int64_t)row * o.ld_var + c, var);
    if (keep && o.std) nt_store(o.std + (int64_t)row * o.ld_std + c, sd);
  }
  if constexpr (MAX) {
#pragma unroll
    for (int i = 0; i < 4; ++i) mx[i] = R.maxs[i] < 0 ? 0.f : R.maxv[i];
    if (keep && o.argmax) {
      i4v s = {R.maxs[0], R.maxs[1], R.maxs[2], R.maxs[3]};
      __builtin_nontemporal_store(s, reinterpret_cast<i4v*>(o.argmax + (int64_t)row * o.ld_argmax + c));
    }
  }
  if constexpr (MIN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) mn[i] = R.mins[i] < 0 ? 0.f : R.minv[i];
    if (keep && o.argmin) {
      i4v s = {R.mins[0], R.mins[1], R.mins[2], R.mins[3]};
      __builtin_nontemporal_store(s, reinterpret_cast<i4v*>(o.argmin + (int64_t)row * o.ld_argmin + c));
    }
  }
  if (A.a && n > 0) {  // no message, nothing to shift
    float av[4];
    load_vec<4>(av, A.a + (int64_t)row * A.lda + c);
    const float fn = (float)n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (M1) { sum[i] = fmaf(fn, av[i], sum[i]); mean[i] += av[i]; }
      if constexpr (MAX) mx[i] = R.maxs[i] < 0 ? 0.f : mx[i] + av[i];
      if constexpr (MIN) mn[i] = R.mins[i] < 0 ? 0.f : mn[i] + av[i];
    }
  }
  const float D = (float)max(n, 1);
  const float logD = logf(D + 1.f);
  const float avg_lin = A.avg_deg[0], avg_log = A.avg_deg[1];
  const int t = c / A.F, f = c - t * A.F;
  const int blocks = A.n_scalers * A.n_aggr;
  float* dst = o.out + (int64_t)row * o.ld_out + (int64_t)t * blocks * A.F + f;
  for (int j = j0; j < blocks; j += jstep) {
    const int s = j / A.n_aggr, k = j - s * A.n_aggr;
    float val[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x = 0.f;
      if constexpr (M1) x = k == A.pos[0] ? sum[i] : (k == A.pos[1] ? mean[i] : x);
      if constexpr (M2) x = k == A.pos[2] ? var[i] : (k == A.pos[3] ? sd[i] : x);
      if constexpr (MAX) x = k == A.pos[4] ? mx[i] : x;
      if constexpr (MIN) x = k == A.pos[5] ? mn[i] : x;
      val[i] = x;
    }
    const int kind = A.scaler[s];
    if (n == 0) {  // exact zeros whatever the averages are
#pragma unroll
      for (int i = 0; i < 4; ++i) val[i] = 0.f;
    } else if (kind != RGBX_PNA_IDENTITY) {
      const float fac = scale_of(kind, D, logD, avg_lin, avg_log);
#pragma unroll
      for (int i = 0; i < 4; ++i) val[i] *= fac;
    }
    nt_store(dst + (int64_t)j * A.F, val);
  }
}

template <int G, bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256) pna_fwd_kernel(const PnaArgs A) {
  constexpr int NG = kWave / G;
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;  // the chunk + combine kernels own long rows
  Rec R;
  pna_slots<G, M1, M2, MAX, MIN>(A, start, end, c, active, lane, g, R);
  if (active) pna_store<M1, M2, MAX, MIN>(A, row, c, end - start, R, g == 0, g, NG);
}

// Chunk records in split->partial: one [n_chunks, d] section of 4-byte words per kept quantity, in this order.
template <bool M1, bool M2, bool MAX, bool MIN>
struct Sections {
  static constexpr int kS = 0;
  static constexpr int kDev = kS + (M1 ? 1 : 0);
  static constexpr int kSq = kDev + (M2 ? 1 : 0);
  static constexpr int kShift = kSq + (M2 ? 1 : 0);
  static constexpr int kMaxV = kShift + (M2 ? 1 : 0);
  static constexpr int kMaxS = kMaxV + (MAX ? 1 : 0);
  static constexpr int kMinV = kMaxS + (MAX ? 1 : 0);
  static constexpr int kMinS = kMinV + (MIN ? 1 : 0);
};

inline int sections_of(int which) {
  const bool m1 = which & (RGBX_MULTI_SUM | RGBX_MULTI_MEAN), m2 = which & (RGBX_MULTI_VAR | RGBX_MULTI_STD);
  return (m1 ? 1 : 0) + (m2 ? 3 : 0) + ((which & RGBX_MULTI_MAX) ? 2 : 0) + ((which & RGBX_MULTI_MIN) ? 2 : 0);
}

// One wave per chunk of a long row: the chunk's record of u into the partial sections.
template <int G, bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256)
pna_chunk_kernel(const PnaArgs A, int n_chunks, const int* __restrict__ chunk_begin, const int* __restrict__ chunk_end,
                 float* __restrict__ partial) {
  using S = Sections<M1, M2, MAX, MIN>;
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  const int64_t sec = (int64_t)n_chunks * A.d;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    Rec R;
    pna_slots<G, M1, M2, MAX, MIN>(A, start, end, c, active, lane, g, R);
    if (g == 0 && active) {
      float* p = partial + (int64_t)ch * A.d + c;
      if constexpr (M1) store_vec<4>(p + S::kS * sec, R.s);
      if constexpr (M2) {
        store_vec<4>(p + S::kDev * sec, R.dev);
        store_vec<4>(p + S::kSq * sec, R.sq);
        store_vec<4>(p + S::kShift * sec, R.shift);
      }
      if constexpr (MAX) {
        store_vec<4>(p + S::kMaxV * sec, R.maxv);
        store_ivec4(reinterpret_cast<int*>(p + S::kMaxS * sec), R.maxs);
      }
      if constexpr (MIN) {
        store_vec<4>(p + S::kMinV * sec, R.minv);
        store_ivec4(reinterpret_cast<int*>(p + S::kMinS * sec), R.mins);
      }
    }
  }
}

// One wave per long row: its chunk records merged in chunk order (ascending slots), then the row's epilogue.
template <bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256)
pna_combine_kernel(const PnaArgs A, int n_long, int n_chunks, const int* __restrict__ long_row,
                   const int* __restrict__ long_chunk_ptr, const int* __restrict__ chunk_begin,
                   const int* __restrict__ chunk_end, const float* __restrict__ partial) {
  using S = Sections<M1, M2, MAX, MIN>;
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int64_t sec = (int64_t)n_chunks * A.d;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < A.d; c += kWave * 4) {
      Rec R;
      rec_init<M1, M2, MAX, MIN>(R);
      for (int ch = c0; ch < c1; ++ch) {
        const float* p = partial + (int64_t)ch * A.d + c;
        const int nb = chunk_end[ch] - chunk_begin[ch];
        float v[4], q[4], k[4];
        int s[4];
        if constexpr (M1) {
          load_vec<4>(v, p + S::kS * sec);
#pragma unroll
          for (int i = 0; i < 4; ++i) R.s[i] += v[i];
        }
        if constexpr (M2) {
          load_vec<4>(v, p + S::kDev * sec);
          load_vec<4>(q, p + S::kSq * sec);
          load_vec<4>(k, p + S::kShift * sec);
#pragma unroll
          for (int i = 0; i < 4; ++i) merge_moments(R.n, R.dev[i], R.sq[i], R.shift[i], nb, v[i], q[i], k[i]);
        }
        if constexpr (MAX) {
          load_vec<4>(v, p + S::kMaxV * sec);
          load_ivec4(s, reinterpret_cast<const int*>(p + S::kMaxS * sec));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool take = v[i] > R.maxv[i];
            R.maxv[i] = take ? v[i] : R.maxv[i];
            R.maxs[i] = take ? s[i] : R.maxs[i];
          }
        }
        if constexpr (MIN) {
          load_vec<4>(v, p + S::kMinV * sec);
          load_ivec4(s, reinterpret_cast<const int*>(p + S::kMinS * sec));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool take = v[i] < R.minv[i];
            R.minv[i] = take ? v[i] : R.minv[i];
            R.mins[i] = take ? s[i] : R.mins[i];
          }
        }
        R.n += nb;
      }
      pna_store<M1, M2, MAX, MIN>(A, row, c, R.n, R, true, 0, 1);
    }
  }
}

template <int G, bool M1, bool M2, bool MAX, bool MIN>
int launch_pna(const PnaArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  // one row per wave, uncapped grid: rows differ in length and the dispatcher balances fresh blocks (as spmm.hip)
  pna_fwd_kernel<G, M1, M2, MAX, MIN><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("pna_fwd_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    pna_chunk_kernel<G, M1, M2, MAX, MIN><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                                sp->partial);
    RGBX_CHECK_LAUNCH("pna_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    pna_combine_kernel<M1, M2, MAX, MIN><<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->n_chunks, sp->long_row,
                                                               sp->long_chunk_ptr, sp->chunk_begin, sp->chunk_end,
                                                               sp->partial);
    RGBX_CHECK_LAUNCH("pna_combine_kernel");
  }
  return RGBX_OK;
}

#define RGBX_PNA_CASE(K) \
  case K: return launch_pna<G, ((K) & 1) != 0, ((K) & 2) != 0, ((K) & 4) != 0, ((K) & 8) != 0>(A, sp, s);

template <int G>
int launch_pna_which(const PnaArgs& A, int key, const rgbx_row_split_t* sp, hipStream_t s) {
  switch (key) {  // bit 0: sum / mean, bit 1: var / std, bit 2: max, bit 3: min
    RGBX_PNA_CASE(1) RGBX_PNA_CASE(2) RGBX_PNA_CASE(3) RGBX_PNA_CASE(4) RGBX_PNA_CASE(5)
    RGBX_PNA_CASE(6) RGBX_PNA_CASE(7) RGBX_PNA_CASE(8) RGBX_PNA_CASE(9) RGBX_PNA_CASE(10)
    RGBX_PNA_CASE(11) RGBX_PNA_CASE(12) RGBX_PNA_CASE(13) RGBX_PNA_CASE(14) RGBX_PNA_CASE(15)
  }
  return fail(RGBX_E_ARG, "pna_fwd: no aggregator wanted");
}
#undef RGBX_PNA_CASE

// ---- backward ------------------------------------------------------------------------------------------------------------

struct PnaBwdArgs {
  const int* rowptr;  // source pass: the transposed CSR (rows = sources, col = targets); edge pass: the forward CSR
  const int* col;
  const int* t2f;
  const float* b;
  const float* c;
  const float* A;
  const float* B;
  const float* ge[2];  // the extremum cotangents that are present, max before min
  const int* ae[2];    // their winning slots
  int64_t ldb, ldc, ldA, ldB, ldge[2], ldae[2];
  float* g;  // g_b [N, ldg] or g_c [nnz, ldg]
  int64_t ldg;
  int N, d;
  int skip_longer;
};

// Slots in flight per group, by the 16-byte fragments a slot loads (A: one; B: its own row and the c row; an extremum:
// cotangent + arg): four for <= 2, two for <= 4, one beyond.
template <bool TA, bool TB, int NE>
constexpr int src_depth() {
  constexpr int L = (TA ? 1 : 0) + (TB ? 2 : 0) + 2 * NE;
  return L <= 2 ? 4 : (L <= 4 ? 2 : 1);
}

// acc += bracket over the slots [start, end) of a transposed row whose own b fragment is bj; groups folded on return.
template <int G, bool TA, bool TB, int NE>
__device__ __forceinline__ void src_slots(const PnaBwdArgs& P, int start, int end, int c, bool active, int lane, int g,
                                          const float (&bj)[4], float (&acc)[4]) {
  constexpr int NG = kWave / G;
  constexpr int U = src_depth<TA, TB, NE>();
  constexpr int NE1 = NE > 0 ? NE : 1;
  const bool need_slot = NE > 0 || (TB && P.c);
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int mycol = 0, myfwd = -2;
    if (lane < n) {
      mycol = P.col[base + lane];
      if (need_slot) myfwd = P.t2f[base + lane];
    }
    for (int k = 0; k < n; k += NG * U) {
      float va[U][4], vb[U][4], vc[U][4], ve[NE1][U][4];
      int we[NE1][U][4];
      int fs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int tgt = __shfl(mycol, idx & 63);
        fs[u] = __shfl(myfwd, idx & 63);
        const bool ok = active && idx < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          va[u][i] = vb[u][i] = vc[u][i] = 0.f;
#pragma unroll
          for (int e = 0; e < NE1; ++e) { ve[e][u][i] = 0.f; we[e][u][i] = -1; }
        }
        if (ok) {
          if constexpr (TA) load_vec<4>(va[u], P.A + (int64_t)tgt * P.ldA + c);
          if constexpr (TB) {
            load_vec<4>(vb[u], P.B + (int64_t)tgt * P.ldB + c);
            if (P.c) load_vec<4>(vc[u], P.c + (int64_t)fs[u] * P.ldc + c);
          }
#pragma unroll
          for (int e = 0; e < NE; ++e) {
            load_ivec4(we[e][u], P.ae[e] + (int64_t)tgt * P.ldae[e] + c);
            load_vec<4>(ve[e][u], P.ge[e] + (int64_t)tgt * P.ldge[e] + c);
          }
        } else {
          fs[u] = -2;  // matches no arg (arg >= -1)
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (TA) acc[i] += va[u][i];
          if constexpr (TB) acc[i] = fmaf(vb[u][i], bj[i] + vc[u][i], acc[i]);  // a slot past the end: B = 0
#pragma unroll
          for (int e = 0; e < NE; ++e) acc[i] += we[e][u][i] == fs[u] ? ve[e][u][i] : 0.f;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
}

template <int G, bool TA, bool TB, int NE, bool CHUNK>
__global__ void __launch_bounds__(256)
pna_bwd_src_kernel(const PnaBwdArgs P, int n_items, const int* __restrict__ chunk_begin,
                   const int* __restrict__ chunk_end, const int* __restrict__ chunk_row, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < P.d;
  const int wpb = blockDim.x >> 6;
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    int row, start, end;
    if constexpr (CHUNK) {
      row = chunk_row[item];
      start = __builtin_amdgcn_readfirstlane(chunk_begin[item]);
      end = __builtin_amdgcn_readfirstlane(chunk_end[item]);
    } else {
      row = item;
      start = __builtin_amdgcn_readfirstlane(P.rowptr[row]);
      end = __builtin_amdgcn_readfirstlane(P.rowptr[row + 1]);
      if (P.skip_longer > 0 && end - start > P.skip_longer) continue;
    }
    float bj[4] = {0.f, 0.f, 0.f, 0.f}, acc[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (TB) {
      if (active) load_vec<4>(bj, P.b + (int64_t)row * P.ldb + c);
    }
    src_slots<G, TA, TB, NE>(P, start, end, c, active, lane, g, bj, acc);
    if (g == 0 && active) {
      if constexpr (CHUNK) store_vec<4>(partial + (int64_t)item * P.d + c, acc);
      else nt_store(P.g + (int64_t)row * P.ldg + c, acc);
    }
  }
}

// One wave per long row: chunk contributions added in chunk order.
__global__ void __launch_bounds__(256)
pna_bwd_combine_kernel(const PnaBwdArgs P, int n_long, const int* __restrict__ long_row,
                       const int* __restrict__ long_chunk_ptr, const float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < P.d; c += kWave * 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = c0; ch < c1; ++ch) {
        float p[4];
        load_vec<4>(p, partial + (int64_t)ch * P.d + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += p[i];
      }
      store_vec<4>(P.g + (int64_t)row * P.ldg + c, acc);
    }
  }
}

template <int G, bool TA, bool TB, int NE>
int launch_src(const PnaBwdArgs& P, const rgbx_row_split_t* sp, hipStream_t s) {
  int64_t rb = cdiv(P.N, 4);
  if (rb > kMaxGrid) rb = kMaxGrid;
  pna_bwd_src_kernel<G, TA, TB, NE, false><<<(int)rb, 256, 0, s>>>(P, P.N, nullptr, nullptr, nullptr, nullptr);
  RGBX_CHECK_LAUNCH("pna_bwd_src_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    pna_bwd_src_kernel<G, TA, TB, NE, true><<<(int)cb, 256, 0, s>>>(P, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                                   sp->chunk_row, sp->partial);
    RGBX_CHECK_LAUNCH("pna_bwd_src_kernel (chunks)");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    pna_bwd_combine_kernel<<<(int)lb, 256, 0, s>>>(P, sp->n_long, sp->long_row, sp->long_chunk_ptr, sp->partial);
    RGBX_CHECK_LAUNCH("pna_bwd_combine_kernel");
  }
  return RGBX_OK;
}

#define RGBX_PNA_SRC_CASE(K) \
  case K: return launch_src<G, ((K) & 1) != 0, ((K) & 2) != 0, ((K) >> 2)>(P, sp, s);

template <int G>
int launch_src_which(const PnaBwdArgs& P, int key, const rgbx_row_split_t* sp, hipStream_t s) {
  switch (key) {  // bit 0: A, bit 1: B, bits 2-3: the number of extremum terms
    RGBX_PNA_SRC_CASE(1) RGBX_PNA_SRC_CASE(2) RGBX_PNA_SRC_CASE(3) RGBX_PNA_SRC_CASE(4) RGBX_PNA_SRC_CASE(5)
    RGBX_PNA_SRC_CASE(6) RGBX_PNA_SRC_CASE(7) RGBX_PNA_SRC_CASE(8) RGBX_PNA_SRC_CASE(9) RGBX_PNA_SRC_CASE(10)
    RGBX_PNA_SRC_CASE(11)
  }
  return fail(RGBX_E_ARG, "pna_bwd_src: no term given");
}
#undef RGBX_PNA_SRC_CASE

// Edge pass over the forward CSR (row = target i): the row's A, B, Gmax, argmax, Gmin, argmin fragments stay in
// registers (a term that is absent: zeros, and an arg no slot has); per slot the b row of the source is gathered, the c
// row streamed and the g_c row stored. Nothing is summed over slots. The chunk items only balance the hub rows.
template <int G, bool CHUNK>
__global__ void __launch_bounds__(256)
pna_bwd_edge_kernel(const PnaBwdArgs P, int n_items, const int* __restrict__ chunk_begin,
                    const int* __restrict__ chunk_end, const int* __restrict__ chunk_row) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < P.d;
  const int wpb = blockDim.x >> 6;
  for (int item = blockIdx.x * wpb + (threadIdx.x >> 6); item < n_items; item += gridDim.x * wpb) {
    int row, start, end;
    if constexpr (CHUNK) {
      row = chunk_row[item];
      start = __builtin_amdgcn_readfirstlane(chunk_begin[item]);
      end = __builtin_amdgcn_readfirstlane(chunk_end[item]);
    } else {
      row = item;
      start = __builtin_amdgcn_readfirstlane(P.rowptr[row]);
      end = __builtin_amdgcn_readfirstlane(P.rowptr[row + 1]);
      if (P.skip_longer > 0 && end - start > P.skip_longer) continue;
    }
    if (start == end) continue;
    float ra[4], rb[4], re[2][4];
    int rs[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = rb[i] = re[0][i] = re[1][i] = 0.f;
      rs[0][i] = rs[1][i] = -2;
    }
    if (active) {
      if (P.A) load_vec<4>(ra, P.A + (int64_t)row * P.ldA + c);
      if (P.B) load_vec<4>(rb, P.B + (int64_t)row * P.ldB + c);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (P.ge[e]) {
          load_vec<4>(re[e], P.ge[e] + (int64_t)row * P.ldge[e] + c);
          load_ivec4(rs[e], P.ae[e] + (int64_t)row * P.ldae[e] + c);
        }
      }
    }
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int mycol = lane < n ? P.col[base + lane] : 0;
      for (int k = 0; k < n; k += NG * U) {
        float bv[U][4], cv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          const int src = __shfl(mycol, idx & 63);
#pragma unroll
          for (int i = 0; i < 4; ++i) bv[u][i] = cv[u][i] = 0.f;
          if (active && idx < n && P.B) {  // u is read by the B term alone
            load_vec<4>(bv[u], P.b + (int64_t)src * P.ldb + c);
            load_vec<4>(cv[u], P.c + (int64_t)(base + idx) * P.ldc + c);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int idx = k + u * NG + g;
          if (active && idx < n) {
            const int p = base + idx;
            float gc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float t = fmaf(rb[i], bv[u][i] + cv[u][i], ra[i]);
              t += rs[0][i] == p ? re[0][i] : 0.f;
              t += rs[1][i] == p ? re[1][i] : 0.f;
              gc[i] = t;
            }
            store_vec<4>(P.g + (int64_t)p * P.ldg + c, gc);
          }
        }
      }
    }
  }
}

template <int G>
int launch_edge(const PnaBwdArgs& P, const rgbx_row_split_t* sp, hipStream_t s) {
  int64_t rb = cdiv(P.N, 4);
  if (rb > kMaxGrid) rb = kMaxGrid;
  pna_bwd_edge_kernel<G, false><<<(int)rb, 256, 0, s>>>(P, P.N, nullptr, nullptr, nullptr);
  RGBX_CHECK_LAUNCH("pna_bwd_edge_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    pna_bwd_edge_kernel<G, true><<<(int)cb, 256, 0, s>>>(P, sp->n_chunks, sp->chunk_begin, sp->chunk_end, sp->chunk_row);
    RGBX_CHECK_LAUNCH("pna_bwd_edge_kernel (chunks)");
  }
  return RGBX_OK;
}

const rgbx_row_split_t* usable_split(const rgbx_row_split_t* split) {
  return (split && split->threshold > 0 && split->n_chunks > 0) ? split : nullptr;
}

bool plan_ok(const rgbx_row_split_t* sp) { return sp->n_long > 0 && sp->chunk_begin && sp->chunk_end && sp->chunk_row; }

bool complete_split(const rgbx_row_split_t* sp) {
  return plan_ok(sp) && sp->long_row && sp->long_chunk_ptr && sp->partial && aligned16(sp->partial);
}

bool vec_ok(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

// The backward terms of both passes into P; RGBX_OK or the argument error.
int take_terms(const rgbx_pna_grad_t& t, int64_t d, const void* out, const char* name, PnaBwdArgs* P) {
  if ((t.gmax != nullptr) != (t.argmax != nullptr) || (t.gmin != nullptr) != (t.argmin != nullptr))
    return fail(RGBX_E_ARG, "%s: an extremum term needs both its cotangent and its arg", name);
  if (!t.A && !t.B && !t.gmax && !t.gmin) return fail(RGBX_E_ARG, "%s: no term given", name);
  const void* ptrs[6] = {t.A, t.B, t.gmax, t.argmax, t.gmin, t.argmin};
  const int64_t lds[6] = {t.ld_A, t.ld_B, t.ld_gmax, t.ld_argmax, t.ld_gmin, t.ld_argmin};
  for (int i = 0; i < 6; ++i) {
    if (ptrs[i] && lds[i] < d) return fail(RGBX_E_ARG, "%s: leading dimension < d", name);
    if (ptrs[i] && ptrs[i] == out) return fail(RGBX_E_ARG, "%s: the output must not alias an input", name);
  }
  for (int i = 0; i < 6; ++i)
    if (ptrs[i] && !vec_ok(ptrs[i], lds[i]))
      return fail(RGBX_E_ALIGN, "%s: every input must be 16-byte aligned with ld %% 4 == 0", name);
  P->A = t.A; P->ldA = t.ld_A; P->B = t.B; P->ldB = t.ld_B;
  int e = 0;
  if (t.gmax) { P->ge[e] = t.gmax; P->ldge[e] = t.ld_gmax; P->ae[e] = t.argmax; P->ldae[e] = t.ld_argmax; ++e; }
  if (t.gmin) { P->ge[e] = t.gmin; P->ldge[e] = t.ld_gmin; P->ae[e] = t.argmin; P->ldae[e] = t.ld_argmin; ++e; }
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

#define RGBX_BY_LANES(FN, ...)                    \
  do {                                            \
    const int lanes_ = (int)(d / 4);              \
    if (lanes_ <= 1) return FN<1>(__VA_ARGS__);   \
    if (lanes_ <= 2) return FN<2>(__VA_ARGS__);   \
    if (lanes_ <= 4) return FN<4>(__VA_ARGS__);   \
    if (lanes_ <= 8) return FN<8>(__VA_ARGS__);   \
    if (lanes_ <= 16) return FN<16>(__VA_ARGS__); \
    if (lanes_ <= 32) return FN<32>(__VA_ARGS__); \
    return FN<64>(__VA_ARGS__);                   \
  } while (0)

extern "C" int rgbx_pna_supported(int64_t d, int64_t F) {
  return d >= 4 && d % 4 == 0 && d <= 256 && F >= 4 && F % 4 == 0 && d % F == 0;
}

extern "C" int rgbx_pna_partial_words(int64_t n_chunks, int64_t d, int which, int64_t* words) {
  if (!words) return fail(RGBX_E_ARG, "pna_partial_words: null pointer");
  if (n_chunks < 0 || d < 0) return fail(RGBX_E_ARG, "pna_partial_words: negative size");
  if (which <= 0 || which > RGBX_MULTI_ALL) return fail(RGBX_E_ARG, "pna_partial_words: `which` names no aggregator");
  *words = n_chunks * d * sections_of(which);
  return RGBX_OK;
}

extern "C" int rgbx_pna_fwd_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b,
                                int64_t ldb, const float* c, int64_t ldc, const float* avg_deg, int which,
                                const int32_t* aggr_order, const int32_t* scalers, int n_scalers,
                                const rgbx_pna_out_t* out, int64_t N, int64_t d, int64_t F,
                                const rgbx_row_split_t* split, int64_t partial_words, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "pna_fwd: negative size");
  if (!rowptr || !col || !b || !avg_deg || !out || !scalers) return fail(RGBX_E_ARG, "pna_fwd: null pointer");
  const rgbx_pna_out_t o = *out;
  if (!o.out) return fail(RGBX_E_ARG, "pna_fwd: null pointer (out)");
  if (which <= 0 || which > RGBX_MULTI_ALL) return fail(RGBX_E_ARG, "pna_fwd: no aggregator wanted (`which` names none)");
  if (n_scalers < 1 || n_scalers > kMaxScalers)
    return fail(RGBX_E_ARG, "pna_fwd: no scaler given, or more than %d (got %d)", kMaxScalers, n_scalers);
  for (int s = 0; s < n_scalers; ++s)
    if (scalers[s] < RGBX_PNA_IDENTITY || scalers[s] > RGBX_PNA_INVERSE_LINEAR)
      return fail(RGBX_E_ARG, "pna_fwd: scaler %d is none of RGBX_PNA_*", (int)scalers[s]);
  if ((o.argmax && !(which & RGBX_MULTI_MAX)) || (o.argmin && !(which & RGBX_MULTI_MIN)))
    return fail(RGBX_E_ARG, "pna_fwd: arg wanted without its extremum");
  if (o.mean && !(which & (RGBX_MULTI_SUM | RGBX_MULTI_MEAN | RGBX_MULTI_VAR | RGBX_MULTI_STD)))
    return fail(RGBX_E_ARG, "pna_fwd: the raw mean is kept only beside sum, mean, var or std");
  if ((o.var || o.std) && !(which & (RGBX_MULTI_VAR | RGBX_MULTI_STD)))
    return fail(RGBX_E_ARG, "pna_fwd: the raw var / std is kept only beside var or std");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "pna_fwd: N exceeds int32");
  if (!rgbx_pna_supported(d, F))
    return fail(RGBX_E_SHAPE, "pna_fwd: needs d %% 4 == 0, 4 <= d <= 256, F %% 4 == 0 and F dividing d (got d = %lld, "
                "F = %lld); pad the towers or cut d at tower boundaries", (long long)d, (long long)F);
  // output positions: the order given, or ascending bits
  PnaArgs A{};
  int n_aggr = 0;
  for (int k = 0; k < 6; ++k) A.pos[k] = -1;
  if (aggr_order) {
    int seen = 0;
    while (seen != which) {
      const int w = aggr_order[n_aggr];
      int idx = -1;
      for (int k = 0; k < 6; ++k) if (w == (1 << k)) idx = k;
      if (idx < 0 || !(which & w) || (seen & w))
        return fail(RGBX_E_ARG, "pna_fwd: aggr_order must list every bit of `which` once");
      A.pos[idx] = n_aggr++;
      seen |= w;
    }
  } else {
    for (int k = 0; k < 6; ++k) if (which & (1 << k)) A.pos[k] = n_aggr++;
  }
  const int64_t wide = (d / F) * n_scalers * n_aggr * F;
  if (ldb < d || (c && ldc < d) || (a && lda < d) || o.ld_out < wide)
    return fail(RGBX_E_ARG, "pna_fwd: leading dimension < d (out: < T * S * A * F)");
  const void* ptrs[5] = {o.mean, o.std, o.var, o.argmax, o.argmin};
  const int64_t lds[5] = {o.ld_mean, o.ld_std, o.ld_var, o.ld_argmax, o.ld_argmin};
  for (int i = 0; i < 5; ++i)
    if (ptrs[i] && lds[i] < d) return fail(RGBX_E_ARG, "pna_fwd: leading dimension < d");
  if ((const void*)o.out == (const void*)b || (c && (const void*)o.out == (const void*)c))
    return fail(RGBX_E_ARG, "pna_fwd: out must not alias an input");
  if (!vec_ok(b, ldb) || (c && !vec_ok(c, ldc)) || (a && !vec_ok(a, lda)))
    return fail(RGBX_E_ALIGN, "pna_fwd: a, b, c must be 16-byte aligned with ld %% 4 == 0");
  if (!vec_ok(o.out, o.ld_out)) return fail(RGBX_E_ALIGN, "pna_fwd: out must be 16-byte aligned with ld %% 4 == 0");
  for (int i = 0; i < 5; ++i)
    if (ptrs[i] && !vec_ok(ptrs[i], lds[i]))
      return fail(RGBX_E_ALIGN, "pna_fwd: every kept matrix must be 16-byte aligned with ld %% 4 == 0");
  if ((reinterpret_cast<uintptr_t>(avg_deg) & 3u) != 0) return fail(RGBX_E_ALIGN, "pna_fwd: avg_deg must be 4-byte aligned");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "pna_fwd: incomplete row-split plan");
  const int64_t need_words = sp ? (int64_t)sp->n_chunks * d * sections_of(which | (o.mean ? RGBX_MULTI_MEAN : 0)) : 0;
  if (partial_words < need_words)
    return fail(RGBX_E_WS, "pna_fwd: split->partial holds %lld words, rgbx_pna_partial_words asks for %lld",
                (long long)partial_words, (long long)need_words);
  A.rowptr = rowptr; A.col = col; A.b = b; A.c = c; A.a = a; A.ldb = ldb; A.ldc = ldc; A.lda = lda;
  A.avg_deg = avg_deg; A.o = o; A.N = (int)N; A.d = (int)d; A.F = (int)F; A.n_aggr = n_aggr; A.n_scalers = n_scalers;
  for (int s = 0; s < kMaxScalers; ++s) A.scaler[s] = s < n_scalers ? scalers[s] : 0;
  A.skip_longer = sp ? sp->threshold : 0;
  const int key = ((which & (RGBX_MULTI_SUM | RGBX_MULTI_MEAN)) || o.mean ? 1 : 0) |
                  ((which & (RGBX_MULTI_VAR | RGBX_MULTI_STD)) ? 2 : 0) | ((which & RGBX_MULTI_MAX) ? 4 : 0) |
                  ((which & RGBX_MULTI_MIN) ? 8 : 0);
  hipStream_t s = (hipStream_t)stream;
  RGBX_BY_LANES(launch_pna_which, A, key, sp, s);
}

extern "C" int rgbx_pna_bwd_src_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f, const float* b,
                                    int64_t ldb, const float* c, int64_t ldc, const rgbx_pna_grad_t* terms, float* g_b,
                                    int64_t ldgb, int64_t N, int64_t d, const rgbx_row_split_t* split,
                                    rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "pna_bwd_src: negative size");
  if (!rowptr_t || !col_t || !terms || !g_b) return fail(RGBX_E_ARG, "pna_bwd_src: null pointer");
  const rgbx_pna_grad_t t = *terms;
  PnaBwdArgs P{};
  if (int rc = take_terms(t, d, g_b, "pna_bwd_src", &P)) return rc;
  const int ne = (t.gmax ? 1 : 0) + (t.gmin ? 1 : 0);
  if ((ne > 0 || (t.B && c)) && !t2f) return fail(RGBX_E_ARG, "pna_bwd_src: null pointer (t2f)");
  if (t.B && !b) return fail(RGBX_E_ARG, "pna_bwd_src: the B term needs b");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "pna_bwd_src: N exceeds int32");
  if (!rgbx_pna_supported(d, 4))
    return fail(RGBX_E_SHAPE, "pna_bwd_src: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld)", (long long)d);
  if (ldgb < d || (t.B && ldb < d) || (t.B && c && ldc < d)) return fail(RGBX_E_ARG, "pna_bwd_src: leading dimension < d");
  if ((const void*)g_b == (const void*)b || (c && (const void*)g_b == (const void*)c))
    return fail(RGBX_E_ARG, "pna_bwd_src: the output must not alias an input");
  if (!vec_ok(g_b, ldgb) || (t.B && !vec_ok(b, ldb)) || (t.B && c && !vec_ok(c, ldc)))
    return fail(RGBX_E_ALIGN, "pna_bwd_src: b, c, g_b must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "pna_bwd_src: incomplete row-split plan");
  P.rowptr = rowptr_t; P.col = col_t; P.t2f = t2f; P.b = b; P.ldb = ldb; P.c = t.B ? c : nullptr; P.ldc = ldc;
  P.g = g_b; P.ldg = ldgb; P.N = (int)N; P.d = (int)d; P.skip_longer = sp ? sp->threshold : 0;
  const int key = (t.A ? 1 : 0) | (t.B ? 2 : 0) | (ne << 2);
  hipStream_t s = (hipStream_t)stream;
  RGBX_BY_LANES(launch_src_which, P, key, sp, s);
}

extern "C" int rgbx_pna_bwd_edge_f32(const int32_t* rowptr, const int32_t* col, const float* b, int64_t ldb,
                                     const float* c, int64_t ldc, const rgbx_pna_grad_t* terms, float* g_c, int64_t ldgc,
                                     int64_t N, int64_t d, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "pna_bwd_edge: negative size");
  if (!rowptr || !col || !terms || !g_c) return fail(RGBX_E_ARG, "pna_bwd_edge: null pointer");
  const rgbx_pna_grad_t t = *terms;
  PnaBwdArgs P{};
  if (int rc = take_terms(t, d, g_c, "pna_bwd_edge", &P)) return rc;
  if (t.B && (!b || !c)) return fail(RGBX_E_ARG, "pna_bwd_edge: the B term needs b and c");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "pna_bwd_edge: N exceeds int32");
  if (!rgbx_pna_supported(d, 4))
    return fail(RGBX_E_SHAPE, "pna_bwd_edge: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld)", (long long)d);
  if (ldgc < d || (t.B && (ldb < d || ldc < d))) return fail(RGBX_E_ARG, "pna_bwd_edge: leading dimension < d");
  if ((const void*)g_c == (const void*)b || (const void*)g_c == (const void*)c)
    return fail(RGBX_E_ARG, "pna_bwd_edge: the output must not alias an input");
  if (!vec_ok(g_c, ldgc) || (t.B && (!vec_ok(b, ldb) || !vec_ok(c, ldc))))
    return fail(RGBX_E_ALIGN, "pna_bwd_edge: b, c, g_c must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !plan_ok(sp)) return fail(RGBX_E_ARG, "pna_bwd_edge: incomplete row-split plan");
  if (t.gmax) { P.ge[0] = t.gmax; P.ldge[0] = t.ld_gmax; P.ae[0] = t.argmax; P.ldae[0] = t.ld_argmax; }
  else { P.ge[0] = nullptr; P.ae[0] = nullptr; }
  if (t.gmin) { P.ge[1] = t.gmin; P.ldge[1] = t.ld_gmin; P.ae[1] = t.argmin; P.ldae[1] = t.ld_argmin; }
  else { P.ge[1] = nullptr; P.ae[1] = nullptr; }
  P.rowptr = rowptr; P.col = col; P.b = b; P.ldb = ldb; P.c = c; P.ldc = ldc;
  P.g = g_c; P.ldg = ldgc; P.N = (int)N; P.d = (int)d; P.skip_longer = sp ? sp->threshold : 0;
  hipStream_t s = (hipStream_t)stream;
  RGBX_BY_LANES(launch_edge, P, sp, s);
}
